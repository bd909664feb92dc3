// Driver of tests/golden/make_reloc_golden.py (ours; the generator compiles it against the reference's FernRelocLib and ORUtils,
// which it reads in place).  Feeds depth frames to two FernRelocLib::Relocaliser<float> -- one asked for k = 1, one for k = 3 --
// and records what they answer, plus the code and the blurred image of every frame computed with the reference's own functions.
//
//   reloc_ref_driver <dir>
//     <dir>/meta.bin    int32 W H numFerns numDecisions nFrames | float32 rangeMin rangeMax threshold |
//                       per frame: int32 harvest sceneId, float32 tx ty tz rx ry rz
//     <dir>/depth.bin   float32 [nFrames, H, W]
//     <dir>/init/       ferns.txt (the table to use), frames.txt and poses.txt of an empty database
//   writes <dir>/codes.bin uint8[n, numFerns], blurred.bin float32[n, h4*w4], res.bin int32[n, 6] (added1 id1 added3 ids3[3]),
//   dist.bin float32[n, 4] (d1 d3[3]), pose.bin float32[n, 32] (M, invM), coeff.bin float32[17], and the k = 1 database's four
//   text files under <dir>/saved/
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "FernRelocLib/Relocaliser.h"

template <class T>
static void dump(const std::string& path, const std::vector<T>& v) {
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(2); }
    fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 2) return 1;
    const std::string dir = std::string(argv[1]) + "/";
    FILE* fm = fopen((dir + "meta.bin").c_str(), "rb");
    if (!fm) return 2;
    int hdr[5];
    float par[3];
    if (fread(hdr, 4, 5, fm) != 5 || fread(par, 4, 3, fm) != 3) return 2;
    const int W = hdr[0], H = hdr[1], numFerns = hdr[2], numDec = hdr[3], n = hdr[4];
    std::vector<int> flags(2 * n);
    std::vector<float> params(6 * n);
    for (int i = 0; i < n; i++)
        if (fread(&flags[2 * i], 4, 2, fm) != 2 || fread(&params[6 * i], 4, 6, fm) != 6) return 2;
    fclose(fm);

    const ORUtils::Vector2<int> size(W, H);
    const ORUtils::Vector2<float> range(par[0], par[1]);
    FernRelocLib::Relocaliser<float> reloc1(size, range, par[2], numFerns, numDec), reloc3(size, range, par[2], numFerns, numDec);
    reloc1.LoadFromDirectory(dir + "init/");
    reloc3.LoadFromDirectory(dir + "init/");
    FernRelocLib::FernConservatory enc(numFerns, size / 32, range, numDec);   // Relocaliser.h:29-30
    enc.LoadFromFile(dir + "init/ferns.txt");

    const int w4 = W / 2 / 2 / 2 / 2, h4 = H / 2 / 2 / 2 / 2;
    ORUtils::Image<float> img(size, MEMORYDEVICE_CPU), p1(size, MEMORYDEVICE_CPU), p2(size, MEMORYDEVICE_CPU);
    std::vector<unsigned char> codes((size_t)n * numFerns);
    std::vector<float> blurred((size_t)n * w4 * h4), dist((size_t)n * 4), pose((size_t)n * 32);
    std::vector<int> res((size_t)n * 6);
    std::vector<char> code(numFerns);
    FILE* fd = fopen((dir + "depth.bin").c_str(), "rb");
    if (!fd) return 2;
    for (int i = 0; i < n; i++) {
        if (fread(img.GetData(MEMORYDEVICE_CPU), 4, (size_t)W * H, fd) != (size_t)W * H) return 2;
        const float* q = &params[6 * i];
        const ORUtils::SE3Pose se3(q[0], q[1], q[2], q[3], q[4], q[5]);
        const ORUtils::Matrix4<float> M = se3.GetM(), invM = se3.GetInvM();
        for (int j = 0; j < 16; j++) { pose[(size_t)i * 32 + j] = M.m[j]; pose[(size_t)i * 32 + 16 + j] = invM.m[j]; }
        // the frame's code and blurred image, by the calls of Relocaliser.h:51-61
        FernRelocLib::filterSubsample(&img, &p1);
        FernRelocLib::filterSubsample(&p1, &p2);
        FernRelocLib::filterSubsample(&p2, &p1);
        FernRelocLib::filterSubsample(&p1, &p2);
        FernRelocLib::filterGaussian(&p2, &p1, 2.5f);
        if (p1.noDims.x != w4 || p1.noDims.y != h4) return 3;
        enc.computeCode(&p1, code.data());
        for (int f = 0; f < numFerns; f++) codes[(size_t)i * numFerns + f] = (unsigned char)code[f];
        for (int j = 0; j < w4 * h4; j++) blurred[(size_t)i * w4 * h4 + j] = p1.GetData(MEMORYDEVICE_CPU)[j];
        int nn1[1], nn3[3];
        float d1[1], d3[3];
        const bool a1 = reloc1.ProcessFrame(&img, &se3, flags[2 * i + 1], 1, nn1, d1, flags[2 * i] != 0);
        const bool a3 = reloc3.ProcessFrame(&img, &se3, flags[2 * i + 1], 3, nn3, d3, flags[2 * i] != 0);
        int* r = &res[(size_t)i * 6];
        r[0] = a1; r[1] = nn1[0]; r[2] = a3; r[3] = nn3[0]; r[4] = nn3[1]; r[5] = nn3[2];
        float* d = &dist[(size_t)i * 4];
        d[0] = d1[0]; d[1] = d3[0]; d[2] = d3[1]; d[3] = d3[2];
    }
    fclose(fd);
    std::vector<float> coeff(17);
    FernRelocLib::createGaussianFilter(17, 2.5f, coeff.data());
    dump(dir + "codes.bin", codes);
    dump(dir + "blurred.bin", blurred);
    dump(dir + "res.bin", res);
    dump(dir + "dist.bin", dist);
    dump(dir + "pose.bin", pose);
    dump(dir + "coeff.bin", coeff);
    reloc1.SaveToDirectory(dir + "saved/");
    return 0;
}
