// Driver of tests/golden/make_bilateral_golden.py (ours; the generator compiles it against the reference's ITMLib CPU sources,
// which it reads in place).  Runs the reference's view builder and ITMBasicEngine on the CPU with useBilateralFilter = true.
//
//   bilateral_ref_driver kernel <in.bin> <out.bin>
//       in: int32 W, H; int16 depth[H * W] (millimetres).  ITMViewBuilder_CPU::UpdateView(..., useBilateralFilter = true) ->
//       chunk "depth_f" (view->depth).
//   bilateral_ref_driver engine <in.bin> <out.bin> <useApproximateRaycast: 0 | 1> <given | track | reloc>
//       in: a sequence as oracle/tsdf_ref.py writes it.  Per frame: "M", "invM", the engine dump of oracle/ref_driver.cpp (counts,
//       visible_ids, vis_type_nz, hash, vba_crc, depth_f, minmax, raycast, icp_points, icp_normals), "age" (age_pointCloud),
//       "live" (runRaycast(NULL, NULL)'s colour image) and "img1" (GetImage(ORIGINAL_DEPTH)).  reloc (given poses,
//       FAILUREMODE_RELOCALISE): also "code", the fern code of view->depth by the calls of Relocaliser.h:51-61 with the engine's
//       own relocaliser's ferns, and once "ferns_xy" (int32 pairs) and "ferns_thr" (float32).
//   Both end with the chunk "expf_calls" (int64): how many exponentials went through the expf below.
//
// THE PINNED expf.  filterDepth's exp(float) is expf in this build.  glibc's expf is not correctly rounded, and a device cannot
// reproduce its table-driven result; with -DGPS_PIN_EXPF this file defines expf itself -- correctly rounded, through long double
// -- and a definition in the program wins over libm's at link time.  The device computes the exponential in double and rounds
// once; on 2e8 arguments in [-110, 0] the two routes agree everywhere.  Without the macro the driver is the plain-glibc
// reference: the generator runs both and records how many filtered pixels differ, as data.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int64_t g_expf_calls = 0;
#ifdef GPS_PIN_EXPF
extern "C" float expf(float x) noexcept {
    g_expf_calls++;
    return (float)expl((long double)x);
}
#endif

#define private public
#define protected public
#include "ITMLib/ITMLibDefines.h"
#include "ITMLib/Core/ITMBasicEngine.h"
#include "ITMLib/Engines/ViewBuilding/CPU/ITMViewBuilder_CPU.h"
#include "ITMLib/Objects/RenderStates/ITMRenderState_VH.h"
#include "FernRelocLib/Relocaliser.h"
#undef private
#undef protected

using namespace ITMLib;

static FILE* g_out;

static void chunk(const char* name, int frame, const void* data, int64_t nbytes) {
    char nm[32];
    memset(nm, 0, sizeof(nm));
    strncpy(nm, name, 31);
    fwrite(nm, 1, 32, g_out);
    int32_t f = frame;
    fwrite(&f, 4, 1, g_out);
    fwrite(&nbytes, 8, 1, g_out);
    if (nbytes) fwrite(data, 1, (size_t)nbytes, g_out);
}

static uint32_t crc32_update(uint32_t crc, const unsigned char* p, size_t n) {
    static uint32_t table[256];
    static bool init = false;
    if (!init) {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            table[i] = c;
        }
        init = true;
    }
    crc = ~crc;
    for (size_t i = 0; i < n; i++) crc = table[(crc ^ p[i]) & 0xFF] ^ (crc >> 8);
    return ~crc;
}

struct Header {
    int32_t magic, W, H, nframes, nfree, dump_vba_every;
    float fx, fy, cx, cy, voxel, mu, vfmin, vfmax;
};

typedef ITMBasicEngine<ITMVoxel, ITMVoxelIndex> Engine;

static int run_kernel(FILE* in) {
    int32_t wh[2];
    if (fread(wh, 4, 2, in) != 2) return 3;
    const int W = wh[0], H = wh[1], P = W * H;
    ITMRGBDCalib calib;
    calib.intrinsics_rgb.SetFrom(W, H, 100.0f, 100.0f, W * 0.5f, H * 0.5f);
    calib.intrinsics_d = calib.intrinsics_rgb;
    calib.disparityCalib.SetStandard();
    Vector2i dims(W, H);
    ITMUChar4Image rgb(dims, true, false);
    ITMShortImage depth(dims, true, false);
    rgb.Clear();
    if (fread(depth.GetData(MEMORYDEVICE_CPU), 2, P, in) != (size_t)P) return 3;
    ITMViewBuilder_CPU builder(calib);
    ITMView* view = NULL;
    builder.UpdateView(&view, &rgb, &depth, true);
    chunk("depth_f", 0, view->depth->GetData(MEMORYDEVICE_CPU), (int64_t)P * 4);
    return 0;
}

static int run_engine(FILE* in, bool approx, const std::string& mode) {
    Header h;
    if (fread(&h, sizeof(h), 1, in) != 1 || h.magic != 0x47505331 || h.nfree != 0) return 2;
    const int P = h.W * h.H;
    const bool track = mode == "track", reloc = mode == "reloc";

    ITMRGBDCalib calib;
    calib.intrinsics_rgb.SetFrom(h.W, h.H, h.fx, h.fy, h.cx, h.cy);
    calib.intrinsics_d = calib.intrinsics_rgb;
    calib.disparityCalib.SetStandard();
    ITMLibSettings* settings = new ITMLibSettings();
    settings->deviceType = ITMLibSettings::DEVICE_CPU;
    settings->createMeshingEngine = false;
    settings->useApproximateRaycast = approx;
    settings->useBilateralFilter = true;
    if (reloc) settings->behaviourOnFailure = ITMLibSettings::FAILUREMODE_RELOCALISE;
    settings->sceneParams.voxelSize = h.voxel;
    settings->sceneParams.mu = h.mu;
    settings->sceneParams.viewFrustum_min = h.vfmin;
    settings->sceneParams.viewFrustum_max = h.vfmax;
    Vector2i dims(h.W, h.H);
    Engine* eng = new Engine(settings, calib, dims, dims);
    if (!track) eng->turnOffTracking();

    std::vector<ITMUChar4Image*> rgbs(h.nframes);
    std::vector<ITMShortImage*> depths(h.nframes);
    std::vector<ORUtils::Matrix4<float>*> poses(h.nframes);
    for (int f = 0; f < h.nframes; f++) {
        rgbs[f] = new ITMUChar4Image(dims, true, false);
        depths[f] = new ITMShortImage(dims, true, false);
        float c2w[16];
        if (fread(rgbs[f]->GetData(MEMORYDEVICE_CPU), 4, P, in) != (size_t)P) return 3;
        if (fread(depths[f]->GetData(MEMORYDEVICE_CPU), 2, P, in) != (size_t)P) return 3;
        if (fread(c2w, 4, 16, in) != 16) return 3;
        ORUtils::Matrix4<float>* m = new ORUtils::Matrix4<float>();
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) m->m[c * 4 + r] = c2w[r * 4 + c];
        poses[f] = m;
    }
    eng->gtC2wPoses = poses;
    ITMUChar4Image* out = new ITMUChar4Image(dims, true, false);

    if (reloc) {
        FernRelocLib::FernConservatory* enc = eng->relocaliser->encoding;
        const int n = enc->mNumFerns * enc->mNumDecisions;
        std::vector<int32_t> xy(2 * n);
        std::vector<float> thr(n);
        for (int e = 0; e < n; e++) {
            xy[2 * e] = enc->mEncoders[e].location.x; xy[2 * e + 1] = enc->mEncoders[e].location.y;
            thr[e] = enc->mEncoders[e].threshold;
        }
        chunk("ferns_xy", 0, xy.data(), (int64_t)n * 8);
        chunk("ferns_thr", 0, thr.data(), (int64_t)n * 4);
    }

    for (int f = 0; f < h.nframes; f++) {
        eng->ProcessFrame(rgbs[f], depths[f]);
        ITMTrackingState* ts = eng->GetTrackingState();
        ORUtils::Matrix4<float> M = ts->pose_d->GetM(), invM = ts->pose_d->GetInvM();
        chunk("M", f, M.m, 64);
        chunk("invM", f, invM.m, 64);
        const int32_t age = ts->age_pointCloud;
        chunk("age", f, &age, 4);

        ITMRenderState_VH* rs = (ITMRenderState_VH*)eng->renderState_live;
        ITMScene<ITMVoxel, ITMVoxelIndex>* scene = eng->GetScene();
        int32_t counts[3] = {rs->noVisibleEntries, scene->localVBA.lastFreeBlockId, scene->index.GetLastFreeExcessListId()};
        chunk("counts", f, counts, 12);
        chunk("visible_ids", f, rs->GetVisibleEntryIDs(), (int64_t)rs->noVisibleEntries * 4);
        {
            const unsigned char* vt = rs->GetEntriesVisibleType();
            std::vector<int32_t> nz;
            for (int i = 0; i < ITMVoxelBlockHash::noTotalEntries; i++)
                if (vt[i]) { nz.push_back(i); nz.push_back(vt[i]); }
            chunk("vis_type_nz", f, nz.data(), (int64_t)nz.size() * 4);
        }
        {
            const ITMHashEntry* ht = scene->index.GetEntries();
            const ITMVoxel* vba = scene->localVBA.GetVoxelBlocks();
            std::vector<int32_t> rows;
            uint32_t crc = 0;
            for (int i = 0; i < ITMVoxelBlockHash::noTotalEntries; i++) {
                const ITMHashEntry& e = ht[i];
                if (e.ptr == -2 && e.offset == 0 && e.pos.x == 0 && e.pos.y == 0 && e.pos.z == 0) continue;
                rows.push_back(i); rows.push_back(e.pos.x); rows.push_back(e.pos.y); rows.push_back(e.pos.z);
                rows.push_back(e.offset); rows.push_back(e.ptr);
                if (e.ptr >= 0) {
                    const unsigned char* b = (const unsigned char*)(vba + (size_t)e.ptr * SDF_BLOCK_SIZE3);
                    for (int v = 0; v < SDF_BLOCK_SIZE3; v++) crc = crc32_update(crc, b + v * sizeof(ITMVoxel), 7);  // skip the pad byte
                }
            }
            chunk("hash", f, rows.data(), (int64_t)rows.size() * 4);
            chunk("vba_crc", f, &crc, 4);
        }
        chunk("depth_f", f, eng->GetView()->depth->GetData(MEMORYDEVICE_CPU), (int64_t)P * 4);
        chunk("minmax", f, rs->renderingRangeImage->GetData(MEMORYDEVICE_CPU), (int64_t)P * 8);
        chunk("raycast", f, rs->raycastResult->GetData(MEMORYDEVICE_CPU), (int64_t)P * 16);
        chunk("icp_points", f, ts->pointCloud->locations->GetData(MEMORYDEVICE_CPU), (int64_t)P * 16);
        chunk("icp_normals", f, ts->pointCloud->colours->GetData(MEMORYDEVICE_CPU), (int64_t)P * 16);
        eng->runRaycast(nullptr, nullptr);
        chunk("live", f, eng->renderState_live->raycastImage->GetData(MEMORYDEVICE_CPU), (int64_t)P * 4);
        eng->GetImage(out, ITMMainEngine::InfiniTAM_IMAGE_ORIGINAL_DEPTH);
        chunk("img1", f, out->GetData(MEMORYDEVICE_CPU), (int64_t)P * 4);
        if (reloc) {
            FernRelocLib::Relocaliser<float>* r = eng->relocaliser;
            ORUtils::Image<float> p1(dims, MEMORYDEVICE_CPU), p2(dims, MEMORYDEVICE_CPU);
            FernRelocLib::filterSubsample(eng->GetView()->depth, &p1);
            FernRelocLib::filterSubsample(&p1, &p2);
            FernRelocLib::filterSubsample(&p2, &p1);
            FernRelocLib::filterSubsample(&p1, &p2);
            FernRelocLib::filterGaussian(&p2, &p1, 2.5f);
            std::vector<char> code(r->encoding->getNumFerns());
            r->encoding->computeCode(&p1, code.data());
            chunk("code", f, code.data(), (int64_t)code.size());
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string what = argv[1];
    FILE* in = fopen(argv[2], "rb");
    g_out = fopen(argv[3], "wb");
    if (!in || !g_out) return 2;
    int r;
    if (what == "kernel") r = run_kernel(in);
    else if (what == "engine" && argc >= 6) r = run_engine(in, std::string(argv[4]) == "1", argv[5]);
    else return 2;
    if (r != 0) return r;
    chunk("expf_calls", 0, &g_expf_calls, 8);
    fclose(in);
    fclose(g_out);
    return 0;
}
