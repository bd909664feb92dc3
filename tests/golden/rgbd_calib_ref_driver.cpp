// Driver of tests/golden/make_rgbd_calib_golden.py (ours; the generator compiles it against the reference's ITMLib CPU sources,
// which it reads in place).  Runs the reference's view builder and ITMBasicEngine on the CPU with a full ITMRGBDCalib: a colour
// camera of its own size, intrinsics and pose, and a depth calibration of either type.
//
//   rgbd_calib_ref_driver conv <in.bin> <out.bin>
//       in: int32 W, H, type (0 kinect, 1 affine), filter; float a, b, fx_d; int16 raw[H * W].
//       ITMViewBuilder_CPU::UpdateView(..., useBilateralFilter = filter) -> chunk "depth_f" (view->depth).
//   rgbd_calib_ref_driver engine <in.bin> <out.bin>
//       in: Header (below); per frame uchar4 rgb[Hc * Wc], int16 raw[Hd * Wd], float c2w[16] (row major).
//       Once: "calib_txt" (writeRGBDCalib's bytes), "reread" (int32: 1 when readRGBDCalib of that text gives the same struct),
//       "calib" and "calib_inv" (trafo_rgb_to_depth, float[16] each).  Per frame: "M", "invM", "M_rgb" (calib_inv * M_d as
//       IntegrateIntoScene forms it), "age", the engine dump of oracle/ref_driver.cpp (counts, visible_ids, vis_type_nz, hash,
//       vba_crc, depth_f, minmax, raycast, icp_points, icp_normals) and "img0" (GetImage(ORIGINAL_RGB), at the colour size).
//       After the last frame: "vba_last", the voxels (8 bytes each) of every allocated block in table order.
//
// The expf of filterDepth is pinned as in bilateral_ref_driver.cpp (correctly rounded through long double; a definition in the
// program wins over libm's at link time), so that the filtered run has a reference a device can reproduce.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

extern "C" float expf(float x) noexcept { return (float)expl((long double)x); }

#define private public
#define protected public
#include "ITMLib/ITMLibDefines.h"
#include "ITMLib/Core/ITMBasicEngine.h"
#include "ITMLib/Engines/ViewBuilding/CPU/ITMViewBuilder_CPU.h"
#include "ITMLib/Objects/Camera/ITMCalibIO.h"
#include "ITMLib/Objects/RenderStates/ITMRenderState_VH.h"
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

static ITMDisparityCalib::TrafoType trafo(int type) { return type == 0 ? ITMDisparityCalib::TRAFO_KINECT : ITMDisparityCalib::TRAFO_AFFINE; }

static int run_conv(FILE* in) {
    int32_t hd[4];
    float par[3];
    if (fread(hd, 4, 4, in) != 4 || fread(par, 4, 3, in) != 3) return 3;
    const int W = hd[0], H = hd[1], P = W * H;
    ITMRGBDCalib calib;
    calib.intrinsics_rgb.SetFrom(W, H, par[2], par[2], W * 0.5f, H * 0.5f);
    calib.intrinsics_d = calib.intrinsics_rgb;
    calib.disparityCalib.SetFrom(par[0], par[1], trafo(hd[2]));
    Vector2i dims(W, H);
    ITMUChar4Image rgb(dims, true, false);
    ITMShortImage depth(dims, true, false);
    rgb.Clear();
    if (fread(depth.GetData(MEMORYDEVICE_CPU), 2, P, in) != (size_t)P) return 3;
    ITMViewBuilder_CPU builder(calib);
    ITMView* view = NULL;
    builder.UpdateView(&view, &rgb, &depth, hd[3] != 0);
    chunk("depth_f", 0, view->depth->GetData(MEMORYDEVICE_CPU), (int64_t)P * 4);
    return 0;
}

struct Header {
    int32_t magic, Wd, Hd, Wc, Hc, nframes, type, filter, track;
    float intr_d[4], intr_c[4], ext[16], a, b, voxel, mu, vfmin, vfmax;
};

typedef ITMBasicEngine<ITMVoxel, ITMVoxelIndex> Engine;

static bool same_intrinsics(const ITMIntrinsics& x, const ITMIntrinsics& y) {
    return x.imgSize.x == y.imgSize.x && x.imgSize.y == y.imgSize.y &&
           memcmp(&x.projectionParamsSimple.all, &y.projectionParamsSimple.all, 16) == 0;
}

static int run_engine(FILE* in) {
    Header h;
    if (fread(&h, sizeof(h), 1, in) != 1 || h.magic != 0x47505343) return 2;
    const int Pd = h.Wd * h.Hd, Pc = h.Wc * h.Hc;

    ITMRGBDCalib calib;
    calib.intrinsics_rgb.SetFrom(h.Wc, h.Hc, h.intr_c[0], h.intr_c[1], h.intr_c[2], h.intr_c[3]);
    calib.intrinsics_d.SetFrom(h.Wd, h.Hd, h.intr_d[0], h.intr_d[1], h.intr_d[2], h.intr_d[3]);
    ORUtils::Matrix4<float> ext;
    memcpy(ext.m, h.ext, 64);
    calib.trafo_rgb_to_depth.SetFrom(ext);
    calib.disparityCalib.SetFrom(h.a, h.b, trafo(h.type));
    {
        std::stringstream text;
        writeRGBDCalib(text, calib);
        const std::string s = text.str();
        chunk("calib_txt", 0, s.data(), (int64_t)s.size());
        ITMRGBDCalib back;
        std::stringstream src(s);
        int32_t ok = readRGBDCalib(src, back) ? 1 : 0;
        ok = ok && same_intrinsics(back.intrinsics_rgb, calib.intrinsics_rgb) && same_intrinsics(back.intrinsics_d, calib.intrinsics_d) &&
             memcmp(back.trafo_rgb_to_depth.calib.m, calib.trafo_rgb_to_depth.calib.m, 64) == 0 &&
             memcmp(back.trafo_rgb_to_depth.calib_inv.m, calib.trafo_rgb_to_depth.calib_inv.m, 64) == 0 &&
             back.disparityCalib.GetType() == calib.disparityCalib.GetType() &&
             back.disparityCalib.GetParams().x == calib.disparityCalib.GetParams().x &&
             back.disparityCalib.GetParams().y == calib.disparityCalib.GetParams().y;
        chunk("reread", 0, &ok, 4);
        chunk("calib", 0, calib.trafo_rgb_to_depth.calib.m, 64);
        chunk("calib_inv", 0, calib.trafo_rgb_to_depth.calib_inv.m, 64);
    }

    ITMLibSettings* settings = new ITMLibSettings();
    settings->deviceType = ITMLibSettings::DEVICE_CPU;
    settings->createMeshingEngine = false;
    settings->useBilateralFilter = h.filter != 0;
    settings->sceneParams.voxelSize = h.voxel;
    settings->sceneParams.mu = h.mu;
    settings->sceneParams.viewFrustum_min = h.vfmin;
    settings->sceneParams.viewFrustum_max = h.vfmax;
    Vector2i dims_d(h.Wd, h.Hd), dims_c(h.Wc, h.Hc);
    Engine* eng = new Engine(settings, calib, dims_c, dims_d);
    if (!h.track) eng->turnOffTracking();

    std::vector<ITMUChar4Image*> rgbs(h.nframes);
    std::vector<ITMShortImage*> depths(h.nframes);
    std::vector<ORUtils::Matrix4<float>*> poses(h.nframes);
    for (int f = 0; f < h.nframes; f++) {
        rgbs[f] = new ITMUChar4Image(dims_c, true, false);
        depths[f] = new ITMShortImage(dims_d, true, false);
        float c2w[16];
        if (fread(rgbs[f]->GetData(MEMORYDEVICE_CPU), 4, Pc, in) != (size_t)Pc) return 3;
        if (fread(depths[f]->GetData(MEMORYDEVICE_CPU), 2, Pd, in) != (size_t)Pd) return 3;
        if (fread(c2w, 4, 16, in) != 16) return 3;
        ORUtils::Matrix4<float>* m = new ORUtils::Matrix4<float>();
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) m->m[c * 4 + r] = c2w[r * 4 + c];
        poses[f] = m;
    }
    eng->gtC2wPoses = poses;
    ITMUChar4Image* out = new ITMUChar4Image(dims_c, true, false);

    for (int f = 0; f < h.nframes; f++) {
        eng->ProcessFrame(rgbs[f], depths[f]);
        ITMTrackingState* ts = eng->GetTrackingState();
        ORUtils::Matrix4<float> M = ts->pose_d->GetM(), invM = ts->pose_d->GetInvM();
        ORUtils::Matrix4<float> M_rgb = eng->GetView()->calib.trafo_rgb_to_depth.calib_inv * M;
        chunk("M", f, M.m, 64);
        chunk("invM", f, invM.m, 64);
        chunk("M_rgb", f, M_rgb.m, 64);
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
            std::vector<unsigned char> last;
            uint32_t crc = 0;
            for (int i = 0; i < ITMVoxelBlockHash::noTotalEntries; i++) {
                const ITMHashEntry& e = ht[i];
                if (e.ptr == -2 && e.offset == 0 && e.pos.x == 0 && e.pos.y == 0 && e.pos.z == 0) continue;
                rows.push_back(i); rows.push_back(e.pos.x); rows.push_back(e.pos.y); rows.push_back(e.pos.z);
                rows.push_back(e.offset); rows.push_back(e.ptr);
                if (e.ptr >= 0) {
                    const unsigned char* b = (const unsigned char*)(vba + (size_t)e.ptr * SDF_BLOCK_SIZE3);
                    for (int v = 0; v < SDF_BLOCK_SIZE3; v++) crc = crc32_update(crc, b + v * sizeof(ITMVoxel), 7);  // skip the pad byte
                    if (f == h.nframes - 1) last.insert(last.end(), b, b + SDF_BLOCK_SIZE3 * sizeof(ITMVoxel));
                }
            }
            chunk("hash", f, rows.data(), (int64_t)rows.size() * 4);
            chunk("vba_crc", f, &crc, 4);
            if (f == h.nframes - 1) chunk("vba_last", f, last.data(), (int64_t)last.size());
        }
        chunk("depth_f", f, eng->GetView()->depth->GetData(MEMORYDEVICE_CPU), (int64_t)Pd * 4);
        chunk("minmax", f, rs->renderingRangeImage->GetData(MEMORYDEVICE_CPU), (int64_t)Pd * 8);
        chunk("raycast", f, rs->raycastResult->GetData(MEMORYDEVICE_CPU), (int64_t)Pd * 16);
        chunk("icp_points", f, ts->pointCloud->locations->GetData(MEMORYDEVICE_CPU), (int64_t)Pd * 16);
        chunk("icp_normals", f, ts->pointCloud->colours->GetData(MEMORYDEVICE_CPU), (int64_t)Pd * 16);
        eng->GetImage(out, ITMMainEngine::InfiniTAM_IMAGE_ORIGINAL_RGB);
        int32_t dims[2] = {out->noDims.x, out->noDims.y};
        chunk("img0_dims", f, dims, 8);
        chunk("img0", f, out->GetData(MEMORYDEVICE_CPU), (int64_t)out->noDims.x * out->noDims.y * 4);
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
    if (what == "conv") r = run_conv(in);
    else if (what == "engine") r = run_engine(in);
    else return 2;
    if (r != 0) return r;
    fclose(in);
    fclose(g_out);
    return 0;
}
