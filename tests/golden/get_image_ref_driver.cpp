// Driver of tests/golden/make_get_image_golden.py (ours; the generator compiles it against the reference's ITMLib CPU sources,
// which it reads in place).  Runs ITMBasicEngine on the CPU with given poses over a synthetic RGB-D sequence (input file as
// oracle/tsdf_ref.py writes it, with free views: {frame, c2w} pairs) and records every image ITMBasicEngine::GetImage answers.
//
//   get_image_ref_driver <in.bin> <out.bin> <useApproximateRaycast: 0 | 1>
//
// Output: chunks {char name[32]; int32 frame; int64 nbytes; bytes}.  After every frame, in this order: "age" (int32
// age_pointCloud), "invM" (pose_d), "depth_f" (view->depth), "rays" (the ray image the live types read: raycastResult while
// age <= 0, forwardProjection afterwards), "img0" .. "img5" (GetImage of ORIGINAL_RGB, ORIGINAL_DEPTH, SCENERAYCAST,
// COLOUR_FROM_VOLUME, COLOUR_FROM_NORMAL, COLOUR_FROM_CONFIDENCE); then for each free view v of the frame, in file order:
// "finvM<v>", "fimg<v>_6" .. "fimg<v>_9" (FREECAMERA_SHADED, _COLOUR_FROM_VOLUME, _COLOUR_FROM_NORMAL, _COLOUR_FROM_CONFIDENCE) and
// "frays<v>" (the free-view render state's raycastResult, the same for the four).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define private public
#define protected public
#include "ITMLib/ITMLibDefines.h"
#include "ITMLib/Core/ITMBasicEngine.h"
#include "ITMLib/Objects/RenderStates/ITMRenderState_VH.h"
#undef private
#undef protected

using namespace ITMLib;

static FILE* g_out;

static void chunk(const std::string& name, int frame, const void* data, int64_t nbytes) {
    char nm[32];
    memset(nm, 0, sizeof(nm));
    strncpy(nm, name.c_str(), 31);
    fwrite(nm, 1, 32, g_out);
    int32_t f = frame;
    fwrite(&f, 4, 1, g_out);
    fwrite(&nbytes, 8, 1, g_out);
    if (nbytes) fwrite(data, 1, (size_t)nbytes, g_out);
}

struct Header {
    int32_t magic, W, H, nframes, nfree, dump_vba_every;
    float fx, fy, cx, cy, voxel, mu, vfmin, vfmax;
};

typedef ITMBasicEngine<ITMVoxel, ITMVoxelIndex> Engine;

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!in || !g_out) return 2;
    const bool approx = std::string(argv[3]) == "1";
    Header h;
    if (fread(&h, sizeof(h), 1, in) != 1 || h.magic != 0x47505331) return 2;
    const int P = h.W * h.H;

    ITMRGBDCalib calib;
    calib.intrinsics_rgb.SetFrom(h.W, h.H, h.fx, h.fy, h.cx, h.cy);
    calib.intrinsics_d = calib.intrinsics_rgb;
    calib.disparityCalib.SetStandard();
    ITMLibSettings* settings = new ITMLibSettings();
    settings->deviceType = ITMLibSettings::DEVICE_CPU;
    settings->createMeshingEngine = false;
    settings->useApproximateRaycast = approx;
    settings->sceneParams.voxelSize = h.voxel;
    settings->sceneParams.mu = h.mu;
    settings->sceneParams.viewFrustum_min = h.vfmin;
    settings->sceneParams.viewFrustum_max = h.vfmax;
    Vector2i dims(h.W, h.H);
    Engine* eng = new Engine(settings, calib, dims, dims);
    eng->turnOffTracking();

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
    std::vector<int> free_frame(h.nfree);
    std::vector<ORUtils::SE3Pose> free_pose(h.nfree);
    for (int k = 0; k < h.nfree; k++) {
        float c2w[16];
        int32_t fr;
        if (fread(&fr, 4, 1, in) != 1 || fread(c2w, 4, 16, in) != 16) return 3;
        ORUtils::Matrix4<float> m;
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) m.m[c * 4 + r] = c2w[r * 4 + c];
        free_frame[k] = fr;
        free_pose[k].SetInvM(m);   // as ITMBasicEngine::ProcessFrame sets a given pose (ITMBasicEngine.tpp:278-279)
        free_pose[k].Coerce();
    }
    fclose(in);
    eng->gtC2wPoses = poses;

    const ITMMainEngine::GetImageType live_types[6] = {
        ITMMainEngine::InfiniTAM_IMAGE_ORIGINAL_RGB, ITMMainEngine::InfiniTAM_IMAGE_ORIGINAL_DEPTH, ITMMainEngine::InfiniTAM_IMAGE_SCENERAYCAST,
        ITMMainEngine::InfiniTAM_IMAGE_COLOUR_FROM_VOLUME, ITMMainEngine::InfiniTAM_IMAGE_COLOUR_FROM_NORMAL,
        ITMMainEngine::InfiniTAM_IMAGE_COLOUR_FROM_CONFIDENCE};
    const ITMMainEngine::GetImageType free_types[4] = {
        ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_SHADED, ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_VOLUME,
        ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_NORMAL, ITMMainEngine::InfiniTAM_IMAGE_FREECAMERA_COLOUR_FROM_CONFIDENCE};
    ITMUChar4Image* out = new ITMUChar4Image(dims, true, false);
    ITMIntrinsics intr = calib.intrinsics_d;

    for (int f = 0; f < h.nframes; f++) {
        eng->ProcessFrame(rgbs[f], depths[f]);
        ITMTrackingState* ts = eng->GetTrackingState();
        const int32_t age = ts->age_pointCloud;
        ORUtils::Matrix4<float> invM = ts->pose_d->GetInvM();
        chunk("age", f, &age, 4);
        chunk("invM", f, invM.m, 64);
        chunk("depth_f", f, eng->GetView()->depth->GetData(MEMORYDEVICE_CPU), (int64_t)P * 4);
        ITMRenderState* rs = eng->renderState_live;
        chunk("rays", f, (age <= 0 ? rs->raycastResult : rs->forwardProjection)->GetData(MEMORYDEVICE_CPU), (int64_t)P * 16);
        for (int k = 0; k < 6; k++) {
            eng->GetImage(out, live_types[k]);
            if (out->noDims.x != h.W || out->noDims.y != h.H) return 5;
            chunk("img" + std::to_string(k), f, out->GetData(MEMORYDEVICE_CPU), (int64_t)P * 4);
        }
        int v = 0;
        for (int q = 0; q < h.nfree; q++) {
            if (free_frame[q] != f) continue;
            ORUtils::Matrix4<float> finvM = free_pose[q].GetInvM();
            chunk("finvM" + std::to_string(v), f, finvM.m, 64);
            for (int k = 0; k < 4; k++) {
                eng->GetImage(out, free_types[k], &free_pose[q], &intr);
                chunk("fimg" + std::to_string(v) + "_" + std::to_string(6 + k), f, out->GetData(MEMORYDEVICE_CPU), (int64_t)P * 4);
            }
            chunk("frays" + std::to_string(v), f, eng->renderState_freeview->raycastResult->GetData(MEMORYDEVICE_CPU), (int64_t)P * 16);
            v++;
        }
    }
    fclose(g_out);
    return 0;
}
