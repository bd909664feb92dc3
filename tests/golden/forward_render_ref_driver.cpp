// Driver of tests/golden/make_forward_render_golden.py (ours; the generator compiles it against the reference's ITMLib CPU
// sources, which it reads in place).  Runs ITMBasicEngine on the CPU with useApproximateRaycast = true over a synthetic RGB-D
// sequence (input file as oracle/tsdf_ref.py writes it) and records, per frame, what ITMTrackingController::Prepare did.
//
//   forward_render_ref_driver <in.bin> <out.bin> [track]
//
// Output: chunks {char name[32]; int32 frame; int64 nbytes; bytes}.  Per frame: M, invM, the engine dump of oracle/ref_driver.cpp
// (counts, visible_ids, vis_type_nz, hash, vba_crc, depth_f, minmax, raycast, icp_points, icp_normals), "prep" = int32 {age before,
// age after, branch (1 = forward render), noFwdProjMissingPoints, targets with more than one source}, "diff" = float32 of the far
// test, "pc_M" = pose_pointCloud before the frame, "live" = runRaycast(NULL, NULL)'s colour image, and on a forward frame "fwd"
// (forwardProjection after the hole fill), "fwd_pre" (the scatter alone, recomputed here with the reference's
// forwardProjectPixel) and "missing" (fwdProjMissingPoints).
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
#include "ITMLib/Engines/Visualisation/Shared/ITMVisualisationEngine_Shared.h"
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

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    g_out = fopen(argv[2], "wb");
    if (!in || !g_out) return 2;
    const bool track = argc >= 4 && std::string(argv[3]) == "track";
    Header h;
    if (fread(&h, sizeof(h), 1, in) != 1 || h.magic != 0x47505331 || h.nfree != 0) return 2;
    const int P = h.W * h.H;

    ITMRGBDCalib calib;
    calib.intrinsics_rgb.SetFrom(h.W, h.H, h.fx, h.fy, h.cx, h.cy);
    calib.intrinsics_d = calib.intrinsics_rgb;
    calib.disparityCalib.SetStandard();
    ITMLibSettings* settings = new ITMLibSettings();
    settings->deviceType = ITMLibSettings::DEVICE_CPU;
    settings->createMeshingEngine = false;
    settings->useApproximateRaycast = true;
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
    fclose(in);
    eng->gtC2wPoses = poses;

    for (int f = 0; f < h.nframes; f++) {
        ITMTrackingState* ts = eng->GetTrackingState();
        const int age_before = ts->age_pointCloud;
        ORUtils::SE3Pose pc_before(*ts->pose_pointCloud);
        eng->ProcessFrame(rgbs[f], depths[f]);
        ts = eng->GetTrackingState();
        ORUtils::Matrix4<float> M = ts->pose_d->GetM(), invM = ts->pose_d->GetInvM(), pcM = pc_before.GetM();
        chunk("M", f, M.m, 64);
        chunk("invM", f, invM.m, 64);
        chunk("pc_M", f, pcM.m, 64);
        // the far test as Prepare saw it (Objects/Tracking/ITMTrackingState.h:63-72): pose_pointCloud of before, pose_d of now
        Vector3f c_pc = -1.0f * (pc_before.GetR().t() * pc_before.GetT());
        Vector3f c_live = -1.0f * (ts->pose_d->GetR().t() * ts->pose_d->GetT());
        Vector3f d3 = c_pc - c_live;
        const float diff = d3.x * d3.x + d3.y * d3.y + d3.z * d3.z;
        chunk("diff", f, &diff, 4);
        const int age_after = ts->age_pointCloud;
        const int branch = age_after > 0 ? 1 : 0;
        const bool far = age_before < 0 || age_before > 5 || diff > 0.0005f;
        if (far == (branch == 1)) { fprintf(stderr, "frame %d: branch %d but far test %d\n", f, branch, (int)far); return 4; }

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
        const Vector4f* rays = rs->raycastResult->GetData(MEMORYDEVICE_CPU);
        chunk("raycast", f, rays, (int64_t)P * 16);
        chunk("icp_points", f, ts->pointCloud->locations->GetData(MEMORYDEVICE_CPU), (int64_t)P * 16);
        chunk("icp_normals", f, ts->pointCloud->colours->GetData(MEMORYDEVICE_CPU), (int64_t)P * 16);

        int32_t prep[5] = {age_before, age_after, branch, 0, 0};
        if (branch) {
            prep[3] = rs->noFwdProjMissingPoints;
            chunk("fwd", f, rs->forwardProjection->GetData(MEMORYDEVICE_CPU), (int64_t)P * 16);
            chunk("missing", f, rs->fwdProjMissingPoints->GetData(MEMORYDEVICE_CPU), (int64_t)prep[3] * 4);
            // the scatter on its own, in the scan order of ForwardRender_common (.tpp:411-420), and how many sources each target got
            std::vector<Vector4f> pre(P, Vector4f(0.0f, 0.0f, 0.0f, 0.0f));
            std::vector<int> hits(P, 0);
            const Vector4f projParams = calib.intrinsics_d.projectionParamsSimple.all;
            for (int i = 0; i < P; i++) {
                const Vector4f pixel = rays[i];
                const int t = forwardProjectPixel(pixel * h.voxel, M, projParams, dims);
                if (t >= 0) { pre[t] = pixel; hits[t]++; }
            }
            for (int i = 0; i < P; i++) prep[4] += hits[i] > 1;
            chunk("fwd_pre", f, pre.data(), (int64_t)P * 16);
        }
        chunk("prep", f, prep, 20);
        eng->runRaycast(nullptr, nullptr);
        chunk("live", f, eng->renderState_live->raycastImage->GetData(MEMORYDEVICE_CPU), (int64_t)P * 4);
    }
    fclose(g_out);
    return 0;
}
