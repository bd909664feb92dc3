// Approximate raycast by forward projection for gfx950 (ITMLibSettings::useApproximateRaycast): on a frame whose camera is still
// close to the pose of the last full cast, the last full cast is projected into the new pose and rays are cast only for the
// pixels the projection left empty.  Compiled with -ffp-contract=off (bit-for-bit with the reference's CPU engine).
//
// Per-element maths: ForwardRender_common (Engines/Visualisation/CPU/ITMVisualisationEngine_CPU.tpp:393-453), forwardProjectPixel
// and castRay (Engines/Visualisation/Shared/ITMVisualisationEngine_Shared.h:223-237, 122-221), ITMTrackingController::Prepare
// (Core/ITMTrackingController.h:67-102), ITMTrackingState::TrackerFarFromPointCloud (Objects/Tracking/ITMTrackingState.h:54-75).
//
// Differences in organisation from the reference's CUDA back-end:
//  * its scatter (forwardProject_device) lets the threads race for a target pixel.  The CPU engine visits the sources in scan
//    order, so the source with the HIGHEST linear index wins; here every source bids its index into a winner image with an
//    integer atomicMax and a second pass gathers the winners' values: the CPU's answer on every run.
//  * the missing-pixel count never travels to the host: the sparse cast strides over the list and reads the count on the device.
#include <math.h>
#include <string.h>
#include <time.h>

#include "tsdf_common.hpp"
#include "tsdf_voxel.hpp"

using namespace gpst;

namespace {

// The caller-allocated block of a forward render (gps_tsdf_forward_block_bytes), P = width * height:
//   [P] float4  forward projection        (offset 0)
//   [P] int32   winner image              (offset 16 P)
//   [P] int32   missing list              (offset 20 P)
//   [16] int32  [0] = length of the list  (offset 24 P)
struct FwdBlock { float4* fwd; int32_t* winner; int32_t* missing; int32_t* count; };

inline FwdBlock carve_block(void* block, int64_t P) {
    char* b = static_cast<char*>(block);
    return FwdBlock{reinterpret_cast<float4*>(b), reinterpret_cast<int32_t*>(b + 16 * P), reinterpret_cast<int32_t*>(b + 20 * P),
                    reinterpret_cast<int32_t*>(b + 24 * P)};
}

__global__ __launch_bounds__(256) void forward_clear_kernel(int P, int32_t* __restrict__ winner, int32_t* __restrict__ count) {
    GPS_FRAME_PRIO();
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < P) winner[i] = -1;
    if (i == 0) count[0] = 0;
}

// forwardProjectPixel (Shared.h:223-237) for source pixel i of the last full cast; the source bids its index at its target.
__global__ __launch_bounds__(256) void forward_scatter_kernel(TsdfState s, Mat4 M, const float4* __restrict__ rays,
                                                             int32_t* __restrict__ winner) {
    GPS_FRAME_PRIO();
    const int W = s.width, H = s.height;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= W * H) return;
    const float4 pixel = rays[i];
    // pixel * voxelSize on all four lanes, then w := 1 (a ray that found nothing, w == 0, is projected like any other)
    const float x = pixel.x * s.voxel_size, y = pixel.y * s.voxel_size, z = pixel.z * s.voxel_size;
    float px, py, pz;
    mul_point(M, x, y, z, 1.0f, px, py, pz);
    const float u = s.fx * px / pz + s.cx;
    const float v = s.fy * py / pz + s.cy;
    if ((u < 0) || (u > W - 1) || (v < 0) || (v > H - 1)) return;
    // A NaN coordinate (0 / 0: a point at the camera centre) passes the four comparisons above, and the float -> int conversion
    // the reference then makes is undefined in C++; on x86 it yields INT_MIN, the sum comes out negative and the pixel is dropped.
    // Decision: a non-finite image coordinate is dropped here explicitly (an infinite one never passes the comparisons).
    if (isnan(u) || isnan(v)) return;
    const int target = (int)(u + 0.5f) + (int)(v + 0.5f) * W;
    atomicMax(&winner[target], i);
}

// forwardProjection[t] = the winner's ray (or zero), and the missing test of ForwardRender_common (.tpp:423-439) on it; the
// missing pixels of a wave are compacted with one ballot and appended with one atomic.  Lanes are consecutive pixels of a row, so
// the list keeps scan order within a wave: neighbouring lanes of the sparse cast march neighbouring rays.
__global__ __launch_bounds__(256) void forward_gather_kernel(TsdfState s, const float4* __restrict__ rays,
                                                            const int32_t* __restrict__ winner, float4* __restrict__ fwd,
                                                            int32_t* __restrict__ missing, int32_t* __restrict__ count) {
    GPS_FRAME_PRIO();
    const int W = s.width, P = s.width * s.height;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    bool miss = false;
    if (i < P) {   // (no early return: every lane takes part in the ballot)
        const int w = winner[i];
        const float4 p = w >= 0 ? rays[w] : make_float4(0.f, 0.f, 0.f, 0.f);
        fwd[i] = p;
        const int y = i / W, x = i - y * W;
        const int loc2 = (int)floorf((float)x / MINMAX_SUB) + (int)floorf((float)y / MINMAX_SUB) * W;
        const float2 mm = reinterpret_cast<const float2*>(s.minmax)[loc2];
        const float depth = s.depth[i];
        miss = (p.w <= 0) && ((p.x == 0 && p.y == 0 && p.z == 0) || (depth >= 0)) && (mm.x < mm.y);
    }
    const unsigned long long mask = __ballot(miss);
    const int lane = threadIdx.x & 63;
    int base = 0;
    if (lane == 0 && mask) base = atomicAdd(count, __popcll(mask));
    base = __shfl(base, 0, 64);
    if (miss) missing[base + __popcll(mask & ((1ull << lane) - 1ull))] = i;   // (at most one entry per pixel: the list holds P)
}

// castRay<..., modifyVisibleEntries = false> (Shared.h:122-221), one missing pixel per lane.  The set-up and the per-step float
// operations are those of raycast_kernel (tsdf_render.hip) -- whose free-space look-ahead takes the same steps with the same
// additions -- so a pixel gets the bits the dense cast writes for it; this loop is the reference's, one lookup per step.
__device__ __forceinline__ float4 cast_ray(const TsdfState& s, const Mat4& invM, int x, int y, float2 mm) {
    const float oneOverVoxelSize = 1.0f / s.voxel_size;
    const float ipx = 1.0f / s.fx, ipy = 1.0f / s.fy, ipz = -s.cx, ipw = -s.cy;
    const float stepScale = s.mu * oneOverVoxelSize;
    float cz = mm.x;
    float cx = cz * (((float)x + ipz) * ipx);
    float cy = cz * (((float)y + ipw) * ipy);
    float l2 = 0; l2 += cx * cx; l2 += cy * cy; l2 += cz * cz;
    float totalLength = sqrtf(l2) * oneOverVoxelSize;
    float qx, qy, qz;
    mul_point(invM, cx, cy, cz, 1.0f, qx, qy, qz);
    const float sx = qx * oneOverVoxelSize, sy = qy * oneOverVoxelSize, sz = qz * oneOverVoxelSize;
    cz = mm.y;
    cx = cz * (((float)x + ipz) * ipx);
    cy = cz * (((float)y + ipw) * ipy);
    l2 = 0; l2 += cx * cx; l2 += cy * cy; l2 += cz * cz;
    const float totalLengthMax = sqrtf(l2) * oneOverVoxelSize;
    mul_point(invM, cx, cy, cz, 1.0f, qx, qy, qz);
    float rx = qx * oneOverVoxelSize - sx, ry = qy * oneOverVoxelSize - sy, rz = qz * oneOverVoxelSize - sz;
    const float dn = 1.0f / sqrtf(rx * rx + ry * ry + rz * rz);
    rx *= dn; ry *= dn; rz *= dn;
    float px = sx, py = sy, pz = sz;
    BlockCache cache = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1};
    float sdfValue = 1.0f, confidence = 0.f, stepLength;
    int vmIndex = 0;
    while (totalLength < totalLengthMax) {
        const uint64_t raw = read_voxel_raw(s, (int)roundf_ref(px), (int)roundf_ref(py), (int)roundf_ref(pz), vmIndex, cache);
        sdfValue = vox_sdf(raw) / 32767.0f;
        if (!vmIndex) {
            stepLength = BLK;
        } else {
            if ((sdfValue <= 0.1f) && (sdfValue >= -0.5f)) {
                float dummy;
                sdfValue = read_sdf_interp<false>(s, px, py, pz, vmIndex, cache, dummy);
            }
            if (sdfValue <= 0.0f) break;
            const float a = sdfValue * stepScale;
            stepLength = (a < 1.0f) ? 1.0f : a;
        }
        px += stepLength * rx; py += stepLength * ry; pz += stepLength * rz;
        totalLength += stepLength;
    }
    if (!(sdfValue <= 0.0f)) return make_float4(px, py, pz, 0.0f);
    stepLength = sdfValue * stepScale;
    px += stepLength * rx; py += stepLength * ry; pz += stepLength * rz;
    sdfValue = read_sdf_interp<true>(s, px, py, pz, vmIndex, cache, confidence);
    stepLength = sdfValue * stepScale;
    px += stepLength * rx; py += stepLength * ry; pz += stepLength * rz;
    return make_float4(px, py, pz, confidence + 1.0f);
}

// One wave per workgroup, striding over the list: the host does not know its length, the grid is sized for the image.
constexpr int CAST_THREADS = 64;
constexpr int CAST_MAX_GROUPS = 2048;
__global__ __launch_bounds__(CAST_THREADS) void forward_cast_kernel(TsdfState s, Mat4 invM, const int32_t* __restrict__ missing,
                                                                   const int32_t* __restrict__ count, float4* __restrict__ fwd) {
    GPS_FRAME_PRIO();
    const int W = s.width, P = s.width * s.height;
    const int n = min(count[0], P);
    const float2* minmax = reinterpret_cast<const float2*>(s.minmax);
    for (int k = blockIdx.x * CAST_THREADS + threadIdx.x; k < n; k += gridDim.x * CAST_THREADS) {
        const int loc = missing[k];
        if (loc < 0 || loc >= P) continue;   // (cannot happen: the gather pass wrote the entry)
        const int y = loc / W, x = loc - y * W;
        const int loc2 = (int)floorf((float)x / MINMAX_SUB) + (int)floorf((float)y / MINMAX_SUB) * W;
        fwd[loc] = cast_ray(s, invM, x, y, minmax[loc2]);
    }
}

}  // namespace

extern "C" {

int64_t gps_tsdf_forward_block_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return GPS_ERR_ARG;
    return 24 * (int64_t)width * height + 64;
}

int gps_tsdf_forward_project(const gps_tsdf_state* sp, void* block, const float* M, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(sp != nullptr && block != nullptr && M != nullptr);
    GPS_REQUIRE(state_valid(*sp));
    GPS_REQUIRE((reinterpret_cast<uintptr_t>(block) & 15) == 0);
    TsdfState s = *sp;
    hipStream_t st = (hipStream_t)stream;
    const int P = s.width * s.height, groups = gps_div_up(P, 256);
    const FwdBlock b = carve_block(block, P);
    const float4* rays = reinterpret_cast<const float4*>(s.raycast);
    forward_clear_kernel<<<groups, 256, 0, st>>>(P, b.winner, b.count);
    forward_scatter_kernel<<<groups, 256, 0, st>>>(s, load_mat(M), rays, b.winner);
    forward_gather_kernel<<<groups, 256, 0, st>>>(s, rays, b.winner, b.fwd, b.missing, b.count);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int gps_tsdf_forward_fill(const gps_tsdf_state* sp, void* block, const float* invM, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(sp != nullptr && block != nullptr && invM != nullptr);
    GPS_REQUIRE(state_valid(*sp));
    GPS_REQUIRE((reinterpret_cast<uintptr_t>(block) & 15) == 0);
    TsdfState s = *sp;
    const int P = s.width * s.height;
    const FwdBlock b = carve_block(block, P);
    const int groups = min(gps_div_up(P, CAST_THREADS), CAST_MAX_GROUPS);
    forward_cast_kernel<<<groups, CAST_THREADS, 0, (hipStream_t)stream>>>(s, load_mat(invM), b.missing, b.count, b.fwd);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int gps_tsdf_forward_render(const gps_tsdf_state* s, void* block, const float* M, const float* invM, gps_stream stream) {
    const int r = gps_tsdf_forward_project(s, block, M, stream);
    return r != GPS_OK ? r : gps_tsdf_forward_fill(s, block, invM, stream);
}

int gps_tsdf_forward_missing(const gps_tsdf_state* sp, const void* block, int32_t* count_out, int32_t* list_out, int capacity,
                             gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(sp != nullptr && block != nullptr && count_out != nullptr && capacity >= 0 && (list_out != nullptr || capacity == 0));
    GPS_REQUIRE(sp->width > 0 && sp->height > 0);
    const int P = sp->width * sp->height;
    const FwdBlock b = carve_block(const_cast<void*>(block), P);
    hipStream_t st = (hipStream_t)stream;
    int32_t n = 0;
    if (hipMemcpyAsync(&n, b.count, 4, hipMemcpyDeviceToHost, st) != hipSuccess) return GPS_ERR_LAUNCH;
    if (hipStreamSynchronize(st) != hipSuccess) return GPS_ERR_LAUNCH;
    if (n < 0 || n > P) return GPS_ERR_LAUNCH;
    *count_out = n;
    const int m = n < capacity ? n : capacity;
    if (m > 0) {
        if (hipMemcpyAsync(list_out, b.missing, (size_t)m * 4, hipMemcpyDeviceToHost, st) != hipSuccess) return GPS_ERR_LAUNCH;
        if (hipStreamSynchronize(st) != hipSuccess) return GPS_ERR_LAUNCH;
    }
    return GPS_OK;
}

int gps_track_far_from_point_cloud(const gps_track_state* ts, float* diff_out) {
    if (!ts) return GPS_ERR_ARG;
    // cameraCenter = -1 * (R^T * T) of pose_pointCloud and of pose_d, in ORUtils' operation order (Matrix.h:285-311)
    float c[2][3];
    const float* Ms[2] = {ts->pose_pc_M, ts->pose_M};
    for (int k = 0; k < 2; k++) {
        const float* M = Ms[k];
        const float t0 = M[12], t1 = M[13], t2 = M[14];
        for (int r = 0; r < 3; r++) c[k][r] = -1.0f * (M[4 * r] * t0 + M[4 * r + 1] * t1 + M[4 * r + 2] * t2);
    }
    const float dx = c[0][0] - c[1][0], dy = c[0][1] - c[1][1], dz = c[0][2] - c[1][2];
    const float diff = dx * dx + dy * dy + dz * dz;
    if (diff_out) *diff_out = diff;
    if (ts->age_point_cloud < 0) return 1;   // no point cloud yet
    if (ts->age_point_cloud > 5) return 1;   // older than 5 frames
    return diff > 0.0005f ? 1 : 0;           // the camera centre has moved
}

int gps_tsdf_prepare(const gps_tsdf_state* s, gps_track_state* ts, void* fwd_block, int use_approximate_raycast, gps_stream stream) {
    GPS_REQUIRE(s && ts);
    int r;
    const bool full = !use_approximate_raycast || fwd_block == nullptr || gps_track_far_from_point_cloud(ts, nullptr) != 0;
    if (full) {
        // CreateExpectedDepths + CreateICPMaps (pass B of the expected depths rides in the dense cast)
        if ((r = gps_tsdf_expected_depths_and_raycast(s, ts->pose_M, ts->pose_invM, 0, 1, stream)) != GPS_OK) return r;
        if ((r = gps_tsdf_icp_maps(s, ts->pose_invM, stream)) != GPS_OK) return r;
        memcpy(ts->pose_pc_M, ts->pose_M, 64);  // pose_pointCloud := pose_d (ITMTrackingController.h:87-93)
        ts->age_point_cloud = (ts->age_point_cloud == -1) ? -2 : 0;
    } else {
        // CreateExpectedDepths + ForwardRender: the ICP maps, the last full cast and pose_pointCloud stay; no block is marked visible
        if ((r = gps_tsdf_expected_depths(s, ts->pose_M, 0, stream)) != GPS_OK) return r;
        if ((r = gps_tsdf_forward_render(s, fwd_block, ts->pose_M, ts->pose_invM, stream)) != GPS_OK) return r;
        ts->age_point_cloud++;
    }
    return GPS_OK;
}

int gps_tsdf_frame_map_fwd(const gps_tsdf_state* s, gps_track_state* ts, int fuse, int reset_visible, void* fwd_block,
                           int use_approximate_raycast, gps_stream stream) {
    GPS_REQUIRE(s && ts);
    int r;
    const double t1 = wall_ms();
    if (fuse) {
        if ((r = gps_tsdf_allocate(s, ts->pose_M, ts->pose_invM, stream)) != GPS_OK) return r;
        if ((r = gps_tsdf_integrate(s, ts->pose_M, stream)) != GPS_OK) return r;
    } else {
        if ((r = gps_tsdf_update_visible_list(s, ts->pose_M, ts->pose_invM, reset_visible, stream)) != GPS_OK) return r;
    }
    if ((r = gps_tsdf_prepare(s, ts, fwd_block, use_approximate_raycast, stream)) != GPS_OK) return r;
    ts->diag[15] = (float)(wall_ms() - t1);   // host milliseconds spent ENQUEUEING the fusion + raycast + ICP-map kernels
    return GPS_OK;
}

int gps_tsdf_frame_map_rgb(const gps_tsdf_state* s, gps_track_state* ts, int fuse, int reset_visible, void* fwd_block,
                           int use_approximate_raycast, const gps_colour_camera* cam, gps_stream stream) {
    if (cam == nullptr) return gps_tsdf_frame_map_fwd(s, ts, fuse, reset_visible, fwd_block, use_approximate_raycast, stream);
    GPS_REQUIRE(s && ts);
    GPS_REQUIRE(gpst::colour_camera_valid(*cam));
    int r;
    const double t1 = wall_ms();
    if (fuse) {
        if ((r = gps_tsdf_allocate(s, ts->pose_M, ts->pose_invM, stream)) != GPS_OK) return r;
        if ((r = gps_tsdf_integrate_rgb(s, ts->pose_M, cam, stream)) != GPS_OK) return r;
    } else {
        if ((r = gps_tsdf_update_visible_list(s, ts->pose_M, ts->pose_invM, reset_visible, stream)) != GPS_OK) return r;
    }
    if ((r = gps_tsdf_prepare(s, ts, fwd_block, use_approximate_raycast, stream)) != GPS_OK) return r;
    ts->diag[15] = (float)(wall_ms() - t1);
    return GPS_OK;
}

int gps_tsdf_process_frame_fwd(const gps_tsdf_state* s, const int16_t* depth_mm, const float* M, const float* invM,
                               gps_track_state* ts, void* fwd_block, int use_approximate_raycast, gps_stream stream) {
    GPS_REQUIRE(s && depth_mm && M && invM && ts);
    int r;
    memcpy(ts->pose_M, M, 64);
    memcpy(ts->pose_invM, invM, 64);
    if ((r = gps_tsdf_convert_depth(s, depth_mm, stream)) != GPS_OK) return r;
    if ((r = gps_tsdf_allocate(s, M, invM, stream)) != GPS_OK) return r;
    if ((r = gps_tsdf_integrate(s, M, stream)) != GPS_OK) return r;
    return gps_tsdf_prepare(s, ts, fwd_block, use_approximate_raycast, stream);
}

int gps_tsdf_render_live(const gps_tsdf_state* s, const gps_track_state* ts, const void* fwd_block, uint8_t* colour_out,
                         gps_stream stream) {
    GPS_REQUIRE(s && ts && colour_out);
    // ITMBasicEngine::runRaycast(NULL, NULL) (Core/ITMBasicEngine.tpp:501-518): the last full cast while it is current,
    // the forward projection afterwards
    if (ts->age_point_cloud <= 0) return gps_tsdf_render_colour_from(s, s->raycast, colour_out, stream);
    GPS_REQUIRE(fwd_block != nullptr);
    return gps_tsdf_render_colour_from(s, static_cast<const float*>(fwd_block), colour_out, stream);
}

}  // extern "C"
