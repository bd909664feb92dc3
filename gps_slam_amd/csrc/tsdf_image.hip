// The views of ITMBasicEngine::GetImage for gfx950: shading from the volume (grey, normal, confidence), shading from the ray image,
// the input depth in false colour; plus the entry points that route a render type.  Compiled with -ffp-contract=off: the images
// are compared byte for byte with the CPU engine's, and a byte is the truncation of a float.
//
// Per-element maths, restated line by line in the reference's operation order:
//   ITMLib/Engines/Visualisation/Shared/ITMVisualisationEngine_Shared.h:239-397, 483-595   computeNormalAndAngle, drawPixel*, processPixel*
//   ITMLib/Objects/Scene/ITMRepresentationAccess.h:486-600                                computeSingleNormalFromSDF
//   ITMLib/Engines/Visualisation/Interface/ITMVisualisationEngine.cpp:8-57                DepthToUchar4
#include <math.h>

#include "launch_timing.hpp"
#include "tsdf_common.hpp"
#include "tsdf_normals.hpp"
#include "tsdf_voxel.hpp"

using namespace gpst;

namespace {

enum Draw { DRAW_GREY = 0, DRAW_NORMAL = 1, DRAW_CONFIDENCE = 2 };

// interpolateCol / baseCol (Shared.h:346-363) == interpolate / base (ITMVisualisationEngine.cpp:7-17)
__device__ __forceinline__ float interpolate_col(float val, float y0, float x0, float y1, float x1) {
    return (val - x0) * (y1 - y0) / (x1 - x0) + y0;
}
__device__ __forceinline__ float base_col(float val) {
    if (val <= -0.75f) return 0.0f;
    else if (val <= -0.25f) return interpolate_col(val, 0.0f, -0.75f, 1.0f, -0.25f);
    else if (val <= 0.25f) return 1.0f;
    else if (val <= 0.75f) return interpolate_col(val, 1.0f, 0.25f, 0.0f, 0.75f);
    else return 0.0f;
}

// Vector4f::toUChar (ORUtils/Vector.h:639-648): ROUND, (int), CLAMP to 0..255
__device__ __forceinline__ unsigned char round_clamp_u8(float x) {
    const int vi = (int)roundf_ref(x);
    const int lo = (255 < vi) ? 255 : vi;
    return (unsigned char)((0 < lo) ? lo : 0);
}

// drawPixelGrey (Shared.h:340-344): the grey value in all four channels
__device__ __forceinline__ uchar4 draw_grey(float angle) {
    const float outRes = (0.8f * angle + 0.2f) * 255.0f;
    const unsigned char g = (unsigned char)outRes;
    return make_uchar4(g, g, g, g);
}
// drawPixelNormal (Shared.h:380-385) writes r, g, b and leaves the destination's alpha; here a found pixel gets alpha 255
__device__ __forceinline__ uchar4 draw_normal(float nx, float ny, float nz) {
    return make_uchar4((unsigned char)((0.3f + (-nx + 1.0f) * 0.35f) * 255.0f), (unsigned char)((0.3f + (-ny + 1.0f) * 0.35f) * 255.0f),
                       (unsigned char)((0.3f + (-nz + 1.0f) * 0.35f) * 255.0f), 255);
}
// drawPixelConfidence (Shared.h:365-378)
__device__ __forceinline__ uchar4 draw_confidence(float angle, float confidence) {
    const float c100 = (100.f < confidence) ? 100.f : confidence;   // CLAMP(confidence, 0, 100.f) = MAX(0, MIN(100.f, confidence))
    const float confidenceNorm = ((0 < c100) ? c100 : 0) / 100.0f;
    const float r = (float)(unsigned char)(base_col(confidenceNorm) * 255.0f);
    const float g = (float)(unsigned char)(base_col(confidenceNorm - 0.5f) * 255.0f);
    const float b = (float)(unsigned char)(base_col(confidenceNorm + 0.5f) * 255.0f);
    const float sc = 0.8f * angle + 0.2f;
    return make_uchar4(round_clamp_u8(sc * r), round_clamp_u8(sc * g), round_clamp_u8(sc * b), round_clamp_u8(sc * 255.0f));
}

// computeSingleNormalFromSDF (ITMRepresentationAccess.h:486-600).  Its 32 readVoxel calls cover the 4 x 4 x 4 voxels around the
// interpolation cell minus the edges of that cube; a lookup has no side effect the value depends on (the four-argument readVoxel
// has no cache), so they are organised by BLOCK: the cube touches at most two blocks per axis, the <= 8 distinct ones are
// resolved once each -- one lookup when the cube lies inside one block -- with their bucket heads fetched as one batch, then
// the 32 sdf values are loaded as one batch.  An unallocated block reads as sdf 32767, TVoxel().
struct Gradient { float x, y, z; };
__device__ __forceinline__ Gradient single_normal_from_sdf(const TsdfState& s, float px, float py, float pz) {
    const float fx_ = floorf(px), fy_ = floorf(py), fz_ = floorf(pz);
    const float cx = px - fx_, cy = py - fy_, cz = pz - fz_;
    const float ncx = 1.0f - cx, ncy = 1.0f - cy, ncz = 1.0f - cz;
    const int ix = (int)fx_, iy = (int)fy_, iz = (int)fz_;
    // the two candidate blocks per axis: the one of offset -1 and the one of offset +2
    const int bx0 = floor_div_blk(ix - 1), by0 = floor_div_blk(iy - 1), bz0 = floor_div_blk(iz - 1);
    const int bx1 = floor_div_blk(ix + 2), by1 = floor_div_blk(iy + 2), bz1 = floor_div_blk(iz + 2);
    const bool sx = bx1 != bx0, sy = by1 != by0, sz = bz1 != bz0;
    int hidx[8], base[8];
    uint4 hraw[8];
    bool need[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        need[k] = (!(k & 1) || sx) && (!(k & 2) || sy) && (!(k & 4) || sz);
        hidx[k] = hash_index((k & 1) ? bx1 : bx0, (k & 2) ? by1 : by0, (k & 4) ? bz1 : bz0, s.n_buckets - 1);
        hraw[k] = make_uint4(0, 0, 0, 0);
        if (need[k]) hraw[k] = load_raw(s.hash, hidx[k]);
    }
#pragma unroll
    for (int k = 0; k < 8; k += 2) pin(hraw[k], hraw[k + 1]);
#pragma unroll
    for (int k = 0; k < 8; k++) {
        base[k] = -1;
        if (need[k]) {
            int vm;
            BlockCache none = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1};
            base[k] = resolve_with_head(s, (k & 1) ? bx1 : bx0, (k & 2) ? by1 : by0, (k & 4) ? bz1 : bz0, decode_entry(hraw[k]), hidx[k],
                                        vm, none);
        }
    }
    // an axis the cube does not straddle: its "+2" blocks are its "-1" blocks
    if (!sx) { base[1] = base[0]; base[3] = base[2]; base[5] = base[4]; base[7] = base[6]; }
    if (!sy) { base[2] = base[0]; base[3] = base[1]; base[6] = base[4]; base[7] = base[5]; }
    if (!sz) { base[4] = base[0]; base[5] = base[1]; base[6] = base[2]; base[7] = base[3]; }
    // index of voxel (ix + o, ...) in the voxel array, or -1; o in -1..2 -> [o + 1]
    bool hx[4], hy[4], hz[4];
    int lx[4], ly[4], lz[4];
#pragma unroll
    for (int o = 0; o < 4; o++) {
        hx[o] = floor_div_blk(ix + o - 1) != bx0; hy[o] = floor_div_blk(iy + o - 1) != by0; hz[o] = floor_div_blk(iz + o - 1) != bz0;
        lx[o] = (ix + o - 1) & 7; ly[o] = ((iy + o - 1) & 7) * BLK; lz[o] = ((iz + o - 1) & 7) * BLK * BLK;
    }
    const int16_t* sdf16 = reinterpret_cast<const int16_t*>(s.vba);   // gps_voxel: the sdf is the first of its 8 bytes
    int vidx[32];
    // the reads in the reference's order: front / back (the cell's corners), then x -1, x +2, y -1, y +2, z -1, z +2
    constexpr signed char off[32][3] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0}, {0, 0, 1}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1},
                                    {-1, 0, 0}, {-1, 1, 0}, {-1, 0, 1}, {-1, 1, 1}, {2, 0, 0}, {2, 1, 0}, {2, 0, 1}, {2, 1, 1},
                                    {0, -1, 0}, {1, -1, 0}, {0, -1, 1}, {1, -1, 1}, {0, 2, 0}, {1, 2, 0}, {0, 2, 1}, {1, 2, 1},
                                    {0, 0, -1}, {1, 0, -1}, {0, 1, -1}, {1, 1, -1}, {0, 0, 2}, {1, 0, 2}, {0, 1, 2}, {1, 1, 2}};
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const int ox = off[i][0] + 1, oy = off[i][1] + 1, oz = off[i][2] + 1;
        const int b4_0 = hz[oz] ? base[4] : base[0], b4_1 = hz[oz] ? base[5] : base[1], b4_2 = hz[oz] ? base[6] : base[2],
                  b4_3 = hz[oz] ? base[7] : base[3];
        const int b2_0 = hy[oy] ? b4_2 : b4_0, b2_1 = hy[oy] ? b4_3 : b4_1;
        const int b = hx[ox] ? b2_1 : b2_0;
        vidx[i] = b >= 0 ? b + lx[ox] + ly[oy] + lz[oz] : -1;
    }
    int16_t t[32];
#pragma unroll
    for (int i = 0; i < 32; i++) t[i] = sdf16[4 * (size_t)(vidx[i] >= 0 ? vidx[i] : 0)];   // unconditional: one batch, no branches
    float v[32];
#pragma unroll
    for (int i = 0; i < 32; i++) v[i] = vidx[i] >= 0 ? (float)t[i] : 32767.0f;
    const float front_x = v[0], front_y = v[1], front_z = v[2], front_w = v[3], back_x = v[4], back_y = v[5], back_z = v[6], back_w = v[7];
    Gradient ret;
    float p1, p2, v1;
    // gradient x
    p1 = front_x * ncy * ncz + front_z * cy * ncz + back_x * ncy * cz + back_z * cy * cz;
    p2 = v[8] * ncy * ncz + v[9] * cy * ncz + v[10] * ncy * cz + v[11] * cy * cz;
    v1 = p1 * cx + p2 * ncx;
    p1 = front_y * ncy * ncz + front_w * cy * ncz + back_y * ncy * cz + back_w * cy * cz;
    p2 = v[12] * ncy * ncz + v[13] * cy * ncz + v[14] * ncy * cz + v[15] * cy * cz;
    ret.x = (p1 * ncx + p2 * cx - v1) / 32767.0f;
    // gradient y
    p1 = front_x * ncx * ncz + front_y * cx * ncz + back_x * ncx * cz + back_y * cx * cz;
    p2 = v[16] * ncx * ncz + v[17] * cx * ncz + v[18] * ncx * cz + v[19] * cx * cz;
    v1 = p1 * cy + p2 * ncy;
    p1 = front_z * ncx * ncz + front_w * cx * ncz + back_z * ncx * cz + back_w * cx * cz;
    p2 = v[20] * ncx * ncz + v[21] * cx * ncz + v[22] * ncx * cz + v[23] * cx * cz;
    ret.y = (p1 * ncy + p2 * cy - v1) / 32767.0f;
    // gradient z
    p1 = front_x * ncx * ncy + front_y * cx * ncy + front_z * ncx * cy + front_w * cx * cy;
    p2 = v[24] * ncx * ncy + v[25] * cx * ncy + v[26] * ncx * cy + v[27] * cx * cy;
    v1 = p1 * cz + p2 * ncz;
    p1 = back_x * ncx * ncy + back_y * cx * ncy + back_z * ncx * cy + back_w * cx * cy;
    p2 = v[28] * ncx * ncy + v[29] * cx * ncy + v[30] * ncx * cy + v[31] * cx * cy;
    ret.z = (p1 * ncz + p2 * cz - v1) / 32767.0f;
    return ret;
}

// processPixelGrey / processPixelNormal / processPixelConfidence (Shared.h:539-595) over a ray image of W x H pixels.  One wave =
// one 8 x 8 pixel patch (2 x 2 waves per workgroup), as the raycaster that wrote the rays: neighbouring rays end in the same blocks.
template <int DRAW>
__global__ __launch_bounds__(256) void shade_volume_kernel(TsdfState s, int W, int H, Mat4 invM, const float4* __restrict__ rays,
                                                           uchar4* __restrict__ out, gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    const int wave_in_wg = threadIdx.x >> 6, lane_ = threadIdx.x & 63;
    const int x = blockIdx.x * 16 + (wave_in_wg & 1) * 8 + (lane_ & 7), y = blockIdx.y * 16 + (wave_in_wg >> 1) * 8 + (lane_ >> 3);
    if (x >= W || y >= H) return;
    const int loc = x + y * W;
    const float4 r = rays[loc];
    uchar4 px = make_uchar4(0, 0, 0, 0);
    if (r.w > 0) {
        // computeNormalAndAngle (Shared.h:239-255)
        const Gradient g = single_normal_from_sdf(s, r.x, r.y, r.z);
        const float normScale = 1.0f / sqrtf(g.x * g.x + g.y * g.y + g.z * g.z);
        const float nx = g.x * normScale, ny = g.y * normScale, nz = g.z * normScale;
        const float angle = nx * (-invM.m[8]) + ny * (-invM.m[9]) + nz * (-invM.m[10]);
        if (angle > 0.0) {
            if (DRAW == DRAW_GREY) px = draw_grey(angle);
            else if (DRAW == DRAW_NORMAL) px = draw_normal(nx, ny, nz);
            else px = draw_confidence(angle, r.w - 1.0f);
        }
    }
    out[loc] = px;
}

// processPixelGrey_ImageNormals<useSmoothing = true, flipNormals = false> (Shared.h:482-499)
__global__ __launch_bounds__(256) void shade_image_normals_kernel(int W, int H, float voxel_size, Mat4 invM, const float4* __restrict__ rays,
                                                                  uchar4* __restrict__ out, gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (x >= W || y >= H) return;
    const int loc = x + y * W;
    bool found = rays[loc].w > 0.0f;
    float nx, ny, nz, angle = 0.f;
    if (found) found = image_normal_and_angle(rays, x, y, W, H, voxel_size, invM, nx, ny, nz, angle);
    out[loc] = found ? draw_grey(angle) : make_uchar4(0, 0, 0, 0);
}

// DepthToUchar4 (ITMVisualisationEngine.cpp:19-57), pass 1: min and max over the depths > 0.  Positive floats order like their bit
// patterns; the minimum is kept as the maximum of the inverted bits, so that both words start from 0 (one memset) and "no valid
// depth" is a max word of 0.  One pair of atomics per wave.
__global__ __launch_bounds__(256) void depth_limits_kernel(const float* __restrict__ depth, int n, uint32_t* __restrict__ lims) {
    uint32_t inv_min = 0u, mx = 0u;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float v = depth[i];
        if (v > 0.0f) { const uint32_t b = __float_as_uint(v); inv_min = max(inv_min, ~b); mx = max(mx, b); }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        inv_min = max(inv_min, (uint32_t)__shfl_xor((int)inv_min, o, 64));
        mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    }
    if ((threadIdx.x & 63) == 0 && mx != 0u) { atomicMax(&lims[0], inv_min); atomicMax(&lims[1], mx); }
}

// ... pass 2: the three ramps.  (The reference's other scale, 1 / max for max - min == 0, is never used: it returns first.)
__global__ __launch_bounds__(256) void depth_colour_kernel(const float* __restrict__ depth, int n, const uint32_t* __restrict__ lims,
                                                           uchar4* __restrict__ out, gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t mx_bits = lims[1];
    const float lo = __uint_as_float(~lims[0]), hi = __uint_as_float(mx_bits);
    uchar4 px = make_uchar4(0, 0, 0, 0);
    float sourceVal = depth[i];
    if (mx_bits != 0u && lo != hi && sourceVal > 0.0f) {
        const float scale = 1.0f / (hi - lo);
        sourceVal = (sourceVal - lo) * scale;
        px = make_uchar4((unsigned char)(base_col(sourceVal - 0.5f) * 255.0f), (unsigned char)(base_col(sourceVal) * 255.0f),
                         (unsigned char)(base_col(sourceVal + 0.5f) * 255.0f), 255);
    }
    out[i] = px;
}

}  // namespace

extern "C" {

int gps_tsdf_render_image(const gps_tsdf_state* sp, const float* rays, int width, int height, const float* invM, int type,
                          uint8_t* out_rgba8, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(sp != nullptr && rays != nullptr && invM != nullptr && out_rgba8 != nullptr);
    GPS_REQUIRE(width > 0 && height > 0 && (int64_t)width * height <= 0x7fffffff / 4);
    GPS_REQUIRE(type >= 0 && type < GPS_RENDER_N_TYPES);
    hipStream_t st = (hipStream_t)stream;
    const float4* pr = reinterpret_cast<const float4*>(rays);
    uchar4* out = reinterpret_cast<uchar4*>(out_rgba8);
    const dim3 grid(gps_div_up(width, 16), gps_div_up(height, 16));
    if (type == GPS_RENDER_SHADED_GREYSCALE_IMAGENORMALS) {
        GPS_REQUIRE(sp->voxel_size > 0.f);
        GPS_REQUIRE(!(sp->fx * sp->fy < 0.f));   // ITMIntrinsics::FocalLengthSignsDiffer: flipNormals = true is not implemented
        gps::launch_kernel(gps::TK_RENDER_IMAGE, 0, shade_image_normals_kernel, grid, dim3(256), 0, st, width, height, sp->voxel_size,
                           load_mat(invM), pr, out);
        GPS_LAUNCH_CHECK();
        return GPS_OK;
    }
    GPS_REQUIRE(state_valid(*sp));
    TsdfState s = *sp;
    s.width = width; s.height = height;
    if (type == GPS_RENDER_COLOUR_FROM_VOLUME) return gps_tsdf_render_colour_from(&s, rays, out_rgba8, stream);
    if (type == GPS_RENDER_SHADED_GREYSCALE)
        gps::launch_kernel(gps::TK_RENDER_IMAGE, 0, shade_volume_kernel<DRAW_GREY>, grid, dim3(256), 0, st, s, width, height, load_mat(invM), pr, out);
    else if (type == GPS_RENDER_COLOUR_FROM_NORMAL)
        gps::launch_kernel(gps::TK_RENDER_IMAGE, 0, shade_volume_kernel<DRAW_NORMAL>, grid, dim3(256), 0, st, s, width, height, load_mat(invM), pr, out);
    else
        gps::launch_kernel(gps::TK_RENDER_IMAGE, 0, shade_volume_kernel<DRAW_CONFIDENCE>, grid, dim3(256), 0, st, s, width, height, load_mat(invM), pr, out);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int64_t gps_tsdf_depth_to_rgba8_scratch_bytes(void) { return 16; }

int gps_tsdf_depth_to_rgba8(const float* depth, int n, void* scratch, uint8_t* out_rgba8, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(depth != nullptr && scratch != nullptr && out_rgba8 != nullptr && n > 0);
    hipStream_t st = (hipStream_t)stream;
    uint32_t* lims = reinterpret_cast<uint32_t*>(scratch);
    if (hipMemsetAsync(lims, 0, 8, st) != hipSuccess) return GPS_ERR_LAUNCH;
    const int groups = min(gps_div_up(n, 256), 1024);
    depth_limits_kernel<<<groups, 256, 0, st>>>(depth, n, lims);
    gps::launch_kernel(gps::TK_RENDER_IMAGE, 1, depth_colour_kernel, dim3(gps_div_up(n, 256)), dim3(256), 0, st, depth, n, (const uint32_t*)lims,
                       reinterpret_cast<uchar4*>(out_rgba8));
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int gps_tsdf_get_image(const gps_tsdf_state* s, const float* M, const float* invM, int type, uint8_t* out_rgba8, gps_stream stream) {
    GPS_REQUIRE(s != nullptr && M != nullptr && invM != nullptr);
    GPS_REQUIRE(type >= 0 && type < GPS_RENDER_N_TYPES && type != GPS_RENDER_SHADED_GREYSCALE_IMAGENORMALS);
    GPS_REQUIRE(state_valid(*s));
    int r;
    if ((r = gps_tsdf_find_visible(s, M, stream)) != GPS_OK) return r;
    if ((r = gps_tsdf_expected_depths_and_raycast(s, M, invM, 1, 0, stream)) != GPS_OK) return r;
    return gps_tsdf_render_image(s, s->fv_raycast, s->width, s->height, invM, type, out_rgba8 ? out_rgba8 : s->fv_colour, stream);
}

}  // extern "C"
