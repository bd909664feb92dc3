// View building for gfx950: the bilateral depth filter of ITMLibSettings::useBilateralFilter
// (ITMViewBuilder_CPU::UpdateView, ViewBuilding/CPU/ITMViewBuilder_CPU.cpp:53-62): five passes of filterDepth
// (ViewBuilding/Shared/ITMViewBuilder_Shared.h:38-67), a 5x5 bilateral filter whose range sigma is the sensor's noise at the
// centre's depth, over the converted depth image, in front of everything else a frame does.  Compiled with -ffp-contract=off.
//
// What a pass computes is the reference's, operation for operation, because every later stage ends in comparisons and
// truncating stores:
//  * DepthFiltering clears its output and filters y in [2, H-2), x in [2, W-2) only: the two outer rows and columns of EVERY
//    pass's output are 0.0f (not -1), the next pass reads them as valid neighbours, and the final image keeps them.  An image
//    without an interior (W < 5 or H < 5) ends as all zeros.
//  * rows outer, columns inner; w_sum += w and final_depth += w * tmpz in that order in fp32; a neighbour < 0 is skipped, a
//    centre < 0 writes -1.
//  * sigma_z, the L1 spatial term and the exponent are evaluated left to right as the C expression is, with IEEE / and sqrtf.
//  * the exponential: the reference calls expf.  glibc's expf is not correctly rounded and cannot be reproduced here without
//    its tables; this kernel computes exp in double and rounds once, which is what the fixtures' reference is linked against
//    (DESIGN section 8).  Weights at depth steps are denormal or 0 and are NOT flushed; an exponent below -104 (exp < 2^-150:
//    the correctly rounded float is +0) skips the exponential, which changes neither sum.
//
// How it runs is new: one launch per pass, a 256-thread workgroup per 32x8 tile of outputs that stages the 36x12 inputs in LDS
// with row-contiguous loads; pass 1 reads the int16 millimetre image and converts on the way in (convert_depth_kernel's
// arithmetic), pass 5 writes s->depth, every pass writes its own ring of zeros: five launches, no conversion, memset or copy.
#include "launch_timing.hpp"
#include "tsdf_common.hpp"

namespace {

constexpr int TW = 32, TH = 8, HALO = 2;
constexpr int LW = TW + 2 * HALO, LH = TH + 2 * HALO;

template <bool FROM_MM>
__global__ __launch_bounds__(256) void filter_depth_kernel(int W, int H, const int16_t* __restrict__ in_mm, const float* __restrict__ in,
                                                           float* __restrict__ out, gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    __shared__ float tile[LH][LW];
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    for (int k = threadIdx.x; k < LW * LH; k += 256) {
        const int ly = k / LW, lx = k - ly * LW;
        const int gx = x0 - HALO + lx, gy = y0 - HALO + ly;
        float v = -1.0f;   // outside the image: never read by a pixel that is filtered
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const int64_t g = (int64_t)gy * W + gx;
            if (FROM_MM) { const int16_t d = in_mm[g]; v = d <= 0 ? -1.0f : (float)d * (1.0f / 1000.0f) + 0.0f; }
            else v = in[g];
        }
        tile[ly][lx] = v;
    }
    __syncthreads();
    const int tx = threadIdx.x & (TW - 1), ty = threadIdx.x / TW;
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    float* o = out + ((int64_t)y * W + x);
    if (x < 2 || y < 2 || x >= W - 2 || y >= H - 2) { *o = 0.0f; return; }   // image_out->Clear()
    const float z = tile[ty + HALO][tx + HALO];
    if (z < 0.0f) { *o = -1.0f; return; }
    const float sigma_z = 1.0f / (0.0012f + 0.0019f * (z - 0.4f) * (z - 0.4f) + 0.0001f / sqrtf(z) * 0.25f);
    float final_depth = 0.0f, w_sum = 0.0f;
#pragma unroll
    for (int i = -2; i <= 2; i++) {
#pragma unroll
        for (int j = -2; j <= 2; j++) {
            const float tmpz = tile[ty + HALO + i][tx + HALO + j];
            if (tmpz < 0.0f) continue;
            float dz = tmpz - z;
            dz *= dz;
            const float spatial = (float)((i < 0 ? -i : i) + (j < 0 ? -j : j)) * 1.2232f * 1.2232f;
            const float e = -0.5f * (spatial + dz * sigma_z * sigma_z);
            if (e < -104.0f) continue;   // w == +0: w_sum and final_depth stay as they are
            const float w = (float)exp((double)e);
            w_sum += w;
            final_depth += w * tmpz;
        }
    }
    *o = final_depth / w_sum;
}

}  // namespace

extern "C" {

int64_t gps_tsdf_filter_scratch_bytes(int width, int height) {
    if (width <= 0 || height <= 0) return GPS_ERR_ARG;
    return (int64_t)width * height * 2 * (int64_t)sizeof(float);
}

int gps_tsdf_convert_filter_depth(const gps_tsdf_state* s, const int16_t* depth_mm, void* scratch, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(s != nullptr && depth_mm != nullptr && scratch != nullptr);
    GPS_REQUIRE(s->width > 0 && s->height > 0 && s->depth != nullptr);
    GPS_REQUIRE((reinterpret_cast<uintptr_t>(depth_mm) & 1) == 0 && (reinterpret_cast<uintptr_t>(scratch) & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(s->depth) & 3) == 0);
    const int W = s->width, H = s->height;
    hipStream_t st = (hipStream_t)stream;
    float* a = static_cast<float*>(scratch);
    float* b = a + (int64_t)W * H;
    const dim3 grid(gps_div_up(W, TW), gps_div_up(H, TH));
    // floatImage <- depth <- floatImage <- depth <- floatImage, then depth := floatImage (ITMViewBuilder_CPU.cpp:56-61):
    // mm -> a -> b -> a -> b -> s->depth
    gps::launch_kernel(gps::TK_FILTER_DEPTH, 0, filter_depth_kernel<true>, grid, dim3(256), 0, st, W, H, depth_mm, (const float*)nullptr, a);
    gps::launch_kernel(gps::TK_FILTER_DEPTH, 0, filter_depth_kernel<false>, grid, dim3(256), 0, st, W, H, (const int16_t*)nullptr, (const float*)a, b);
    gps::launch_kernel(gps::TK_FILTER_DEPTH, 0, filter_depth_kernel<false>, grid, dim3(256), 0, st, W, H, (const int16_t*)nullptr, (const float*)b, a);
    gps::launch_kernel(gps::TK_FILTER_DEPTH, 0, filter_depth_kernel<false>, grid, dim3(256), 0, st, W, H, (const int16_t*)nullptr, (const float*)a, b);
    gps::launch_kernel(gps::TK_FILTER_DEPTH, 0, filter_depth_kernel<false>, grid, dim3(256), 0, st, W, H, (const int16_t*)nullptr, (const float*)b, s->depth);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

}  // extern "C"
