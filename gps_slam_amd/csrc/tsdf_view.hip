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
// With a depth calibration (gps_tsdf_convert_filter_depth_calib) the calibrated conversion is a launch of its own into s->depth
// and the five passes all read float images: six launches, the five above untouched.
//
// Also here, as the other half of view building with a full ITMRGBDCalib: the colour image registered to the depth camera
// (register_colour_kernel, gps_tsdf_register_colour) -- ours, not the reference's.
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

// Colour registered to the depth camera (gps_tsdf_register_colour) -- ours, not the reference's: per depth pixel, unproject with
// the depth intrinsics, transform with calib_inv, project with the colour intrinsics, sample as interpolateBilinear does
// (ITMPixelUtils.h:13-29: taps b, c, d count only where their weight is non-zero) and round to nearest.  No occlusion test.
struct RegisterArgs {
    int W, H;                       // depth image
    float fx, fy, cx, cy;           // depth intrinsics
    gpst::Mat4 T;                   // calib_inv: depth camera -> colour camera
    int Wc, Hc;                     // colour image
    float fxc, fyc, cxc, cyc;
};

__global__ __launch_bounds__(256) void register_colour_kernel(RegisterArgs a, const float* __restrict__ depth, const uchar4* __restrict__ rgb,
                                                              uchar4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.W * a.H) return;
    const int y = i / a.W, x = i - y * a.W;
    uchar4 o = make_uchar4(0, 0, 0, 0);
    const float z = depth[i];
    if (z > 0.0f) {
        const float X = z * (((float)x - a.cx) / a.fx);
        const float Y = z * (((float)y - a.cy) / a.fy);
        float px, py, pz;
        gpst::mul_point(a.T, X, Y, z, 1.0f, px, py, pz);
        if (pz > 0.0f) {
            const float u = a.fxc * px / pz + a.cxc;
            const float v = a.fyc * py / pz + a.cyc;
            // (written so that a NaN coordinate is outside)
            if (u >= 1 && u <= a.Wc - 2 && v >= 1 && v <= a.Hc - 2) {
                const int qx = (int)floorf(u), qy = (int)floorf(v);
                const float dx = u - (float)qx, dy = v - (float)qy;
                const uchar4 ta = rgb[qx + qy * a.Wc];
                uchar4 tb = rgb[(qx + 1) + qy * a.Wc], tc = rgb[qx + (qy + 1) * a.Wc], td = rgb[(qx + 1) + (qy + 1) * a.Wc];
                const uchar4 zero4 = make_uchar4(0, 0, 0, 0);
                if (!(dx != 0)) tb = zero4;
                if (!(dy != 0)) tc = zero4;
                if (!(dx != 0 && dy != 0)) td = zero4;
                int c[3];
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const float fa = k == 0 ? ta.x : k == 1 ? ta.y : ta.z, fb = k == 0 ? tb.x : k == 1 ? tb.y : tb.z;
                    const float fc = k == 0 ? tc.x : k == 1 ? tc.y : tc.z, fd = k == 0 ? td.x : k == 1 ? td.y : td.z;
                    const float m = ((fa * (1.0f - dx) * (1.0f - dy) + fb * dx * (1.0f - dy)) + fc * (1.0f - dx) * dy) + fd * dx * dy;
                    c[k] = max(0, min(255, (int)(m + 0.5f)));
                }
                o = make_uchar4((unsigned char)c[0], (unsigned char)c[1], (unsigned char)c[2], 255);
            }
        }
    }
    out[i] = o;
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

int gps_tsdf_convert_filter_depth_calib(const gps_tsdf_state* s, const int16_t* raw, const gps_depth_calib* calib, void* scratch,
                                        gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(scratch != nullptr && (reinterpret_cast<uintptr_t>(scratch) & 3) == 0);
    // (the state, the raw image and the calibration are checked by the conversion, before its launch)
    const int r = gps_tsdf_convert_depth_calib(s, raw, calib, stream);
    if (r != GPS_OK) return r;
    const int W = s->width, H = s->height;
    hipStream_t st = (hipStream_t)stream;
    float* a = static_cast<float*>(scratch);
    float* b = a + (int64_t)W * H;
    const dim3 grid(gps_div_up(W, TW), gps_div_up(H, TH));
    // the reference's own sequence (ITMViewBuilder_CPU.cpp:56-61): depth -> a -> b -> a -> b -> depth
    const float* src[5] = {s->depth, a, b, a, b};
    float* dst[5] = {a, b, a, b, s->depth};
    for (int p = 0; p < 5; p++)
        gps::launch_kernel(gps::TK_FILTER_DEPTH, 0, filter_depth_kernel<false>, grid, dim3(256), 0, st, W, H, (const int16_t*)nullptr, src[p], dst[p]);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int gps_tsdf_register_colour(const gps_tsdf_state* s, const gps_colour_camera* cam, uint8_t* out_rgba8, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(s != nullptr && cam != nullptr && out_rgba8 != nullptr);
    GPS_REQUIRE(s->width > 0 && s->height > 0 && s->depth != nullptr);
    GPS_REQUIRE(gpst::colour_camera_valid(*cam) && (reinterpret_cast<uintptr_t>(out_rgba8) & 3) == 0);
    RegisterArgs a;
    a.W = s->width; a.H = s->height;
    a.fx = s->fx; a.fy = s->fy; a.cx = s->cx; a.cy = s->cy;
    a.T = gpst::load_mat(cam->depth_to_rgb);
    a.Wc = cam->width; a.Hc = cam->height;
    a.fxc = cam->fx; a.fyc = cam->fy; a.cxc = cam->cx; a.cyc = cam->cy;
    const int P = a.W * a.H;
    register_colour_kernel<<<gps_div_up(P, 256), 256, 0, (hipStream_t)stream>>>(a, s->depth, reinterpret_cast<const uchar4*>(cam->rgb),
                                                                                 reinterpret_cast<uchar4*>(out_rgba8));
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

}  // extern "C"
