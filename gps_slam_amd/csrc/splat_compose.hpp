// The `ges` compose with the TSDF layer (raw_gs_model.cpp:318-326), its L1 sign gradient and its backward, written once:
//   rgb   = (raw + base) / (Ws + 1)                          the base colour's weight is always 1 (:321-323)
//   depth = (raw_d + ref [ref > 0]) / (Ws + [ref > 0])       a depth weight only where the raycast hit (:324-326)
// Every kernel that composes goes through these helpers -- gps_compose_l1 (splat_optim.hip), the forward rasterizer's compose
// epilogue (splat_raster.hip), gps_compose_exposure (splat_exposure.hip) and the loss-terms stage (splat_loss.hip) -- so on the
// same render they give the same bits (tests/test_compose_sites_gpu.py).
#pragma once
#include "common.hpp"
#include "splat_exposure.hpp"

namespace gps {

struct ComposedColor {
    float n0, n1, n2;   // numerators raw + base
    float den;          // Ws + 1
    float c0, c1, c2;   // n / den
};

// rc = render_colors[p], w = weight_sum[p]
__device__ __forceinline__ ComposedColor compose_color(float4 rc, float w, const float* base_color, int p) {
    ComposedColor k;
    k.den = w + 1.0f;
    k.n0 = rc.x + base_color[3 * p]; k.n1 = rc.y + base_color[3 * p + 1]; k.n2 = rc.z + base_color[3 * p + 2];
    k.c0 = k.n0 / k.den; k.c1 = k.n1 / k.den; k.c2 = k.n2 / k.den;
    return k;
}

// channel c of compose_color(..) alone, for a channel known only at run time (one division instead of three)
__device__ __forceinline__ float compose_channel(float4 rc, float w, const float* base_color, int p, int c) {
    const float den = w + 1.0f;
    return ((c == 0 ? rc.x : (c == 1 ? rc.y : rc.z)) + base_color[3 * p + c]) / den;
}

// ref = the raw reference depth of the pixel (0 where the raycast missed); 0 / 0 = NaN where nothing was hit either
__device__ __forceinline__ float compose_depth(float raw_d, float w, float ref) {
    const float bw = ref > 0.f ? 1.f : 0.f;
    return (raw_d + ref * bw) / (w + bw);
}

// d (g_abs |gt - x|) / d x for d = gt - x: -g_abs sgn(d), sgn(0) = 0 as in torch
__device__ __forceinline__ float l1_sign_grad(float d, float g_abs) { return d > 0.f ? -g_abs : (d < 0.f ? g_abs : 0.f); }

// (g0, g1, g2) = d loss / d composed colour -> v_render_colors.xyz and v_render_alphas (= d loss / d Ws)
__device__ __forceinline__ void compose_color_bwd(const ComposedColor& k, float g0, float g1, float g2, float& v0, float& v1,
                                                  float& v2, float& va) {
    v0 = g0 / k.den; v1 = g1 / k.den; v2 = g2 / k.den;
    const float dd = k.den * k.den;
    va = -(g0 * k.n0) / dd - (g1 * k.n1) / dd - (g2 * k.n2) / dd;
}

// gz = d loss / d composed depth -> v_render_colors.w; va -= its share of d loss / d Ws (the caller knows the denominator
// Ws + [ref > 0] to be positive: the pixel's depth is valid)
__device__ __forceinline__ void compose_depth_bwd(float raw_d, float w, float ref, float gz, float& v3, float& va) {
    const float bw = ref > 0.f ? 1.f : 0.f;
    const float dden = w + bw, nd = raw_d + ref * bw;
    v3 = gz / dden;
    va -= (gz * nd) / (dden * dden);
}

// 12 per-thread values (one row of d loss / d E) of a 256-thread workgroup -> workgroup sum k returned in thread k < 12: butterfly
// sums inside each wave, then the four waves in order.  One barrier inside; red must not be in use by another thread before it.
__device__ __forceinline__ float block_sum12(float (&v)[12], float* red /* LDS [4][12] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 12; k++) v[k] = wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) red[wave * 12 + k] = v[k];
    }
    __syncthreads();
    const int k = threadIdx.x < 12 ? threadIdx.x : 0;
    return ((red[k] + red[12 + k]) + red[24 + k]) + red[36 + k];
}

}  // namespace gps
