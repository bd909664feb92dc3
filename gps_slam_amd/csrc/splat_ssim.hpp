// The 11-tap separable Gaussian window (sigma 1.5) of the fused SSIM map and the arithmetic around it, shared by the operator-level
// kernels (splat_ssim.hip: gps_ssim_fwd / gps_ssim_bwd) and the train step's loss-terms stage (splat_loss.hip), so that both
// compute the same values: tap order and the use of fused multiply-adds follow the reference (`val += G_k * p` contracted by
// nvcc, ssim.cu:209-383).  A workgroup of 256 threads works on a 32 x 32 output tile with a 5-pixel halo held in LDS.
#pragma once
#include "common.hpp"

namespace gps {
namespace ssim {

constexpr int TS = 32;          // output tile edge
constexpr int HALO = 5;
constexpr int TIN = TS + 2 * HALO;  // 42
constexpr int LD_IN = TIN + 1;      // padded row stride of the input tiles
constexpr int LD_H = TS + 1;        // padded row stride of the x-pass results

static __device__ __constant__ float G[11] = {0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f,
                                              0.10936068743467331f,  0.21300552785396576f,   0.26601171493530273f,
                                              0.21300552785396576f,  0.10936068743467331f,   0.036000773310661316f,
                                              0.0075987582094967365f, 0.001028380123898387f};

// forward x-pass: ALL moments (x1, x1^2, x2, x2^2, x1 x2) of row ly of the halo tiles at output column lx, from the same 22 LDS reads
__device__ __forceinline__ void xpass5(const float (*a)[LD_IN], const float (*bb)[LD_IN], float (*h)[TIN][LD_H], int ly, int lx) {
    float s1 = 0.f, s11 = 0.f, s2 = 0.f, s22 = 0.f, s12 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        const float p = a[ly][lx + k], r = bb[ly][lx + k];
        s1 = fmaf(G[k], p, s1);
        s11 = fmaf(G[k], p * p, s11);
        s2 = fmaf(G[k], r, s2);
        s22 = fmaf(G[k], r * r, s22);
        s12 = fmaf(G[k], p * r, s12);
    }
    h[0][ly][lx] = s1; h[1][ly][lx] = s11; h[2][ly][lx] = s2; h[3][ly][lx] = s22; h[4][ly][lx] = s12;
}

// forward y-pass of output pixel (ly, lx)
__device__ __forceinline__ void ypass5(const float (*h)[TIN][LD_H], int ly, int lx, float& mu1, float& e11, float& mu2, float& e22,
                                       float& e12) {
    mu1 = 0.f; e11 = 0.f; mu2 = 0.f; e22 = 0.f; e12 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        mu1 = fmaf(G[k], h[0][ly + k][lx], mu1);
        e11 = fmaf(G[k], h[1][ly + k][lx], e11);
        mu2 = fmaf(G[k], h[2][ly + k][lx], mu2);
        e22 = fmaf(G[k], h[3][ly + k][lx], e22);
        e12 = fmaf(G[k], h[4][ly + k][lx], e12);
    }
}

// the SSIM expression of one pixel from its windowed moments, and (train) the three partial derivatives the backward needs
struct Point { float A, B, C, D, mu1, mu2; };
__device__ __forceinline__ Point point(float mu1, float e11, float mu2, float e22, float e12, float C1, float C2) {
    const float sigma1_sq = e11 - mu1 * mu1, sigma2_sq = e22 - mu2 * mu2, sigma12 = e12 - mu1 * mu2;
    const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
    Point p;
    p.C = 2.0f * mu1_mu2 + C1; p.D = 2.0f * sigma12 + C2;
    p.A = mu1_sq + mu2_sq + C1; p.B = sigma1_sq + sigma2_sq + C2;
    p.mu1 = mu1; p.mu2 = mu2;
    return p;
}
__device__ __forceinline__ float value(const Point& p) { return (p.C * p.D) / (p.A * p.B); }
// value(point(...)) AS gps_ssim_fwd's KERNEL COMPUTES IT, written out.  point() leaves its a * b + c to the compiler's
// floating-point contraction, and hipcc fuses a different part of it in every kernel it is inlined into; in ssim_fwd_kernel
// (splat_ssim.hip, default flags) the two variances become fma(-mu, mu, e) and the covariance does not.  A kernel that must
// return the operator's values bit for bit (image_metrics.hip) cannot call point() and hope for the same choice: it calls this,
// where the choice is explicit and contraction is off.  tests/test_image_eval_gpu.py holds the two together.
// The sequence is not symmetric in the two images (sigma12 rounds mu1 mu2 first, the variances do not): on IDENTICAL windows it
// returns 1 +- ~1e-6, not 1.
__device__ __forceinline__ float value_as_operator(float mu1, float e11, float mu2, float e22, float e12, float C1, float C2) {
#pragma clang fp contract(off)
    const float sigma1_sq = fmaf(-mu1, mu1, e11), sigma2_sq = fmaf(-mu2, mu2, e22);
    const float mu1_mu2 = mu1 * mu2, sigma12 = e12 - mu1_mu2;
    const float C = fmaf(mu1_mu2, 2.0f, C1), D = fmaf(sigma12, 2.0f, C2);
    const float A = (mu1 * mu1 + mu2 * mu2) + C1, B = (sigma1_sq + sigma2_sq) + C2;
    return (C * D) / (A * B);
}
__device__ __forceinline__ float d_mu1(const Point& p) {
    return (p.mu2 * 2.0f * p.D) / (p.A * p.B) - (p.mu2 * 2.0f * p.C) / (p.A * p.B) - (p.mu1 * 2.0f * p.C * p.D) / (p.A * p.A * p.B) +
           (p.mu1 * 2.0f * p.C * p.D) / (p.A * p.B * p.B);
}
__device__ __forceinline__ float d_sigma1_sq(const Point& p) { return (-p.C * p.D) / (p.A * p.B * p.B); }
__device__ __forceinline__ float d_sigma12(const Point& p) { return (2 * p.C) / (p.A * p.B); }

// backward x-pass over t = dL * {dm_dmu1, dm_dsigma1_sq, dm_dsigma12} (with halo)
__device__ __forceinline__ void xpass3(const float (*t)[TIN][LD_IN], float (*h)[TIN][LD_H], int ly, int lx) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        s0 = fmaf(G[k], t[0][ly][lx + k], s0);
        s1 = fmaf(G[k], t[1][ly][lx + k], s1);
        s2 = fmaf(G[k], t[2][ly][lx + k], s2);
    }
    h[0][ly][lx] = s0; h[1][ly][lx] = s1; h[2][ly][lx] = s2;
}

// backward y-pass of output pixel (ly, lx) and d L / d img1 there (p1 = img1, p2 = img2 at the pixel)
__device__ __forceinline__ float ypass3(const float (*h)[TIN][LD_H], int ly, int lx, float p1, float p2) {
    float v0 = 0.f, v1 = 0.f, v2 = 0.f;
#pragma unroll
    for (int k = 0; k < 11; k++) {
        v0 = fmaf(G[k], h[0][ly + k][lx], v0);
        v1 = fmaf(G[k], h[1][ly + k][lx], v1);
        v2 = fmaf(G[k], h[2][ly + k][lx], v2);
    }
    float d = 0.0f;
    d += v0;
    d += p1 * 2.0f * v1;
    d += p2 * v2;
    return d;
}

}  // namespace ssim
}  // namespace gps
