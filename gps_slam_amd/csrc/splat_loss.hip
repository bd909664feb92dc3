// The train step's loss-terms stage (ssim_weight / depth_weight; raw_gs_model.cpp:369-417 computeLoss composed with the compose
// of gps_compose_l1): between the forward rasterizer (plain render instance) and the backward rasterizer, two launches.
//
//   loss_fwd_kernel  one workgroup per 32 x 32 tile and colour channel: compose rgb (+ depth), |gt - rgb|, the SSIM value of the
//                    tile's pixels and the three partial derivatives its backward needs (workspace maps, planar), the masked depth
//                    |gt_depth - depth| and the number of valid depth pixels -> one row {l1, ssim, depth, n_valid} of the slab
//   loss_bwd_kernel  one workgroup per tile: the slab's fixed-order sum (the masked mean's denominator depends on the render),
//                    the SSIM backward of the three channels, the L1 and depth sign gradients, and their composition into exactly
//                    what the backward rasterizers read: v_render_colors, v_render_alphas, pix2.  Workgroup 0 writes loss_terms.
//
// rgb_loss = (1 - s) mean|gt - rgb| + s (1 - mean SSIM over the crop [5:H-5, 5:W-5] of the three channels), or mean|gt - rgb| for
// s = 0;  total = rgb_loss + d mean_valid |gt_depth - depth|, valid = gt_depth > 0 & depth > 0.  With no valid pixel the depth term
// is 0 with a zero gradient (the reference's value there is the mean of an empty tensor, NaN; its gradient is zero as well).
// No float atomics, no allocation, no host synchronisation: every output is bit-identical run to run.
//
// The exposure instance (EXPO; use_exposure, raw_gs_model.cpp:331-346 between the compose and computeLoss): the terms are taken on
// rgb = E(lin), lin the composed colour and E the camera's row of the exposure table.  loss_fwd_kernel then composes all three
// channels of every halo element (each output channel reads all of them; outside the image the SSIM input stays 0, the
// reference's zero padding of the transformed image); loss_bwd_kernel pulls d loss / d rgb back through E before the compose
// backward and writes its tile's 12 partial sums of d loss / d E as one row of the exposure slab (plain stores, every workgroup,
// fixed order), which gps::exposure_reduce_launch sums.
#include <type_traits>

#include "common.hpp"
#include "splat_compose.hpp"
#include "splat_ssim.hpp"

namespace {

using namespace gps::ssim;

constexpr int LOSS_THREADS = 256;
constexpr int SLAB_ROW = 4;   // {sum |gt - rgb|, sum SSIM over the crop, sum valid |gt_depth - depth|, valid depth pixels}

struct LossArgs {
    int W, H;
    const float4* render_colors;   // [P,4]
    const float* weight_sum;       // [P]
    const float* base_color;       // [P,3]
    const float* ref_depth_raw;    // [P] or NULL (no depth output)
    const float* ref_depth_clamped;   // [P] (pix2 only)
    const float* gt_rgb;           // [P,3]
    const float* gt_depth;         // [P] or NULL (no depth term)
    float ssim_weight, depth_weight, delta_depth;
    float* rgb;                    // [P,3]
    float* depth;                  // [P] or NULL
    float* loss_terms;             // [4]
    float* loss;                   // the step's scalar (receives total) or NULL
    float4* v_render_colors;       // [P,4]
    float* v_render_alphas;        // [P]
    float2* pix2;                  // [P] or NULL
    float* slab;                   // [tiles * 3, SLAB_ROW]
    float* maps;                   // [3 (map), 3 (channel), P]
};

struct LossArgsExposure : LossArgs {
    const float* row;              // [3,4] of this camera
    float* eslab;                  // [tiles, 12]: each tile workgroup's sum of d loss / d E
};
template <bool EXPO>
using Args = std::conditional_t<EXPO, LossArgsExposure, LossArgs>;

// channel c of the composed colour at (y, x), with EXPO of E(composed): what gps_compose_l1 / gps_compose_exposure write there; 0
// outside the image
template <bool EXPO>
__device__ __forceinline__ float composed(const LossArgs& a, [[maybe_unused]] const float (&E)[EXPO ? 12 : 1], int c, int y, int x) {
    if (x >= a.W || y >= a.H || x < 0 || y < 0) return 0.0f;
    const int p = y * a.W + x;
    if constexpr (EXPO) {
        const gps::ComposedColor k = gps::compose_color(a.render_colors[p], a.weight_sum[p], a.base_color, p);
        float e0, e1, e2;
        gps::exposure_apply(E, k.c0, k.c1, k.c2, e0, e1, e2);
        return c == 0 ? e0 : (c == 1 ? e1 : e2);
    } else {
        return gps::compose_channel(a.render_colors[p], a.weight_sum[p], a.base_color, p, c);
    }
}

__device__ __forceinline__ float image_at(const float* __restrict__ img, int c, int y, int x, int H, int W) {
    return (x >= W || y >= H || x < 0 || y < 0) ? 0.0f : img[3 * (y * W + x) + c];
}

// SLAB_ROW per-thread values -> their workgroup sums (wave butterflies, then the four waves in order) in out[] of thread 0
__device__ __forceinline__ void block_sum4(float (&v)[SLAB_ROW], float* red /* LDS [4][SLAB_ROW] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < SLAB_ROW; k++) v[k] = wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < SLAB_ROW; k++) red[wave * SLAB_ROW + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < SLAB_ROW; k++)
        v[k] = ((red[k] + red[SLAB_ROW + k]) + red[2 * SLAB_ROW + k]) + red[3 * SLAB_ROW + k];
}

template <bool SSIM, bool EXPO = false>
__global__ __launch_bounds__(LOSS_THREADS) void loss_fwd_kernel(Args<EXPO> a) {
    __shared__ float ta[SSIM ? TIN : 1][LD_IN], tb[SSIM ? TIN : 1][LD_IN];
    __shared__ float h[SSIM ? 5 : 1][TIN][SSIM ? LD_H : 1];
    __shared__ float red[4 * SLAB_ROW];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS, c = blockIdx.z;
    const int W = a.W, H = a.H;
    [[maybe_unused]] float E[EXPO ? 12 : 1];
    if constexpr (EXPO) gps::exposure_load(a.row, E);
    if constexpr (SSIM) {
        for (int q = tid; q < TIN * TIN; q += LOSS_THREADS) {
            const int ly = q / TIN, lx = q - ly * TIN;
            ta[ly][lx] = composed<EXPO>(a, E, c, y0 + ly - HALO, x0 + lx - HALO);
            tb[ly][lx] = image_at(a.gt_rgb, c, y0 + ly - HALO, x0 + lx - HALO, H, W);
        }
        __syncthreads();
        for (int q = tid; q < TIN * TS; q += LOSS_THREADS) {
            const int ly = q / TS, lx = q - ly * TS;
            xpass5(ta, tb, h, ly, lx);
        }
        __syncthreads();
    }
    float acc[SLAB_ROW] = {0.f, 0.f, 0.f, 0.f};
    const size_t P = (size_t)W * H;
    for (int q = tid; q < TS * TS; q += LOSS_THREADS) {
        const int ly = q / TS, lx = q - ly * TS;
        const int x = x0 + lx, y = y0 + ly;
        float mu1, e11, mu2, e22, e12;
        if constexpr (SSIM) ypass5(h, ly, lx, mu1, e11, mu2, e22, e12);
        if (x >= W || y >= H) continue;
        const int p = y * W + x;
        float col;
        if constexpr (SSIM) col = ta[ly + HALO][lx + HALO];
        else col = composed<EXPO>(a, E, c, y, x);
        a.rgb[3 * p + c] = col;
        acc[0] += fabsf(a.gt_rgb[3 * p + c] - col);
        if constexpr (SSIM) {
            const Point pt = point(mu1, e11, mu2, e22, e12, (float)(0.01 * 0.01), (float)(0.03 * 0.03));   // raw_gs_model.cpp:388-389
            if (x >= HALO && x < W - HALO && y >= HALO && y < H - HALO) acc[1] += value(pt);   // padding == "valid"
            const size_t o = (size_t)c * P + p;
            a.maps[o] = d_mu1(pt);
            a.maps[3 * P + o] = d_sigma1_sq(pt);
            a.maps[6 * P + o] = d_sigma12(pt);
        }
        if (c == 0 && a.depth) {
            const float ref = a.ref_depth_raw[p];
            const float d = gps::compose_depth(a.render_colors[p].w, a.weight_sum[p], ref);
            a.depth[p] = d;
            if (a.gt_depth) {
                const float gd = a.gt_depth[p];
                if (gd > 0.f && d > 0.f) { acc[2] += fabsf(gd - d); acc[3] += 1.f; }
            }
        }
    }
    block_sum4(acc, red);
    if (tid == 0) {
        float* row = a.slab + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 3 + c) * SLAB_ROW;
#pragma unroll
        for (int k = 0; k < SLAB_ROW; k++) row[k] = acc[k];
    }
}

template <bool SSIM, bool EXPO = false>
__global__ __launch_bounds__(LOSS_THREADS) void loss_bwd_kernel(Args<EXPO> a) {
    __shared__ float t[SSIM ? 3 : 1][TIN][SSIM ? LD_IN : 1];
    __shared__ float h[SSIM ? 3 : 1][TIN][SSIM ? LD_H : 1];
    __shared__ double dred[LOSS_THREADS][SLAB_ROW];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
    const int W = a.W, H = a.H;
    const size_t P = (size_t)W * H;
    // the slab's sums, the same in every workgroup: thread t adds rows t, t + 256, ... in that order, then a fixed tree in LDS
    {
        const int rows = (int)(gridDim.x * gridDim.y) * 3;
        double s[SLAB_ROW] = {0.0, 0.0, 0.0, 0.0};
        for (int r = tid; r < rows; r += LOSS_THREADS) {
#pragma unroll
            for (int k = 0; k < SLAB_ROW; k++) s[k] += (double)a.slab[(size_t)r * SLAB_ROW + k];
        }
#pragma unroll
        for (int k = 0; k < SLAB_ROW; k++) dred[tid][k] = s[k];
        __syncthreads();
        for (int half = LOSS_THREADS / 2; half > 0; half >>= 1) {
            if (tid < half) {
#pragma unroll
                for (int k = 0; k < SLAB_ROW; k++) dred[tid][k] += dred[tid + half][k];
            }
            __syncthreads();
        }
    }
    const double l1_sum = dred[0][0], ssim_sum = dred[0][1], d_sum = dred[0][2], n_valid = dred[0][3];
    const float s = a.ssim_weight, dw = a.gt_depth ? a.depth_weight : 0.f;
    const int crop = SSIM ? (W - 2 * HALO) * (H - 2 * HALO) * 3 : 1;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
        const float l1 = (float)(l1_sum / (3.0 * (double)P));
        const float ssim_loss = SSIM ? 1.0f - (float)(ssim_sum / (double)crop) : 0.f;
        const float depth_loss = n_valid > 0.0 ? (float)(d_sum / n_valid) : 0.f;
        const float rgb_loss = SSIM ? (1.0f - s) * l1 + s * ssim_loss : l1;
        const float total = rgb_loss + dw * depth_loss;
        a.loss_terms[0] = total; a.loss_terms[1] = l1; a.loss_terms[2] = ssim_loss; a.loss_terms[3] = depth_loss;
        if (a.loss) a.loss[0] = total;
    }
    // upstream gradients as autograd forms them: mean -> grad / n, abs -> grad * sgn
    const float g_l1 = (SSIM ? 1.0f - s : 1.0f) / (float)(3 * P);
    const float g_map = SSIM ? -s / (float)crop : 0.f;
    const float g_depth = (dw > 0.f && n_valid > 0.0) ? dw / (float)n_valid : 0.f;

    float g[4][3];   // d loss / d rgb of this thread's four pixels
#pragma unroll
    for (int j = 0; j < 4; j++) { g[j][0] = 0.f; g[j][1] = 0.f; g[j][2] = 0.f; }
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if constexpr (SSIM) {
            __syncthreads();   // the previous channel's tiles are consumed
            for (int q = tid; q < TIN * TIN; q += LOSS_THREADS) {
                const int ly = q / TIN, lx = q - ly * TIN;
                const int y = y0 + ly - HALO, x = x0 + lx - HALO;
                const bool in_crop = x >= HALO && x < W - HALO && y >= HALO && y < H - HALO;
                float m0 = 0.f, m1 = 0.f, m2 = 0.f;
                if (in_crop) {   // (d loss / d map is zero outside the crop: those pixels' maps are not read)
                    const size_t o = (size_t)c * P + (size_t)y * W + x;
                    m0 = a.maps[o]; m1 = a.maps[3 * P + o]; m2 = a.maps[6 * P + o];
                }
                const float gm = in_crop ? g_map : 0.f;
                t[0][ly][lx] = m0 * gm; t[1][ly][lx] = m1 * gm; t[2][ly][lx] = m2 * gm;
            }
            __syncthreads();
            for (int q = tid; q < TIN * TS; q += LOSS_THREADS) {
                const int ly = q / TS, lx = q - ly * TS;
                xpass3(t, h, ly, lx);
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int q = tid + j * LOSS_THREADS;
            const int ly = q / TS, lx = q - ly * TS;
            const int x = x0 + lx, y = y0 + ly;
            if (x >= W || y >= H) continue;
            const int p = y * W + x;
            const float col = a.rgb[3 * p + c], gt = a.gt_rgb[3 * p + c];
            const float d = gt - col;
            float gc = gps::l1_sign_grad(d, g_l1);
            if constexpr (SSIM) gc += ypass3(h, ly, lx, col, gt);
            g[j][c] = gc;
        }
    }
    [[maybe_unused]] float E[EXPO ? 12 : 1], ve[EXPO ? 12 : 1];
    if constexpr (EXPO) {
        gps::exposure_load(a.row, E);
#pragma unroll
        for (int k = 0; k < 12; k++) ve[k] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int q = tid + j * LOSS_THREADS;
        const int ly = q / TS, lx = q - ly * TS;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const int p = y * W + x;
        const float4 rc = a.render_colors[p];
        const float w = a.weight_sum[p];
        const gps::ComposedColor k = gps::compose_color(rc, w, a.base_color, p);
        if constexpr (EXPO) {   // g: d loss / d E(lin) -> d loss / d E, then d loss / d lin
            gps::exposure_grad_acc(ve, g[j][0], g[j][1], g[j][2], k.c0, k.c1, k.c2);
            float v0, v1, v2;
            gps::exposure_vjp(E, g[j][0], g[j][1], g[j][2], v0, v1, v2);
            g[j][0] = v0; g[j][1] = v1; g[j][2] = v2;
        }
        float v0, v1, v2, va, v3 = 0.f;
        gps::compose_color_bwd(k, g[j][0], g[j][1], g[j][2], v0, v1, v2, va);
        if (g_depth > 0.f) {
            const float gd = a.gt_depth[p], dep = a.depth[p];
            if (gd > 0.f && dep > 0.f)   // (valid: the denominator W + [ref > 0] is positive here)
                gps::compose_depth_bwd(rc.w, w, a.ref_depth_raw[p], gps::l1_sign_grad(gd - dep, g_depth), v3, va);
        }
        a.v_render_colors[p] = make_float4(v0, v1, v2, v3);
        a.v_render_alphas[p] = va;
        // what the strip backward gathers per pixel: {d loss / d weight sum, the depth cut ref_depth + delta_depth}
        if (a.pix2) a.pix2[p] = make_float2(va, a.ref_depth_clamped[p] + a.delta_depth);
    }
    if constexpr (EXPO) {   // this tile's row of the exposure slab (every launched tile holds a pixel)
        __syncthreads();    // dred is consumed: its memory holds the four waves' sums
        const float tot = gps::block_sum12(ve, reinterpret_cast<float*>(&dred[0][0]));
        if (tid < 12) a.eslab[(size_t)(blockIdx.y * gridDim.x + blockIdx.x) * 12 + tid] = tot;
    }
}

}  // namespace

extern "C" {

int64_t gps_loss_terms_workspace_floats(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    const int64_t tiles = (int64_t)gps_div_up(width, TS) * gps_div_up(height, TS);
    return tiles * 3 * SLAB_ROW + 9 * (int64_t)width * height;
}

// row == NULL: the plain instances; otherwise the exposure instances, which also write eslab[tiles, 12]
static int loss_terms_launch(int width, int height, const float* render_colors, const float* weight_sum, const float* base_color,
                             const float* ref_depth_raw, const float* ref_depth_clamped, float delta_depth, const float* gt_rgb,
                             const float* gt_depth, float ssim_weight, float depth_weight, float* rgb, float* depth,
                             float* loss_terms, float* loss, float* v_render_colors, float* v_render_alphas, float* pix2,
                             float* workspace, const float* row, float* eslab, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(width > 0 && height > 0 && (int64_t)width * height <= (int64_t)1 << 26);
    GPS_REQUIRE(render_colors && weight_sum && base_color && gt_rgb && rgb && loss_terms && v_render_colors && v_render_alphas &&
                workspace);
    GPS_REQUIRE(ssim_weight >= 0.f && depth_weight >= 0.f);   // (also refuses NaN)
    GPS_REQUIRE(!(ssim_weight > 0.f) || (width >= 2 * HALO + 1 && height >= 2 * HALO + 1));
    GPS_REQUIRE(depth == nullptr || ref_depth_raw != nullptr);
    GPS_REQUIRE(!(depth_weight > 0.f && gt_depth) || depth != nullptr);
    GPS_REQUIRE(pix2 == nullptr || ref_depth_clamped != nullptr);
    const dim3 tiles(gps_div_up(width, TS), gps_div_up(height, TS));
    float* slab = workspace;
    LossArgs a = {width, height, (const float4*)render_colors, weight_sum, base_color, ref_depth_raw, ref_depth_clamped, gt_rgb,
                  depth_weight > 0.f ? gt_depth : nullptr, ssim_weight, depth_weight, delta_depth, rgb, depth, loss_terms, loss,
                  (float4*)v_render_colors, v_render_alphas, (float2*)pix2, slab, slab + (size_t)tiles.x * tiles.y * 3 * SLAB_ROW};
    hipStream_t s = (hipStream_t)stream;
    if (row) {
        LossArgsExposure ae;
        static_cast<LossArgs&>(ae) = a;
        ae.row = row; ae.eslab = eslab;
        if (ssim_weight > 0.f) {
            loss_fwd_kernel<true, true><<<dim3(tiles.x, tiles.y, 3), LOSS_THREADS, 0, s>>>(ae);
            GPS_LAUNCH_CHECK();
            loss_bwd_kernel<true, true><<<tiles, LOSS_THREADS, 0, s>>>(ae);
        } else {
            loss_fwd_kernel<false, true><<<dim3(tiles.x, tiles.y, 3), LOSS_THREADS, 0, s>>>(ae);
            GPS_LAUNCH_CHECK();
            loss_bwd_kernel<false, true><<<tiles, LOSS_THREADS, 0, s>>>(ae);
        }
    } else if (ssim_weight > 0.f) {
        loss_fwd_kernel<true><<<dim3(tiles.x, tiles.y, 3), LOSS_THREADS, 0, s>>>(a);
        GPS_LAUNCH_CHECK();
        loss_bwd_kernel<true><<<tiles, LOSS_THREADS, 0, s>>>(a);
    } else {
        loss_fwd_kernel<false><<<dim3(tiles.x, tiles.y, 3), LOSS_THREADS, 0, s>>>(a);
        GPS_LAUNCH_CHECK();
        loss_bwd_kernel<false><<<tiles, LOSS_THREADS, 0, s>>>(a);
    }
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int gps_loss_terms(int width, int height, const float* render_colors, const float* weight_sum, const float* base_color,
                   const float* ref_depth_raw, const float* ref_depth_clamped, float delta_depth, const float* gt_rgb,
                   const float* gt_depth, float ssim_weight, float depth_weight, float* rgb, float* depth, float* loss_terms,
                   float* loss, float* v_render_colors, float* v_render_alphas, float* pix2, float* workspace, gps_stream stream) {
    return loss_terms_launch(width, height, render_colors, weight_sum, base_color, ref_depth_raw, ref_depth_clamped, delta_depth,
                             gt_rgb, gt_depth, ssim_weight, depth_weight, rgb, depth, loss_terms, loss, v_render_colors,
                             v_render_alphas, pix2, workspace, nullptr, nullptr, stream);
}

int64_t gps_loss_terms_exposure_partials(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    return (int64_t)gps_div_up(width, TS) * gps_div_up(height, TS);
}

int gps_loss_terms_exposure(int width, int height, const float* render_colors, const float* weight_sum, const float* base_color,
                            const float* ref_depth_raw, const float* ref_depth_clamped, float delta_depth, const float* gt_rgb,
                            const float* gt_depth, float ssim_weight, float depth_weight, float* rgb, float* depth,
                            float* loss_terms, float* loss, float* v_render_colors, float* v_render_alphas, float* pix2,
                            float* workspace, const float* row, float* slab, gps_stream stream) {
    GPS_REQUIRE(row && slab);
    return loss_terms_launch(width, height, render_colors, weight_sum, base_color, ref_depth_raw, ref_depth_clamped, delta_depth,
                             gt_rgb, gt_depth, ssim_weight, depth_weight, rgb, depth, loss_terms, loss, v_render_colors,
                             v_render_alphas, pix2, workspace, row, slab, stream);
}

}  // extern "C"
