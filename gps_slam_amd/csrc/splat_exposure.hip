// Per-frame exposure compensation (use_exposure): the kernels outside the forward rasterizer.
//
// gps_compose_exposure <- raw_gs_model.cpp:318-346 under NoGradGuard: gps_compose_l1's render-only compose with the camera's
//                         exposure row applied to the colour
// gps_exposure_fwd/bwd <- the autograd of `matmul(rgb, E[:, :3].t()) + E[:, 3].t()` (raw_gs_model.cpp:341-345) for the
//                         operator route (forward -> computeLoss -> backward): d rgb, and d E as one row of 12 partial sums per
//                         workgroup
// exposure_reduce      <- the sum of those rows in a fixed order -> the table's gradient (zero outside the camera's row), and in
//                         the train step the table's torch::optim::Adam step (exposureOpt, raw_gs_model.cpp:672) in the same launch
//
// Nothing here uses float atomics: d E is bit-identical run to run.
#include "common.hpp"
#include "launch_timing.hpp"
#include "splat_compose.hpp"

namespace {

constexpr int EXPO_THREADS = 256;
constexpr int EXPO_BWD_BLOCKS = GPS_EXPOSURE_BWD_PARTIALS;

__global__ __launch_bounds__(EXPO_THREADS) void compose_exposure_kernel(int P, const float4* __restrict__ render_colors,
                                                                        const float* __restrict__ weight_sum,
                                                                        const float* __restrict__ base_color,
                                                                        const float* __restrict__ ref_depth_raw,
                                                                        const float* __restrict__ row, float* __restrict__ rgb,
                                                                        float* __restrict__ depth, gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    float E[12];
    gps::exposure_load(row, E);
    const int stride = gridDim.x * blockDim.x;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
        const float4 rc = render_colors[p];
        const float w = weight_sum[p];
        const gps::ComposedColor k = gps::compose_color(rc, w, base_color, p);
        float e0, e1, e2;
        gps::exposure_apply(E, k.c0, k.c1, k.c2, e0, e1, e2);
        rgb[3 * p] = e0; rgb[3 * p + 1] = e1; rgb[3 * p + 2] = e2;
        if (depth) depth[p] = gps::compose_depth(rc.w, w, ref_depth_raw[p]);
    }
}

__global__ __launch_bounds__(EXPO_THREADS) void exposure_fwd_kernel(int P, const float* __restrict__ rgb, const float* __restrict__ row,
                                                                    float* __restrict__ out, gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    float E[12];
    gps::exposure_load(row, E);
    const int stride = gridDim.x * blockDim.x;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
        float e0, e1, e2;
        gps::exposure_apply(E, rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2], e0, e1, e2);
        out[3 * p] = e0; out[3 * p + 1] = e1; out[3 * p + 2] = e2;
    }
}

// grid = EXPO_BWD_BLOCKS workgroups (grid-stride over the pixels): workgroup b writes row b of the slab, zeros if it has no pixel
__global__ __launch_bounds__(EXPO_THREADS) void exposure_bwd_kernel(int P, const float* __restrict__ rgb, const float* __restrict__ row,
                                                                    const float* __restrict__ v_out, float* __restrict__ v_rgb,
                                                                    float* __restrict__ slab, gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    __shared__ float red[48];
    float E[12], ve[12];
    gps::exposure_load(row, E);
#pragma unroll
    for (int k = 0; k < 12; k++) ve[k] = 0.f;
    const int stride = gridDim.x * blockDim.x;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < P; p += stride) {
        const float g0 = v_out[3 * p], g1 = v_out[3 * p + 1], g2 = v_out[3 * p + 2];
        float v0, v1, v2;
        gps::exposure_vjp(E, g0, g1, g2, v0, v1, v2);
        v_rgb[3 * p] = v0; v_rgb[3 * p + 1] = v1; v_rgb[3 * p + 2] = v2;
        gps::exposure_grad_acc(ve, g0, g1, g2, rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
    }
    const float tot = gps::block_sum12(ve, red);
    if (threadIdx.x < 12) slab[(size_t)blockIdx.x * 12 + threadIdx.x] = tot;
}

// ONE workgroup: thread t sums slab rows t, t + 256, ... (in that order), then block_sum12; grad := the full-table gradient;
// with table != NULL the Adam step of every element of the table (rows without a gradient still move through their moments,
// as torch::optim::Adam does with a zero gradient)
__global__ __launch_bounds__(EXPO_THREADS) void exposure_reduce_kernel(const float* __restrict__ slab, int n_partials, int rows,
                                                                       int row, float* __restrict__ grad, float* __restrict__ table,
                                                                       float* __restrict__ m, float* __restrict__ v,
                                                                       gps::AdamScalars sc, gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    __shared__ float red[48], tot[12];
    float acc[12];
#pragma unroll
    for (int k = 0; k < 12; k++) acc[k] = 0.f;
    for (int s = threadIdx.x; s < n_partials; s += EXPO_THREADS) {
#pragma unroll
        for (int k = 0; k < 12; k++) acc[k] += slab[(size_t)s * 12 + k];
    }
    const float sum = gps::block_sum12(acc, red);
    if (threadIdx.x < 12) tot[threadIdx.x] = sum;
    __syncthreads();
    const int n = rows * 12;
    for (int e = threadIdx.x; e < n; e += EXPO_THREADS) {
        const int r = e / 12;
        const float g = r == row ? tot[e - 12 * r] : 0.f;
        grad[e] = g;
        if (table) {
            float mm = 0.f, vv = 0.f, p = table[e];
            if (!sc.fresh) { mm = m[e]; vv = v[e]; }
            gps::adam_update(sc, g, mm, vv, p);
            m[e] = mm; v[e] = vv; table[e] = p;
        }
    }
}

}  // namespace

namespace gps {

int exposure_reduce_launch(const float* slab, int n_partials, int rows, int row, float* grad, float* table, float* m, float* v,
                           const AdamScalars* sc, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(slab && grad && n_partials > 0 && rows > 0 && row >= 0 && row < rows);
    GPS_REQUIRE(!table || (m && v && sc));
    const AdamScalars none = {};
    launch_kernel(TK_EXPOSURE, table ? 1 : 0, exposure_reduce_kernel, dim3(1), dim3(EXPO_THREADS), 0, (hipStream_t)stream, slab,
                  n_partials, rows, row, grad, table, m, v, table ? *sc : none);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

}  // namespace gps

extern "C" {

int64_t gps_exposure_slab_floats(int width, int height) {
    if (width <= 0 || height <= 0) return 0;
    const int64_t tiles = (int64_t)gps_div_up(width, 16) * gps_div_up(height, 16);
    return 12 * (tiles > EXPO_BWD_BLOCKS ? tiles : (int64_t)EXPO_BWD_BLOCKS);
}

int gps_compose_exposure(int width, int height, const float* render_colors, const float* weight_sum, const float* base_color,
                         const float* ref_depth_raw, const float* row, float* rgb, float* depth, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(width > 0 && height > 0);
    GPS_REQUIRE(render_colors && weight_sum && base_color && row && rgb);
    GPS_REQUIRE(depth == nullptr || ref_depth_raw != nullptr);
    const int P = width * height;
    gps::launch_kernel(gps::TK_EXPOSURE, 0, compose_exposure_kernel, dim3(min(1024, gps_div_up(P, EXPO_THREADS))), dim3(EXPO_THREADS),
                       0, (hipStream_t)stream, P, (const float4*)render_colors, weight_sum, base_color, ref_depth_raw, row, rgb, depth);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int gps_exposure_fwd(int n_pixels, const float* rgb, const float* row, float* out, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(n_pixels >= 0 && rgb && row && out);
    if (n_pixels == 0) return GPS_OK;
    gps::launch_kernel(gps::TK_EXPOSURE, 0, exposure_fwd_kernel, dim3(min(1024, gps_div_up(n_pixels, EXPO_THREADS))),
                       dim3(EXPO_THREADS), 0, (hipStream_t)stream, n_pixels, rgb, row, out);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int gps_exposure_bwd(int n_pixels, const float* rgb, const float* row, const float* v_out, float* v_rgb, float* slab,
                     gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(n_pixels >= 0 && rgb && row && v_out && v_rgb && slab);
    gps::launch_kernel(gps::TK_EXPOSURE, 0, exposure_bwd_kernel, dim3(EXPO_BWD_BLOCKS), dim3(EXPO_THREADS), 0, (hipStream_t)stream,
                       n_pixels, rgb, row, v_out, v_rgb, slab);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int gps_exposure_reduce(const float* slab, int n_partials, int rows, int row, float* grad, gps_stream stream) {
    return gps::exposure_reduce_launch(slab, n_partials, rows, row, grad, nullptr, nullptr, nullptr, nullptr, stream);
}

}  // extern "C"
