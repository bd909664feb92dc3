// Image-quality evaluation of K rendered views against their ground truth in one launch (gps_image_metrics): per view the mean
// squared error and the mean SSIM, the two numbers the reference's scripts/metric.py and scripts/metric_general.py report as PSNR
// and SSIM (scripts/utils/image_utils.py:19-21, scripts/utils/loss_utils.py:56-86).  No map goes to HBM.
//
// Images are [K,H,W,3] interleaved, uint8 (what the reference measures: the files it wrote, read back through to_tensor) or
// float32 (the unquantised render).  uint8 converts as float(v) / 255.0f, a correctly rounded division like to_tensor's
// .div(255) -- never a multiplication by a reciprocal, which differs in the last bit for some levels.
//
// Depth mask (metric_general.py:62-64): both images are MULTIPLIED by depth > 0 (NaN masks).  Masked pixels become 0 in both
// images, still count in every mean and still feed their neighbours' windows.  They are NOT excluded: excluding them is another
// number (29.05 dB instead of the reference's 29.56 dB on case d_masked of tests/golden/image_metrics_ref.npz).
//
// A workgroup takes one 32 x 32 tile of one view.  SSIM: per channel the halo tiles go to LDS converted and masked, then the two
// passes of splat_ssim.hpp and its value_as_operator with the reference's C1 = 0.01^2, C2 = 0.03^2: per pixel the values of
// gps_ssim_fwd's map on the same float inputs, bit for bit (value_as_operator spells out the contraction hipcc gives that kernel;
// point() here would be fused differently).  One exception: where the windowed moments of the two images coincide -- identical
// images, or both masked to zero -- the expression is 1 by identity (C == A, D == B) and 1 is what is summed, as the reference's
// Python returns; the operator's rounding sequence is not symmetric in the two images and gives 1 +- ~1e-6 there.
// Squared error: of the tile's own pixels; for uint8 the integer differences summed exactly in 64 bits, for float32 the square of
// the fp32 difference summed in double, like the SSIM values.
// Reduction without floating-point atomics: lanes -> wave (shuffles; the helpers of wave_reduce.hpp are fp32, these sums are
// 64-bit) -> workgroup (LDS, wave order) -> one partial per tile in the workspace; a second kernel adds a view's partials in
// tile-index order.  Results are bitwise the same from run to run and do not depend on K or on scheduling.
#include "common.hpp"
#include "splat_ssim.hpp"

namespace {

using namespace gps::ssim;

struct Partial { double ssim, sse; long long sse_u8; };   // one per (view, tile)

static inline int64_t metrics_ws_bytes(int K, int H, int W) {
    return (int64_t)K * gps_div_up(W, TS) * gps_div_up(H, TS) * (int64_t)sizeof(Partial);
}

__device__ __forceinline__ float to_unit(uint8_t v) { return (float)v / 255.0f; }
__device__ __forceinline__ float to_unit(float v) { return v; }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// 1 where the pixel is kept, 0 where the depth masks it (depth > 0 is false for NaN); the images are multiplied by it
__device__ __forceinline__ float keep(const float* __restrict__ depth, int64_t pixel) {
    return (!depth || depth[pixel] > 0.0f) ? 1.0f : 0.0f;
}

template <class T>
__global__ __launch_bounds__(256) void image_metrics_kernel(int H, int W, float C1, float C2, const T* __restrict__ render,
                                                           const T* __restrict__ gt, const float* __restrict__ depth,
                                                           Partial* __restrict__ partials) {
    __shared__ float a[TIN][LD_IN], bb[TIN][LD_IN];
    __shared__ float h[5][TIN][LD_H];
    __shared__ double red_f[4][2];
    __shared__ long long red_i[4];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
    const int64_t view = (int64_t)blockIdx.z * H * W;   // first pixel of this view
    double ssim_sum = 0.0, sse = 0.0;
    long long sse_u8 = 0;

    // squared error of the tile's own pixels, all three channels
    for (int q = tid; q < TS * TS; q += 256) {
        const int ly = q / TS, lx = q - ly * TS;
        const int x = x0 + lx, y = y0 + ly;
        if (x >= W || y >= H) continue;
        const int64_t p = view + (int64_t)y * W + x;
        const float m = keep(depth, p);
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const T r = render[3 * p + c], g = gt[3 * p + c];
            if constexpr (sizeof(T) == 1) {
                const int d = m != 0.0f ? (int)r - (int)g : 0;
                sse_u8 += d * d;
            } else {
                const float d = r * m - g * m;
                sse += (double)d * (double)d;
            }
        }
    }

    for (int c = 0; c < 3; c++) {
        for (int q = tid; q < TIN * TIN; q += 256) {
            const int ly = q / TIN, lx = q - ly * TIN;
            const int x = x0 + lx - HALO, y = y0 + ly - HALO;
            float va = 0.0f, vb = 0.0f;   // zero padding outside the image
            if (x >= 0 && y >= 0 && x < W && y < H) {
                const int64_t p = view + (int64_t)y * W + x;
                const float m = keep(depth, p);
                va = to_unit(render[3 * p + c]) * m;
                vb = to_unit(gt[3 * p + c]) * m;
            }
            a[ly][lx] = va;
            bb[ly][lx] = vb;
        }
        __syncthreads();
        for (int q = tid; q < TIN * TS; q += 256) {
            const int ly = q / TS, lx = q - ly * TS;
            xpass5(a, bb, h, ly, lx);
        }
        __syncthreads();
        // (the next channel's loads write a / bb, which nobody reads after the barrier above; its x-pass writes h only after the
        // next barrier, when every thread is through this loop)
        for (int q = tid; q < TS * TS; q += 256) {
            const int ly = q / TS, lx = q - ly * TS;
            if (x0 + lx >= W || y0 + ly >= H) continue;
            float mu1, e11, mu2, e22, e12;
            ypass5(h, ly, lx, mu1, e11, mu2, e22, e12);
            const bool same = mu1 == mu2 && e11 == e22 && e11 == e12;   // (then the expression is 1 exactly: see the header)
            ssim_sum += same ? 1.0 : (double)value_as_operator(mu1, e11, mu2, e22, e12, C1, C2);
        }
    }

    ssim_sum = wave_sum_f64(ssim_sum);
    sse = wave_sum_f64(sse);
    sse_u8 = wave_sum_i64(sse_u8);
    const int wave = tid >> 6;
    if ((tid & 63) == 0) { red_f[wave][0] = ssim_sum; red_f[wave][1] = sse; red_i[wave] = sse_u8; }
    __syncthreads();
    if (tid == 0) {
        Partial p;
        p.ssim = ((red_f[0][0] + red_f[1][0]) + red_f[2][0]) + red_f[3][0];
        p.sse = ((red_f[0][1] + red_f[1][1]) + red_f[2][1]) + red_f[3][1];
        p.sse_u8 = red_i[0] + red_i[1] + red_i[2] + red_i[3];
        partials[((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = p;
    }
}

// one workgroup per view: its partials added in tile-index order
__global__ __launch_bounds__(64) void image_metrics_finish_kernel(int H, int W, int tiles, int is_u8, const Partial* __restrict__ partials,
                                                                 double* __restrict__ mse, double* __restrict__ ssim,
                                                                 int64_t* __restrict__ sse_u8) {
    if (threadIdx.x != 0) return;
    const Partial* p = partials + (int64_t)blockIdx.x * tiles;
    double s = 0.0, e = 0.0;
    long long ei = 0;
    for (int t = 0; t < tiles; t++) { s += p[t].ssim; e += p[t].sse; ei += p[t].sse_u8; }
    const double n = 3.0 * (double)H * (double)W;
    mse[blockIdx.x] = is_u8 ? (double)ei / (65025.0 * n) : e / n;
    ssim[blockIdx.x] = s / n;
    sse_u8[blockIdx.x] = is_u8 ? ei : 0;
}

}  // namespace

extern "C" {

int64_t gps_image_metrics_workspace_bytes(int K, int H, int W) {
    return (K <= 0 || H <= 0 || W <= 0) ? (int64_t)GPS_ERR_ARG : metrics_ws_bytes(K, H, W);
}

int gps_image_metrics(int K, int H, int W, int dtype, const void* render, const void* gt, const float* depth, void* workspace,
                      int64_t workspace_bytes, double* mse, double* ssim, int64_t* sse_u8, gps_stream stream) {
    GPS_REQUIRE(K > 0 && H > 0 && W > 0 && K <= 65535 && gps_div_up(H, TS) <= 65535);   // (grid limits of the y and z dimensions)
    GPS_REQUIRE((int64_t)gps_div_up(W, TS) * gps_div_up(H, TS) <= INT32_MAX);
    GPS_REQUIRE(dtype == GPS_IMAGE_U8 || dtype == GPS_IMAGE_F32);
    GPS_REQUIRE(render && gt && mse && ssim && sse_u8);
    GPS_REQUIRE(workspace && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0 && workspace_bytes >= metrics_ws_bytes(K, H, W));
    GPS_ENTER();
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(gps_div_up(W, TS), gps_div_up(H, TS), K);
    const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);   // loss_utils.py:78-79
    Partial* partials = reinterpret_cast<Partial*>(workspace);
    if (dtype == GPS_IMAGE_U8)
        image_metrics_kernel<uint8_t><<<grid, 256, 0, st>>>(H, W, C1, C2, (const uint8_t*)render, (const uint8_t*)gt, depth, partials);
    else
        image_metrics_kernel<float><<<grid, 256, 0, st>>>(H, W, C1, C2, (const float*)render, (const float*)gt, depth, partials);
    image_metrics_finish_kernel<<<K, 64, 0, st>>>(H, W, (int)(grid.x * grid.y), dtype == GPS_IMAGE_U8, partials, mse, ssim, sse_u8);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

}  // extern "C"
