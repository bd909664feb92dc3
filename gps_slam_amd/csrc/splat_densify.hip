// Densification of the classic 3DGS trainer (RawGaussianModel::stepPostBackward / updateDensifyGrad / densifiyGs,
// src/raw_gs_model.cpp:419-633) on the device:
//
// gps_densify_accumulate <- updateDensifyGrad: the screen-space gradient norm and the visibility count of every row with
//                           radii > 0, one launch instead of ~12 tensor ops (max2DSize is not built: nothing reads it).
// gps_densify_plan       <- densifiyGs up to its masks: clone / split / prune classes per row, the ordered ranks of the four
//                           row sets and the destination table of the new model, two launches over 256-row blocks in the
//                           shape of gps_compact_mask (per-block counts, then every block sums the counts in front of it),
//                           with the block scan of common.hpp.  The five counts go to a device and a pinned host word.
// gps_densify_apply      <- the cat of {originals, split children, clones} and the order-preserving prune behind it, for
//                           the parameters and both Adam moments, in one out-of-place pass whose threads run along the
//                           floats of the DESTINATION tensors (coalesced stores; a source row is read by neighbouring lanes).
#include <math.h>

#include "common.hpp"

namespace {

constexpr int DP_THREADS = GPS_DENSIFY_PLAN_BLOCK;
constexpr int NCLS = 4;   // keep, split (all parents), split surviving, clone surviving
static_assert(DP_THREADS / 64 == NCLS, "plan_write_kernel: one wave per class sums the block counts");
enum : uint8_t { F_KEEP = 1, F_SPLIT = 2, F_SPLIT_SURV = 4, F_DUP_SURV = 8 };

// sizeFac of densifiyGs (raw_gs_model.cpp:553), the float the reference divides by
constexpr float SPLIT_SIZE_FAC = 1.6f;

__device__ __forceinline__ float child_log_scale(float s) {
    // log(exp(s) / 1.6) evaluated in double and rounded once (the float sequence can be 5 half-ulps off around |s| = 1)
    return (float)log(exp((double)s) / (double)SPLIT_SIZE_FAC);
}

__global__ __launch_bounds__(256) void accumulate_kernel(int N, const float2* __restrict__ v_means2d, const int32_t* __restrict__ radii,
                                                        float half_w, float half_h, float* __restrict__ grad_sum,
                                                        float* __restrict__ vis_count) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || radii[i] <= 0) return;
    const float2 g = v_means2d[i];
    const float x = g.x * half_w, y = g.y * half_h;
    grad_sum[i] += sqrtf(x * x + y * y);
    vis_count[i] += 1.0f;
}

struct PlanArgs {
    int N;
    const float *grad_sum, *vis_count, *log_scales, *opac_logit;
    float grad_thres, split_scale, prune_opac, prune_scale;
};

// the classes of row i as the reference's masks decide them (float sequence of the tensor ops: expf, 1 / (1 + expf(-x)))
__device__ __forceinline__ uint8_t classify(const PlanArgs& a, int i) {
    const float avg = a.grad_sum[i] / fmaxf(a.vis_count[i], 1.0f);
    const bool high = avg > a.grad_thres;
    const float l0 = a.log_scales[3 * i], l1 = a.log_scales[3 * i + 1], l2 = a.log_scales[3 * i + 2];
    const float smax = fmaxf(fmaxf(expf(l0), expf(l1)), expf(l2));
    const bool large = smax > a.split_scale;
    const bool split = high && large, dup = high && !large;
    const float op = 1.0f / (1.0f + expf(-a.opac_logit[i]));
    const bool low = op < a.prune_opac;
    const bool pruned = low || smax > a.prune_scale;   // of the row's own values: the row and its clone alike
    uint8_t f = 0;
    if (split) {
        f |= F_SPLIT;
        const float cmax = fmaxf(fmaxf(expf(child_log_scale(l0)), expf(child_log_scale(l1))), expf(child_log_scale(l2)));
        if (!low && !(cmax > a.prune_scale)) f |= F_SPLIT_SURV;
    } else if (!pruned) {
        f |= F_KEEP;
        if (dup) f |= F_DUP_SURV;
    }
    return f;
}

__global__ __launch_bounds__(DP_THREADS) void plan_count_kernel(PlanArgs a, uint8_t* __restrict__ flags, int32_t* __restrict__ blk, int nblk) {
    __shared__ int red[NCLS][DP_THREADS / 64];
    const int i = blockIdx.x * DP_THREADS + threadIdx.x;
    const uint8_t f = i < a.N ? classify(a, i) : 0;
    if (i < a.N) flags[i] = f;
#pragma unroll
    for (int c = 0; c < NCLS; c++) {
        const int s = wave_sum_i((f >> c) & 1);
        if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x < NCLS) {
        int s = 0;
        for (int w = 0; w < DP_THREADS / 64; w++) s += red[threadIdx.x][w];
        blk[threadIdx.x * nblk + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(DP_THREADS) void plan_write_kernel(int N, const uint8_t* __restrict__ flags, const int32_t* __restrict__ blk,
                                                               int nblk, int32_t* __restrict__ dst_src, int32_t* __restrict__ dst_sample,
                                                               int32_t* __restrict__ counts, volatile int32_t* host_counts) {
    __shared__ int ws[DP_THREADS / 64 + 1];
    __shared__ int before_s[NCLS], total_s[NCLS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave < NCLS) {   // wave c: rows of class c in front of this block, and in all
        int before = 0, total = 0;
        for (int b = lane; b < nblk; b += 64) { const int v = blk[wave * nblk + b]; total += v; if (b < (int)blockIdx.x) before += v; }
        before = wave_sum_i(before); total = wave_sum_i(total);
        if (lane == 0) { before_s[wave] = before; total_s[wave] = total; }
    }
    __syncthreads();
    const int n_keep = total_s[0], n_split = total_s[1], n_ss = total_s[2], n_ds = total_s[3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int v[GPS_DENSIFY_COUNTS] = {n_keep + 2 * n_ss + n_ds, n_split, n_ss, n_ds, n_keep};
        for (int k = 0; k < GPS_DENSIFY_COUNTS; k++) { counts[k] = v[k]; if (host_counts) host_counts[k] = v[k]; }
    }
    const int i = blockIdx.x * DP_THREADS + threadIdx.x;
    const uint8_t f = i < N ? flags[i] : 0;
    int rank[NCLS], tot;
#pragma unroll
    for (int c = 0; c < NCLS; c++) rank[c] = before_s[c] + block_excl_scan<DP_THREADS>((f >> c) & 1, ws, tot);
    if (f & F_KEEP) dst_src[rank[0]] = i;
    if (f & F_SPLIT_SURV) {
        const int d = n_keep + rank[2];
        dst_src[d] = i; dst_src[d + n_ss] = i;
        dst_sample[d] = rank[1]; dst_sample[d + n_ss] = n_split + rank[1];
    }
    if (f & F_DUP_SURV) dst_src[n_keep + 2 * n_ss + rank[3]] = i;
}

struct ApplyArgs {
    const float* src[6]; float* dst[6];
    const float* m_src[6]; float* m_dst[6];
    const float* v_src[6]; float* v_dst[6];
    int row[6];
    int64_t end[6];
    int n_keep, child_end, n_ss;
    int moments;
    const float* samples;
    const int32_t *dst_src, *dst_sample;
};

// element e of the destination tensors (means | log_scales | quats | sh_dc | sh_rest | opac_logit, each M rows)
__global__ __launch_bounds__(256) void apply_kernel(ApplyArgs a) {
    const int64_t total = a.end[5];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < 5; k++) s += e >= a.end[k] ? 1 : 0;
        const float* src = a.src[0]; float* dst = a.dst[0]; const float* ms = a.m_src[0]; float* md = a.m_dst[0];
        const float* vs = a.v_src[0]; float* vd = a.v_dst[0]; int row = a.row[0]; int64_t first = 0;
#pragma unroll
        for (int k = 1; k < 6; k++)   // (static indices: no scratch copy of the argument arrays)
            if (s == k) { src = a.src[k]; dst = a.dst[k]; ms = a.m_src[k]; md = a.m_dst[k]; vs = a.v_src[k]; vd = a.v_dst[k]; row = a.row[k]; first = a.end[k - 1]; }
        const int64_t le = e - first;
        const int d = (int)(le / row), c = (int)(le - (int64_t)d * row);
        const int p = a.dst_src[d];
        const int64_t from = (int64_t)p * row + c;
        const bool kept = d < a.n_keep, child = !kept && d < a.child_end;
        float val;
        if (child && s == 0) {
            // mean = R(q / |q|) (exp(s) * z) + mean_p   (quatToRotMat, tensor_math.cpp:83-103: q = (w, x, y, z))
            const float* q = a.src[2] + 4 * (int64_t)p;
            const float* ls = a.src[1] + 3 * (int64_t)p;
            const float* z = a.samples + 3 * (int64_t)a.dst_sample[d];
            const float inv = 1.0f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
            const float w = q[0] * inv, x = q[1] * inv, y = q[2] * inv, zz = q[3] * inv;
            const float t0 = expf(ls[0]) * z[0], t1 = expf(ls[1]) * z[1], t2 = expf(ls[2]) * z[2];
            float r0, r1, r2;
            if (c == 0) { r0 = 1.f - 2.f * (y * y + zz * zz); r1 = 2.f * (x * y - w * zz); r2 = 2.f * (x * zz + w * y); }
            else if (c == 1) { r0 = 2.f * (x * y + w * zz); r1 = 1.f - 2.f * (x * x + zz * zz); r2 = 2.f * (y * zz - w * x); }
            else { r0 = 2.f * (x * zz - w * y); r1 = 2.f * (y * zz + w * x); r2 = 1.f - 2.f * (x * x + y * y); }
            val = (r0 * t0 + r1 * t1 + r2 * t2) + src[from];
        } else if (child && s == 1) {
            val = child_log_scale(src[from]);
        } else {
            val = src[from];
        }
        dst[le] = val;
        if (a.moments) {
            md[le] = kept ? ms[from] : 0.0f;
            vd[le] = kept ? vs[from] : 0.0f;
        }
    }
}

}  // namespace

extern "C" {

int gps_densify_accumulate(int N, const float* v_means2d, const int32_t* radii, int width, int height, float* grad_sum,
                           float* vis_count, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(N >= 0 && width > 0 && height > 0);
    if (N == 0) return GPS_OK;
    GPS_REQUIRE(v_means2d && radii && grad_sum && vis_count && (((uintptr_t)v_means2d) & 7) == 0);
    accumulate_kernel<<<gps_div_up(N, 256), 256, 0, (hipStream_t)stream>>>(N, reinterpret_cast<const float2*>(v_means2d), radii,
                                                                          0.5f * (float)width, 0.5f * (float)height, grad_sum, vis_count);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int64_t gps_densify_plan_workspace_bytes(int N) {
    if (N < 0) return GPS_ERR_ARG;
    const int64_t nblk = gps_div_up(N, DP_THREADS);
    return (int64_t)sizeof(int32_t) * NCLS * (nblk + 1) + N;
}

int gps_densify_plan(int N, const float* grad_sum, const float* vis_count, const float* log_scales, const float* opac_logit,
                     float grad_thres, float split_scale, float prune_opac, float prune_scale, int32_t* dst_src, int32_t* dst_sample,
                     int64_t dst_capacity, int32_t* counts, int32_t* host_counts, void* workspace, int64_t workspace_bytes,
                     gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(N >= 0 && counts && workspace && dst_capacity >= 0);
    GPS_REQUIRE(N == 0 || (grad_sum && vis_count && log_scales && opac_logit && dst_src && dst_sample));
    if (workspace_bytes < gps_densify_plan_workspace_bytes(N) || dst_capacity < 2 * (int64_t)N) return GPS_ERR_CAPACITY;
    if (N == 0) {   // nothing to launch: the host words are zeroed here, the device words are left alone
        if (host_counts) for (int k = 0; k < GPS_DENSIFY_COUNTS; k++) host_counts[k] = 0;
        return GPS_OK;
    }
    const int nblk = gps_div_up(N, DP_THREADS);
    int32_t* blk = (int32_t*)workspace;
    uint8_t* flags = (uint8_t*)(blk + (int64_t)NCLS * (nblk + 1));
    hipStream_t s = (hipStream_t)stream;
    const PlanArgs a = {N, grad_sum, vis_count, log_scales, opac_logit, grad_thres, split_scale, prune_opac, prune_scale};
    plan_count_kernel<<<nblk, DP_THREADS, 0, s>>>(a, flags, blk, nblk);
    plan_write_kernel<<<nblk, DP_THREADS, 0, s>>>(N, flags, blk, nblk, dst_src, dst_sample, counts, host_counts);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int gps_densify_apply(int N, int K, int M, int n_split, int n_split_surviving, int n_dup_surviving, int n_keep,
                      const int32_t* dst_src, const int32_t* dst_sample, const float* samples, const float* const* src_params,
                      float* const* dst_params, const float* const* src_m, float* const* dst_m, const float* const* src_v,
                      float* const* dst_v, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(N >= 0 && K >= 1 && M >= 0 && n_split >= 0 && n_split_surviving >= 0 && n_dup_surviving >= 0 && n_keep >= 0);
    GPS_REQUIRE(n_split_surviving <= n_split && (int64_t)n_keep + n_split <= N && n_dup_surviving <= n_keep);
    GPS_REQUIRE((int64_t)M == (int64_t)n_keep + 2 * (int64_t)n_split_surviving + n_dup_surviving);
    GPS_REQUIRE(n_split == 0 || samples != nullptr);
    const bool moments = src_m || dst_m || src_v || dst_v;
    GPS_REQUIRE(!moments || (src_m && dst_m && src_v && dst_v));
    if (M == 0) return GPS_OK;
    GPS_REQUIRE(dst_src && src_params && dst_params && (n_split_surviving == 0 || dst_sample));
    const int rows[6] = {3, 3, 4, 3, 3 * (K - 1), 1};
    ApplyArgs a = {};
    int64_t run = 0;
    for (int k = 0; k < 6; k++) {
        if (rows[k] > 0) {
            GPS_REQUIRE(src_params[k] && dst_params[k] && src_params[k] != dst_params[k]);
            GPS_REQUIRE(!moments || (src_m[k] && dst_m[k] && src_v[k] && dst_v[k] && src_m[k] != dst_m[k] && src_v[k] != dst_v[k]));
        }
        a.src[k] = src_params[k]; a.dst[k] = dst_params[k];
        if (moments) { a.m_src[k] = src_m[k]; a.m_dst[k] = dst_m[k]; a.v_src[k] = src_v[k]; a.v_dst[k] = dst_v[k]; }
        a.row[k] = rows[k] > 0 ? rows[k] : 1;   // (an empty tensor has no element: its row length is never divided by)
        run += (int64_t)M * rows[k];
        a.end[k] = run;
    }
    a.n_keep = n_keep; a.n_ss = n_split_surviving; a.child_end = n_keep + 2 * n_split_surviving;
    a.moments = moments ? 1 : 0;
    a.samples = samples; a.dst_src = dst_src; a.dst_sample = dst_sample;
    apply_kernel<<<(int)min((int64_t)8192, (int64_t)gps_div_up(run, 256)), 256, 0, (hipStream_t)stream>>>(a);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

}  // extern "C"
