// Per-frame exposure compensation (use_exposure; raw_gs_model.cpp:331-346): one camera's [3,4] affine colour transform E applied
// to the composed `ges` image,  out[i] = sum_j rgb[j] E[i][j] + E[i][3].  The arithmetic every kernel of the feature shares (the
// forward rasterizer's exposure epilogue in splat_raster.hip, the loss-terms stage in splat_loss.hip, the operator-level kernels and
// the table's reduce + Adam step in splat_exposure.hip).  Every multiply-add is spelled out (fmaf, or a product and a sum that no
// fmaf joins), so the compiler has no contraction left to choose per call site: all routes round alike and give the same bits
// (tests/test_compose_sites_gpu.py).
#pragma once
#include "common.hpp"
#include "splat_adam.hpp"

namespace gps {

constexpr int EXPOSURE_FLOATS = 12;   // one row of the table: E[3][4] row-major

// rgb -> E(rgb)
__device__ __forceinline__ void exposure_apply(const float (&E)[12], float c0, float c1, float c2, float& o0, float& o1,
                                               float& o2) {
    o0 = fmaf(E[2], c2, fmaf(E[0], c0, E[1] * c1)) + E[3];
    o1 = fmaf(E[6], c2, fmaf(E[4], c0, E[5] * c1)) + E[7];
    o2 = fmaf(E[10], c2, fmaf(E[8], c0, E[9] * c1)) + E[11];
}

// d loss / d rgb = E[:, :3]^T d loss / d out
__device__ __forceinline__ void exposure_vjp(const float (&E)[12], float g0, float g1, float g2, float& v0, float& v1,
                                             float& v2) {
    v0 = fmaf(g2, E[8], fmaf(g0, E[0], g1 * E[4]));
    v1 = fmaf(g2, E[9], fmaf(g0, E[1], g1 * E[5]));
    v2 = fmaf(g2, E[10], fmaf(g0, E[2], g1 * E[6]));
}

// d loss / d E += d loss / d out (x) [rgb, 1]
__device__ __forceinline__ void exposure_grad_acc(float (&ve)[12], float g0, float g1, float g2, float c0, float c1, float c2) {
    ve[0] = fmaf(g0, c0, ve[0]); ve[1] = fmaf(g0, c1, ve[1]); ve[2] = fmaf(g0, c2, ve[2]); ve[3] += g0;
    ve[4] = fmaf(g1, c0, ve[4]); ve[5] = fmaf(g1, c1, ve[5]); ve[6] = fmaf(g1, c2, ve[6]); ve[7] += g1;
    ve[8] = fmaf(g2, c0, ve[8]); ve[9] = fmaf(g2, c1, ve[9]); ve[10] = fmaf(g2, c2, ve[10]); ve[11] += g2;
}

__device__ __forceinline__ void exposure_load(const float* __restrict__ row, float (&E)[12]) {
#pragma unroll
    for (int k = 0; k < 12; k++) E[k] = row[k];
}

// what the forward rasterizer's exposure instance needs on top of gps::FwdCompose
struct FwdExposure {
    const float* row;   // [3,4] of this camera
    float* slab;        // [tiles, 12]: each tile workgroup's sum of d loss / d E (plain stores, summed by the reduce kernel)
};

// splat_exposure.hip: the fixed-order sum of n_partials rows of the slab -> grad[rows,3,4] (zero outside `row`), and with
// table != NULL the Adam step of the whole table (AdamScalars of the table's own step count)
int exposure_reduce_launch(const float* slab, int n_partials, int rows, int row, float* grad, float* table, float* m, float* v,
                           const AdamScalars* sc, gps_stream stream);

}  // namespace gps
