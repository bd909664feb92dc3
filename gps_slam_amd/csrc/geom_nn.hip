// Exact nearest neighbour between two DIFFERENT point sets (gps_nn_index_build / gps_nn_query): for every query point the
// squared distance to, and the index of, the nearest of R reference points.  This is the KD-tree query of the reference's
// geometry evaluation (scripts/geo_general.py: accuracy / completion and their ratios, two 10^6-point clouds), as device work.
//
// The index is the uniform grid of knn_grid.hpp over the reference set (shared with splat_knn.hip).  The query kernel is the
// ring search of splat_knn.hip's knn_query_kernel with these differences:
//   * queries come from another set, in caller order: no self-skip, the walk starts at the query's CLAMPED cell;
//   * a query may lie outside the grid's box by any finite amount: see the face distances below;
//   * one neighbour, with its index; ties in the squared distance resolve to the LOWEST original index (the scatter's atomic
//     order differs from run to run: without the rule the index output would not be reproducible);
//   * the squared distance is knn_dist2 of differences of the ORIGINAL coordinates, so its error is relative to the distance;
//   * bounded work: after NN_MAX_RINGS rings an unfinished query is appended to a list and a second launch finishes the listed
//     queries by tiled brute force over all R points (same distance expression, same tie rule: the same answer).
// A squared distance that overflows float is +inf and selects nothing (index -1), like a non-finite point.
#include <float.h>
#include <math.h>

#include "common.hpp"
#include "knn_grid.hpp"
#include "splat_knn.hpp"

// rings searched around the query's cell before the query goes to the brute force (ring r costs O(r^2) row lookups)
#ifndef GPS_NN_MAX_RINGS
#define GPS_NN_MAX_RINGS 6
#endif
GPS_TUNABLE_REPORT(GPS_NN_MAX_RINGS, 6);

namespace {

constexpr int NN_MAX_RINGS = GPS_NN_MAX_RINGS;
constexpr int NQ_LANES = 8;

struct NnQueryWs {        // header (16 bytes) | list[Q]
    int* n_far;           // queries the ring search did not finish
    int* far_list;
};
static inline int64_t nn_query_ws_bytes(int Q) { return 16 + align16(4 * (int64_t)Q); }
static inline NnQueryWs nn_query_ws(void* base) {
    NnQueryWs w;
    w.n_far = reinterpret_cast<int*>(base);
    w.far_list = reinterpret_cast<int*>(reinterpret_cast<char*>(base) + 16);
    return w;
}

__device__ __forceinline__ bool finite3(float x, float y, float z) {
    return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX;
}
// candidate (d, i) replaces (bd, bi) when nearer, or as near with a lower index; NaN / +inf distances never do
__device__ __forceinline__ void keep1(float d, int i, float& bd, int& bi) {
    if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
}

// NQ_LANES lanes per query.  The lanes of a query walk the same cells and split every run of candidates between them, each
// keeps the best of ITS candidates; the termination test and the result use their merge (three xor-shuffles inside the query's
// lanes, which run the loops below in lockstep: every loop bound depends on merged values only).
__global__ __launch_bounds__(256) void nn_query_kernel(int Q, const float* __restrict__ queries, const KnnGrid* __restrict__ grid,
                                                       const int* __restrict__ starts, const float4* __restrict__ sorted,
                                                       float* __restrict__ dist2, int32_t* __restrict__ nn_index,
                                                       int* __restrict__ n_far, int* __restrict__ far_list) {
    const int64_t t64 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / NQ_LANES;
    const int sub = threadIdx.x & (NQ_LANES - 1);
    if (t64 >= Q) return;   // (whole sub-groups leave together: the shuffles below stay inside a sub-group)
    const int t = (int)t64;
    const KnnGrid g = *grid;
    const float qx = queries[3 * t64], qy = queries[3 * t64 + 1], qz = queries[3 * t64 + 2];
    float bd = INFINITY, md = INFINITY;   // of this lane's candidates / merged over the query's lanes
    int bi = -1, mi = -1;
    bool far = false;
    // a NaN / inf query is at no finite distance from anything: +inf and -1 without walking the grid
    if (finite3(qx, qy, qz)) {
        const int cx = cell_coord(qx, g.minx, g.inv_h, g.gx), cy = cell_coord(qy, g.miny, g.inv_h, g.gy),
                  cz = cell_coord(qz, g.minz, g.inv_h, g.gz);
        auto scan_run = [&](int lo, int hi) {
            for (int k = lo + sub; k < hi; k += NQ_LANES) {
                const float4 c = sorted[k];
                keep1(gps::knn_dist2(c.x - qx, c.y - qy, c.z - qz), __float_as_int(c.w), bd, bi);
            }
        };
        // The faces of the searched cube are trusted up to a margin: 1 % of a cell for the rounding of a computed cell at a face,
        // plus a few ulps of the largest coordinate magnitude involved -- the box's corners AND the query's own coordinates (the
        // face distances are taken in the grid's frame, q - min: one rounding of |q|'s magnitude, and |q| is unbounded here).
        const float reach = fmaxf(fmaxf(fmaxf(fmaxf(fabsf(g.minx), fabsf(g.minx + (float)g.gx * g.h)), fmaxf(fabsf(g.miny), fabsf(g.miny + (float)g.gy * g.h))),
                                        fmaxf(fabsf(g.minz), fabsf(g.minz + (float)g.gz * g.h))),
                                  fmaxf(fmaxf(fabsf(qx), fabsf(qy)), fabsf(qz)));
        const float margin = 0.01f * g.h + 4.0f * 1.1920929e-7f * reach;
        // Position in the grid's frame.  Outside the box these are negative or beyond g * h, and the cell is the clamped one.  A
        // face distance below is taken only on a side that still has grid behind it: on the low side that needs c - r > 0, so
        // the query is not below the box on that axis (its clamped cell would be 0) and s - (c - r) h is its distance to that
        // plane, however far ABOVE the box it lies; likewise on the high side.  Both stay lower bounds for every finite query.
        const float sx = qx - g.minx, sy = qy - g.miny, sz = qz - g.minz;
        far = true;
        for (int r = 0; r <= NN_MAX_RINGS; r++) {
            const int x0 = max(cx - r, 0), x1 = min(cx + r, g.gx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.gy - 1),
                      z0 = max(cz - r, 0), z1 = min(cz + r, g.gz - 1);
            for (int z = z0; z <= z1; z++)
                for (int y = y0; y <= y1; y++) {
                    // the shell of ring r: whole x-runs on its z / y faces, the two end cells elsewhere
                    const bool face = (z == cz - r) | (z == cz + r) | (y == cy - r) | (y == cy + r);
                    const int row = g.gx * (y + g.gy * z);
                    if (face) {
                        scan_run(starts[row + x0], starts[row + x1 + 1]);   // cells x0..x1 of a row: one run of sorted points
                    } else {
                        if (cx - r >= 0) scan_run(starts[row + cx - r], starts[row + cx - r + 1]);
                        if (cx + r < g.gx) scan_run(starts[row + cx + r], starts[row + cx + r + 1]);
                    }
                }
            md = bd; mi = bi;
#pragma unroll
            for (int o = 1; o < NQ_LANES; o <<= 1) keep1(__shfl_xor(md, o, 64), __shfl_xor(mi, o, 64), md, mi);
            float dmin = FLT_MAX;
            bool open = false;
            if (cx - r > 0) { open = true; dmin = fminf(dmin, sx - (float)(cx - r) * g.h); }
            if (cx + r < g.gx - 1) { open = true; dmin = fminf(dmin, (float)(cx + r + 1) * g.h - sx); }
            if (cy - r > 0) { open = true; dmin = fminf(dmin, sy - (float)(cy - r) * g.h); }
            if (cy + r < g.gy - 1) { open = true; dmin = fminf(dmin, (float)(cy + r + 1) * g.h - sy); }
            if (cz - r > 0) { open = true; dmin = fminf(dmin, sz - (float)(cz - r) * g.h); }
            if (cz + r < g.gz - 1) { open = true; dmin = fminf(dmin, (float)(cz + r + 1) * g.h - sz); }
            if (!open) { far = false; break; }   // the cube covers the grid
            // (the 1e-4 keeps the bound strict against the rounding of the squared distances themselves: a point behind the
            // faces is strictly farther than the best found, so the tie rule never has to look there)
            dmin = (dmin - margin) * 0.9999f;
            if (dmin > 0.f && md <= dmin * dmin) { far = false; break; }
        }
    }
    // unfinished queries: one atomic per wave, not per query (the sub-groups have reconverged here; lanes of the last, part-filled
    // wave that left above are simply absent from the ballot)
    const bool append = far && sub == 0;
    const unsigned long long mask = __ballot(append);
    if (mask) {
        const int leader = __ffsll((long long)mask) - 1;
        int base = 0;
        if (lane_id() == leader) base = atomicAdd(n_far, __popcll(mask));
        base = __shfl(base, leader, 64);
        if (append) far_list[base + __popcll(mask & lanemask_lt())] = t;
    }
    if (sub == 0 && !far) {
        dist2[t] = md;
        if (nn_index) nn_index[t] = mi;
    }
}

// The listed queries against all R points, exactly: one query per lane, 256-point tiles of the index's float4 array staged in
// LDS (every lane reads the same slot: a broadcast), as the brute force of splat_init.hip.  Fixed grid; the number of listed
// queries is read on the device.  Workgroup 0 also writes the statistics.
constexpr int NF_TILE = 256, NF_BLOCKS = 1024;
__global__ __launch_bounds__(NF_TILE) void nn_far_kernel(int R, int Q, const float* __restrict__ queries, const float4* __restrict__ sorted,
                                                         const int* __restrict__ n_far, const int* __restrict__ far_list,
                                                         float* __restrict__ dist2, int32_t* __restrict__ nn_index, int32_t* __restrict__ stats) {
    __shared__ float4 tile[NF_TILE];
    const int n = *n_far;
    if (blockIdx.x == 0 && threadIdx.x == 0 && stats) { stats[0] = Q - n; stats[1] = n; }
    for (int first = blockIdx.x * NF_TILE; first < n; first += NF_BLOCKS * NF_TILE) {   // (uniform per workgroup: barriers inside)
        const int k = first + threadIdx.x;
        const bool live = k < n;
        const int t = live ? far_list[k] : 0;
        const float qx = live ? queries[3 * (int64_t)t] : 0.f, qy = live ? queries[3 * (int64_t)t + 1] : 0.f,
                    qz = live ? queries[3 * (int64_t)t + 2] : 0.f;
        float bd = INFINITY;
        int bi = -1;
        for (int base = 0; base < R; base += NF_TILE) {
            const int j = base + threadIdx.x;
            __syncthreads();
            if (j < R) tile[threadIdx.x] = sorted[j];
            __syncthreads();
            const int m = min(NF_TILE, R - base);
#pragma unroll 4
            for (int s = 0; s < m; s++) {
                const float4 c = tile[s];
                keep1(gps::knn_dist2(c.x - qx, c.y - qy, c.z - qz), __float_as_int(c.w), bd, bi);
            }
        }
        if (live) {
            dist2[t] = bd;
            if (nn_index) nn_index[t] = bi;
        }
    }
}

}  // namespace

extern "C" {

int64_t gps_nn_index_workspace_bytes(int R) { return R < 0 ? (int64_t)GPS_ERR_ARG : knn_index_bytes(R); }

int gps_nn_index_build(int R, const float* ref_points, void* ws, int64_t ws_bytes, gps_stream stream) {
    GPS_REQUIRE(R > 0);
    GPS_ENTER();
    GPS_REQUIRE(ref_points && ws && (reinterpret_cast<uintptr_t>(ws) & 15) == 0);
    if (ws_bytes < knn_index_bytes(R)) return GPS_ERR_CAPACITY;
    const KnnWs w = knn_ws(ws, R);
    float* partials = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + knn_ws_bytes(R));
    knn_build_index(R, ref_points, w, partials, (hipStream_t)stream);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int64_t gps_nn_query_workspace_bytes(int Q) { return Q < 0 ? (int64_t)GPS_ERR_ARG : nn_query_ws_bytes(Q); }

int gps_nn_query(int R, const void* index_ws, int Q, const float* query_points, float* dist2, int32_t* nn_index, int32_t* stats,
                 void* query_ws, int64_t query_ws_bytes, gps_stream stream) {
    GPS_REQUIRE(R > 0 && Q >= 0);
    if (Q == 0) return GPS_OK;
    GPS_ENTER();
    GPS_REQUIRE(index_ws && (reinterpret_cast<uintptr_t>(index_ws) & 15) == 0 && query_points && dist2);
    GPS_REQUIRE(query_ws && (reinterpret_cast<uintptr_t>(query_ws) & 15) == 0);
    if (query_ws_bytes < nn_query_ws_bytes(Q)) return GPS_ERR_CAPACITY;
    hipStream_t st = (hipStream_t)stream;
    const KnnWs w = knn_ws(const_cast<void*>(index_ws), R);
    const NnQueryWs qw = nn_query_ws(query_ws);
    if (hipMemsetAsync(qw.n_far, 0, 16, st) != hipSuccess) return GPS_ERR_LAUNCH;
    nn_query_kernel<<<gps_div_up((int64_t)Q * NQ_LANES, 256), 256, 0, st>>>(Q, query_points, w.grid, w.starts, w.sorted, dist2, nn_index,
                                                                          qw.n_far, qw.far_list);
    nn_far_kernel<<<NF_BLOCKS, NF_TILE, 0, st>>>(R, Q, query_points, w.sorted, qw.n_far, qw.far_list, dist2, nn_index, stats);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

}  // extern "C"
