// Exact sub-quadratic distCUDA2 for large point sets (gps_knn_mean_dist2_grid): mean squared distance to the 3 nearest
// neighbours, the same numbers as the tiled brute force of splat_init.hip (gps_knn_mean_dist2) bit for bit.
//
// The reference (gsplat/rasterizer/simple_knn.cu:67-227) sorts the points along a Morton curve, boxes every 1024 of them and
// prunes boxes by their distance to the query.  On this path the points are samples of SURFACES seen by a depth camera (a first
// keyframe or a newly revealed room adds up to 0.25 x W x H of them: 76,800 at 640x480, 230,400 at 720p), so a uniform grid over
// their bounding box is the better fit for a wide machine: a counting sort by cell (histogram, scan, scatter -- no comparison
// sort, no cub), then eight lanes per point IN CELL ORDER that search the point's own cell and grow the searched cube ring by ring
// until the third-best distance found is no larger than the distance to the nearest face of the cube that still has grid behind
// it -- the exact termination test, so the result is the brute force's: the three smallest squared distances are a set
// property, both kernels keep them sorted ascending and add them in that order, and both compute a squared distance with
// knn_dist2() (one explicit fma chain).  Neighbouring lanes sit in the same or adjacent cells and walk the same candidate
// runs: their loads are broadcasts out of L2.
//
// The grid itself (bounding box, cell size, counting sort) is knn_grid.hpp, shared with geom_nn.hip.
#include <float.h>

#include "common.hpp"
#include "knn_grid.hpp"
#include "splat_knn.hpp"

namespace {


// (6) KQ_LANES lanes per point, points in cell order.  The lanes of a point walk the same cells and split every run of
// candidates between them (candidate lo + lane, + KQ_LANES, ...): KQ_LANES independent loads in flight per point instead of one
// dependent chain -- one lane per point made the search latency-bound (94 us for 5 k points: ~100 candidates x one L2 round
// trip each).  Every lane keeps the three smallest distances of ITS candidates; the termination test and the result use their
// merge (three xor-shuffles; the private triples are never overwritten, so no candidate is counted twice).
constexpr int KQ_LANES = 8;
__device__ __forceinline__ void merge3(float& b0, float& b1, float& b2) {
#pragma unroll
    for (int o = 1; o < KQ_LANES; o <<= 1) {
        const float o0 = __shfl_xor(b0, o, 64), o1 = __shfl_xor(b1, o, 64), o2 = __shfl_xor(b2, o, 64);
        gps::keep3(o0, b0, b1, b2); gps::keep3(o1, b0, b1, b2); gps::keep3(o2, b0, b1, b2);
    }
}
__global__ __launch_bounds__(256) void knn_query_kernel(int P, const KnnGrid* __restrict__ grid, const int* __restrict__ starts,
                                                        const float4* __restrict__ sorted, float* __restrict__ out) {
    const int t = (blockIdx.x * blockDim.x + threadIdx.x) / KQ_LANES, sub = threadIdx.x & (KQ_LANES - 1);
    if (t >= P) return;   // (whole sub-groups leave together: the shuffles below stay inside a sub-group)
    const KnnGrid g = *grid;
    const float4 q = sorted[t];
    const int self = __float_as_int(q.w);
    const int cx = cell_coord(q.x, g.minx, g.inv_h, g.gx), cy = cell_coord(q.y, g.miny, g.inv_h, g.gy),
              cz = cell_coord(q.z, g.minz, g.inv_h, g.gz);
    float b0 = FLT_MAX, b1 = FLT_MAX, b2 = FLT_MAX;   // of this lane's candidates
    float m0 = FLT_MAX, m1 = FLT_MAX, m2 = FLT_MAX;   // merged over the point's lanes
    if (!(fabsf(q.x) <= FLT_MAX) || !(fabsf(q.y) <= FLT_MAX) || !(fabsf(q.z) <= FLT_MAX)) {
        // a NaN / inf query is at no finite distance from anything: the brute force leaves its three slots at FLT_MAX (every
        // comparison fails) -- the same expression here, without walking the whole grid for it
        if (sub == 0) out[self] = (m0 + m1 + m2) / 3.0f;
        return;
    }
    auto scan_run = [&](int lo, int hi) {
        for (int k = lo + sub; k < hi; k += KQ_LANES) {
            const float4 c = sorted[k];
            if (__float_as_int(c.w) == self) continue;
            gps::keep3(gps::knn_dist2(c.x - q.x, c.y - q.y, c.z - q.z), b0, b1, b2);
        }
    };
    // a point's computed cell can differ from its exact one by rounding at a face: the faces of the searched cube are trusted only
    // up to a margin of 1 % of a cell (the coordinate error is < 1e-4 cells at <= 1024 cells per axis)
    // -- plus, for point sets far from the origin relative to their extent, the rounding of the coordinates themselves: the face
    // distances are taken in the grid's own frame (q - min, one rounding of |q|'s magnitude) and the margin grows by a few ulps of
    // the largest coordinate magnitude in the box
    const float reach = fmaxf(fmaxf(fmaxf(fabsf(g.minx), fabsf(g.minx + (float)g.gx * g.h)), fmaxf(fabsf(g.miny), fabsf(g.miny + (float)g.gy * g.h))),
                              fmaxf(fabsf(g.minz), fabsf(g.minz + (float)g.gz * g.h)));
    const float margin = 0.01f * g.h + 4.0f * 1.1920929e-7f * reach;
    const float sx = q.x - g.minx, sy = q.y - g.miny, sz = q.z - g.minz;
    for (int r = 0;; r++) {
        const int x0 = max(cx - r, 0), x1 = min(cx + r, g.gx - 1), y0 = max(cy - r, 0), y1 = min(cy + r, g.gy - 1),
                  z0 = max(cz - r, 0), z1 = min(cz + r, g.gz - 1);
        for (int z = z0; z <= z1; z++)
            for (int y = y0; y <= y1; y++) {
                // the shell of ring r: whole x-runs on its z / y faces, the two end cells elsewhere
                const bool face = (z == cz - r) | (z == cz + r) | (y == cy - r) | (y == cy + r);
                const int row = g.gx * (y + g.gy * z);
                if (face) {
                    scan_run(starts[row + x0], starts[row + x1 + 1]);   // cells x0..x1 of a row are consecutive: one run of sorted points
                } else {
                    if (cx - r >= 0) scan_run(starts[row + cx - r], starts[row + cx - r + 1]);
                    if (cx + r < g.gx) scan_run(starts[row + cx + r], starts[row + cx + r + 1]);
                }
            }
        m0 = b0; m1 = b1; m2 = b2;
        merge3(m0, m1, m2);
        // distance from the query to the nearest face of the searched cube that has grid behind it
        float dmin = FLT_MAX;
        bool open = false;
        if (cx - r > 0) { open = true; dmin = fminf(dmin, sx - (float)(cx - r) * g.h); }
        if (cx + r < g.gx - 1) { open = true; dmin = fminf(dmin, (float)(cx + r + 1) * g.h - sx); }
        if (cy - r > 0) { open = true; dmin = fminf(dmin, sy - (float)(cy - r) * g.h); }
        if (cy + r < g.gy - 1) { open = true; dmin = fminf(dmin, (float)(cy + r + 1) * g.h - sy); }
        if (cz - r > 0) { open = true; dmin = fminf(dmin, sz - (float)(cz - r) * g.h); }
        if (cz + r < g.gz - 1) { open = true; dmin = fminf(dmin, (float)(cz + r + 1) * g.h - sz); }
        if (!open) break;                       // the cube covers the grid
        dmin -= margin;
        if (dmin > 0.f && m2 <= dmin * dmin) break;   // nothing outside the cube can be closer than the third best
    }
    if (sub == 0) out[self] = (m0 + m1 + m2) / 3.0f;
}

}  // namespace

extern "C" {

int64_t gps_knn_grid_workspace_bytes(int P) { return P < 0 ? (int64_t)GPS_ERR_ARG : knn_index_bytes(P); }

int gps_knn_mean_dist2_grid(int P, const float* points, float* mean_dist2, void* workspace, int64_t workspace_bytes, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(P >= 0);
    if (P == 0) return GPS_OK;
    GPS_REQUIRE(points && mean_dist2 && workspace && (reinterpret_cast<uintptr_t>(workspace) & 15) == 0);
    GPS_REQUIRE(workspace_bytes >= gps_knn_grid_workspace_bytes(P));
    hipStream_t st = (hipStream_t)stream;
    const KnnWs w = knn_ws(workspace, P);
    float* partials = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + knn_ws_bytes(P));
    knn_build_index(P, points, w, partials, st);
    knn_query_kernel<<<gps_div_up((int64_t)P * KQ_LANES, 256), 256, 0, st>>>(P, w.grid, w.starts, w.sorted, mean_dist2);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

}  // extern "C"
