// Voxel access through the block hash (ITMRepresentationAccess.h), shared by the dense raycaster and the colour pass
// (tsdf_render.hip) and by the sparse cast of the forward render (tsdf_forward.hip).  Everything here is force-inlined.
// Files including this header are compiled with -ffp-contract=off.
#pragma once
#include "tsdf_common.hpp"

namespace gpst {

// ---------------------------------------------------------------- voxel access (ITMRepresentationAccess.h)
struct BlockCache { int bx, by, bz, ptr; };

__device__ __forceinline__ int floor_div_blk(int v) { return v >> 3; }  // floor(v / 8): arithmetic shift (BLK == 8)

// findVoxel (ITMRepresentationAccess.h:81-113) split into "which block" and "which voxel".  resolve_with_head returns
// the first voxel index of block (bx,by,bz) or -1 with the reference's cache and vmIndex side effects (cache hit ->
// vmIndex = 1; hash hit -> vmIndex = entry + 1 and the cache moves; miss -> vmIndex = 0).  The bucket-head entry is
// passed in: callers fetch the heads of everything they are about to look up in ONE batch of independent loads, then
// replay the lookups in the reference's order from registers (only excess-list chains, which are rare, cost further
// round trips), then issue the voxel loads together.  A wave therefore pays ~2 memory round trips per lookup group
// instead of one per lane-divergent branch.
__device__ __forceinline__ int resolve_with_head(const TsdfState& s, int bx, int by, int bz, HashEntry he, int hashIdx,
                                                 int& vmIndex, BlockCache& c) {
    if (bx == c.bx && by == c.by && bz == c.bz) { vmIndex = 1; return c.ptr; }  // :89-93 (vmIndex = true)
    while (true) {
        if (entry_is(he, bx, by, bz) & (he.ptr >= 0)) {
            c.bx = bx; c.by = by; c.bz = bz; c.ptr = he.ptr * BLK3;
            vmIndex = hashIdx + 1;
            return c.ptr;
        }
        if (he.offset < 1) break;
        hashIdx = s.n_buckets + he.offset - 1;
        he = load_entry(s.hash, hashIdx);
    }
    vmIndex = 0;
    return -1;
}

__device__ __forceinline__ int resolve_block(const TsdfState& s, int px, int py, int pz, int& lin, int& vmIndex,
                                             BlockCache& c) {
    const int bx = floor_div_blk(px), by = floor_div_blk(py), bz = floor_div_blk(pz);
    lin = px + (py - bx) * BLK + (pz - by) * BLK * BLK - bz * BLK3;
    if (bx == c.bx && by == c.by && bz == c.bz) { vmIndex = 1; return c.ptr; }
    const int hashIdx = hash_index(bx, by, bz, s.n_buckets - 1);
    return resolve_with_head(s, bx, by, bz, load_entry(s.hash, hashIdx), hashIdx, vmIndex, c);
}

constexpr uint64_t EMPTY_VOXEL = 0x7FFFull;  // TVoxel(): sdf 32767, weights / colour 0

__device__ __forceinline__ uint64_t read_voxel_raw(const TsdfState& s, int px, int py, int pz, int& vmIndex,
                                                   BlockCache& c) {
    int lin;
    const int base = resolve_block(s, px, py, pz, lin, vmIndex, c);
    return base >= 0 ? reinterpret_cast<const uint64_t*>(s.vba)[base + lin] : EMPTY_VOXEL;
}
__device__ __forceinline__ float vox_sdf(uint64_t raw) { return (float)(int16_t)(raw & 0xFFFF); }
__device__ __forceinline__ float vox_wdepth(uint64_t raw) { return (float)((raw >> 16) & 0xFF); }
__device__ __forceinline__ float roundf_ref(float x) { return (x < 0) ? (x - 0.5f) : (x + 0.5f); }

// the trilinear blend of readFromSDF_float_interpolated, in the reference's operation order; r[dx + 2*dy + 4*dz]
template <bool WITH_CONF>
__device__ __forceinline__ float blend_corners(const uint64_t (&r)[8], float cx, float cy, float cz, float& conf) {
    float res1 = (1.0f - cx) * vox_sdf(r[0]) + cx * vox_sdf(r[1]);
    res1 = (1.0f - cy) * res1 + cy * ((1.0f - cx) * vox_sdf(r[2]) + cx * vox_sdf(r[3]));
    float res2 = (1.0f - cx) * vox_sdf(r[4]) + cx * vox_sdf(r[5]);
    res2 = (1.0f - cy) * res2 + cy * ((1.0f - cx) * vox_sdf(r[6]) + cx * vox_sdf(r[7]));
    if (WITH_CONF) {
        float c1 = (1.0f - cx) * vox_wdepth(r[0]) + cx * vox_wdepth(r[1]);
        c1 = (1.0f - cy) * c1 + cy * ((1.0f - cx) * vox_wdepth(r[2]) + cx * vox_wdepth(r[3]));
        float c2 = (1.0f - cx) * vox_wdepth(r[4]) + cx * vox_wdepth(r[5]);
        c2 = (1.0f - cy) * c2 + cy * ((1.0f - cx) * vox_wdepth(r[6]) + cx * vox_wdepth(r[7]));
        conf = (1.0f - cz) * c1 + cz * c2;
    }
    return ((1.0f - cz) * res1 + cz * res2) / 32767.0f;
}

// readFromSDF_float_interpolated / readWithConfidenceFromSDF_float_interpolated (ITMRepresentationAccess.h:117-187).
// The reference reads the eight corners one after the other through the block cache.  Here:
//  * cell inside one block (local coordinates <= 6, 67% of cells): after the first lookup either the cache holds that
//    block and all eight voxels are loaded together, or the block is unallocated and the other seven lookups would fail
//    exactly like the first (no side effects, cache untouched);
//  * cell straddling blocks: the eight bucket heads are fetched together, the eight lookups are replayed in the
//    reference's order from registers (identical cache evolution), then the eight voxels are loaded together.
// the eight voxels of the interpolation cell at (ix, iy, iz), x fastest: r[dx + 2*dy + 4*dz]; unallocated -> EMPTY_VOXEL
__device__ __forceinline__ void fetch_cell(const TsdfState& s, int ix, int iy, int iz, int& vmIndex, BlockCache& c, uint64_t (&r)[8]) {
    const uint64_t* vox = reinterpret_cast<const uint64_t*>(s.vba);
    if ((ix & 7) < 7 && (iy & 7) < 7 && (iz & 7) < 7) {
        int lin;
        const int base = resolve_block(s, ix, iy, iz, lin, vmIndex, c);
        if (base >= 0) {
            const uint64_t* v = vox + base + lin;
            r[0] = v[0]; r[1] = v[1]; r[2] = v[BLK]; r[3] = v[BLK + 1];
            r[4] = v[BLK * BLK]; r[5] = v[BLK * BLK + 1]; r[6] = v[BLK * BLK + BLK]; r[7] = v[BLK * BLK + BLK + 1];
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) r[k] = EMPTY_VOXEL;
        }
    } else {
        int kx[8], ky[8], kz[8], hidx[8], idx[8];
        uint4 hraw[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            kx[k] = floor_div_blk(ix + (k & 1)); ky[k] = floor_div_blk(iy + ((k >> 1) & 1));
            kz[k] = floor_div_blk(iz + (k >> 2));
            hidx[k] = hash_index(kx[k], ky[k], kz[k], s.n_buckets - 1);
            hraw[k] = load_raw(s.hash, hidx[k]);
        }
#pragma unroll
        for (int k = 0; k < 8; k += 2) pin(hraw[k], hraw[k + 1]);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int vx = ix + (k & 1), vy = iy + ((k >> 1) & 1), vz = iz + (k >> 2);
            const int lin = vx + (vy - kx[k]) * BLK + (vz - ky[k]) * BLK * BLK - kz[k] * BLK3;
            const int base = resolve_with_head(s, kx[k], ky[k], kz[k], decode_entry(hraw[k]), hidx[k], vmIndex, c);
            idx[k] = base >= 0 ? base + lin : -1;
        }
        uint64_t t[8];
#pragma unroll
        for (int k = 0; k < 8; k++) t[k] = vox[idx[k] >= 0 ? idx[k] : 0];  // unconditional: one batch, no branches
#pragma unroll
        for (int k = 0; k < 8; k++) r[k] = idx[k] >= 0 ? t[k] : EMPTY_VOXEL;
    }
}

template <bool WITH_CONF>
__device__ __forceinline__ float read_sdf_interp(const TsdfState& s, float px, float py, float pz, int& vmIndex,
                                                 BlockCache& c, float& conf) {
    const float fx_ = floorf(px), fy_ = floorf(py), fz_ = floorf(pz);
    const float cx = px - fx_, cy = py - fy_, cz = pz - fz_;
    uint64_t r[8];  // x fastest: r[dx + 2*dy + 4*dz]
    fetch_cell(s, (int)fx_, (int)fy_, (int)fz_, vmIndex, c, r);
    vmIndex = 1;
    return blend_corners<WITH_CONF>(r, cx, cy, cz, conf);
}

}  // namespace gpst
