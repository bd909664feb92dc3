// `ges` rasterizer: order-independent depth-cut weighted splat (forward) and the
// Gaussian-parallel backward over each Gaussian's 2r x 2r pixel box.
//
// gps_raster_ges_fwd    <- gsplat::rasterize_to_pixels_fwd_ges_tensor
//                          (gsplat/rasterizer/rasterize_to_pixels_fwd_ges.cu:18-221)
// gps_raster_ges_bwd_gs <- gsplat::rasterize_to_pixels_bwd_ges_gs_parallel_tensor
//                          (gsplat/rasterizer/rasterize_to_pixels_bwd_ges_new_parallel.cu:18-201)
//
// Forward: one 256-thread workgroup (4 wave64) per 16x16 tile; wave w owns pixel
// rows 4w..4w+3.  The tile's sorted Gaussian list is staged through LDS in
// batches of 256 complete records {xy, conic, opacity, depth, rgb} (40 B) so the
// per-pixel loop reads only LDS (broadcast reads, conflict free) -- the
// reference re-reads the depth/colour channels from global memory for every
// (pixel, Gaussian) pair (:165-166).  No MFMA: this is not a contraction.
//
// Backward: the reference gives each 32-lane warp 32 consecutive 32-pixel groups
// and issues 10 atomics per group.  Here a wave64 takes 32 consecutive groups as
// two contiguous runs of 16 (one per half-wave), keeps the 10 partial sums in
// registers while consecutive groups belong to the same Gaussian, and only
// reduces (within the 32-lane half) + atomically adds when the Gaussian changes:
// ~N_visible x 10 atomics instead of n_groups x 10.  Pixel/box semantics
// (int() truncation, +1 offsets, i > y_max guard) are the reference's.
#include "common.hpp"
#include "launch_timing.hpp"
#include "splat_bin.hpp"
#include "splat_compose.hpp"

namespace {

constexpr int TILE_THREADS = 256;


template <int TILE>
__global__ __launch_bounds__(TILE_THREADS) void raster_ges_fwd_kernel(
    const float2* __restrict__ means2d, const float* __restrict__ conics, const float4* __restrict__ colors,
    const float* __restrict__ opacities, const float* __restrict__ ref_depth, int W, int H, int tw, int th,
    const int32_t* __restrict__ tile_offsets, const int32_t* __restrict__ flatten_ids,
    const int64_t* __restrict__ counts, float delta_depth, float4* __restrict__ render_colors,
    float* __restrict__ render_alphas, int32_t* __restrict__ last_ids) {
    static_assert(TILE == 16, "one thread per pixel of a 16x16 tile");
    __shared__ float4 rec0[TILE_THREADS];
    __shared__ float4 rec1[TILE_THREADS];
    __shared__ float2 rec2[TILE_THREADS];

    const int tile_id = blockIdx.x;
    const int ty = tile_id / tw, tx = tile_id - ty * tw;
    const int tid = threadIdx.x;
    const int i = ty * TILE + (tid >> 4), j = tx * TILE + (tid & 15);
    const bool inside = (i < H) && (j < W);
    const float px = (float)j + 0.5f, py = (float)i + 0.5f;
    const int pix = i * W + j;

    const int n_isects = (int)counts[0];
    const int range_start = tile_offsets[tile_id];
    const int range_end = (tile_id == tw * th - 1) ? n_isects : tile_offsets[tile_id + 1];

    // pixels outside the image never pass the depth test
    const float cut = inside ? ref_depth[pix] + delta_depth : -3.0e38f;
    float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, wsum = 0.f;
    int cur_idx = 0;

    for (int batch_start = range_start; batch_start < range_end; batch_start += TILE_THREADS) {
        __syncthreads();  // previous batch fully consumed
        const int idx = batch_start + tid;
        if (idx < range_end) {
            const int g = flatten_ids[idx];
            const float2 xy = means2d[g];
            const float4 c = colors[g];
            const float ca = conics[3 * g], cb = conics[3 * g + 1], cc = conics[3 * g + 2];
            rec0[tid] = make_float4(xy.x, xy.y, ca, cb);
            rec1[tid] = make_float4(cc, opacities[g], c.w, c.x);
            rec2[tid] = make_float2(c.y, c.z);
        }
        __syncthreads();
        const int batch_size = min(TILE_THREADS, range_end - batch_start);
        for (int t = 0; t < batch_size; ++t) {
            const float4 a = rec0[t];
            const float4 b = rec1[t];
            const float dx = a.x - px, dy = a.y - py;
            const float sigma = 0.5f * (a.z * dx * dx + b.x * dy * dy) + a.w * dx * dy;
            const float alpha = fminf(0.999f, b.y * __expf(-sigma));
            const bool hit = !(b.z > cut) && !(sigma < 0.f) && !(alpha < 1.f / 255.f);
            if (hit) {
                const float2 gb = rec2[t];
                o0 += b.w * alpha; o1 += gb.x * alpha; o2 += gb.y * alpha; o3 += b.z * alpha;
                wsum += alpha;
                cur_idx = batch_start + t;
            }
        }
    }
    if (inside) {
        render_colors[pix] = make_float4(o0, o1, o2, o3);
        render_alphas[pix] = wsum;
        if (last_ids) last_ids[pix] = cur_idx;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Forward from the packed per-Gaussian records of gps_gauss_preprocess_fwd (the fused model path), packed math.
// record = 3 x float4: a = {mx, my, ca, cb}  b = {cc, opac, depth, r}  c = {g, b, xbounds, ybounds}, see pack_record() in
// splat_math.hpp.  The pair evaluation is VALU bound (PMC: ~23 wave
// instructions per Gaussian x 64-pixel strip), so the lever is instructions per pixel:
//   * each lane owns TWO horizontally adjacent pixels and evaluates them with v_pk_{add,mul,fma}_f32 -- dy, c*dy^2 and
//     b*dy are shared by the pair, everything in dx and the five accumulators are 2-wide: ~25 VALU per Gaussian for
//     128 pixels instead of ~23 per 64;
//   * the staging step rewrites the record for the inner loop once per tile: conic pre-multiplied by log2(e) (and 1/2),
//     opacity as -log2(opacity) folded into the exponent, so alpha = exp2(-(sigma' - log2 o)) is one v_exp_f32;
//   * a 16x16 tile is covered by two waves (16x8 pixels each); to keep four waves per workgroup in flight the batch's
//     Gaussian list is split in two halves, waves {0,1} and {2,3} each take one, and the partial sums are added
//     through LDS at the end in a fixed order (deterministic; the sum is order independent in exact arithmetic).
typedef float v2f __attribute__((ext_vector_type(2)));

// one pixel of gps_compose_l1 on a render that is still in registers; returns the pixel's |gt - rgb| sum.  EXPO: the camera's
// exposure row E applied to the composed colour c (raw_gs_model.cpp:331-346): rgb := E(c), the L1 sign gradient g is taken on E(c),
// the image gradients come from E^T g, and g (x) [c, 1] is added to ve (d loss / d E)
template <bool EXPO>
__device__ __forceinline__ float compose_l1_pixel(const gps::FwdCompose& fc, [[maybe_unused]] const float (&E)[EXPO ? 12 : 1],
                                                  [[maybe_unused]] float (&ve)[EXPO ? 12 : 1], int p, float4 rc, float w, float cut) {
    const gps::ComposedColor k = gps::compose_color(rc, w, fc.base_color, p);
    float e0 = k.c0, e1 = k.c1, e2 = k.c2;
    if constexpr (EXPO) gps::exposure_apply(E, k.c0, k.c1, k.c2, e0, e1, e2);
    fc.rgb[3 * p] = e0; fc.rgb[3 * p + 1] = e1; fc.rgb[3 * p + 2] = e2;
    const float d0 = fc.gt_rgb[3 * p] - e0, d1 = fc.gt_rgb[3 * p + 1] - e1, d2 = fc.gt_rgb[3 * p + 2] - e2;
    float g0 = gps::l1_sign_grad(d0, fc.inv_count), g1 = gps::l1_sign_grad(d1, fc.inv_count), g2 = gps::l1_sign_grad(d2, fc.inv_count);
    if constexpr (EXPO) {
        gps::exposure_grad_acc(ve, g0, g1, g2, k.c0, k.c1, k.c2);
        gps::exposure_vjp(E, g0, g1, g2, g0, g1, g2);
    }
    float v0, v1, v2, va;
    gps::compose_color_bwd(k, g0, g1, g2, v0, v1, v2, va);
    reinterpret_cast<float4*>(fc.v_render_colors)[p] = make_float4(v0, v1, v2, 0.f);
    fc.v_render_alphas[p] = va;
    // what the strip backward gathers per pixel: {d loss / d weight sum, the depth cut ref_depth + delta_depth}
    if (fc.pix2) reinterpret_cast<float2*>(fc.pix2)[p] = make_float2(va, cut);
    return fabsf(d0) + fabsf(d1) + fabsf(d2);
}

#ifndef GPS_FWD_LIST_SPLIT
#define GPS_FWD_LIST_SPLIT 4
#endif
GPS_TUNABLE_REPORT(GPS_FWD_LIST_SPLIT, 4);
#ifdef GPS_FWD_STAMPS
GPS_SWITCH_REPORT(GPS_FWD_STAMPS);
// probe builds only (tools/probe/fwd_stamps.py): 100 MHz timestamps of workgroup phases, 8 slots per tile (0..6 written; 6, the group lists, between 2 and 3)
__device__ unsigned long long gps_fwd_stamps_buf[4096 * 8];
extern "C" GPS_API void* gps_fwd_stamps() { void* p = nullptr; (void)hipGetSymbolAddress(&p, HIP_SYMBOL(gps_fwd_stamps_buf)); return p; }
#define FWD_STAMP(k) do { if (threadIdx.x == 0) gps_fwd_stamps_buf[blockIdx.x * 8 + (k)] = wall_clock64(); } while (0)
#else
#define FWD_STAMP(k) do { } while (0)
#endif
// A 16 x 16 tile = two 16 x 8 pixel halves (one wave each, 2 px per lane) x FWD_SPLIT list parts: 2 * FWD_SPLIT waves per tile.
// History of the inner loop (bench scene, 1,200 tiles, ~500 k list entries):
//   round 1   every entry evaluated for every pixel                                                   81.6 us
//   round 2   wave-uniform skip in the loop (test e > 8 for all 128 pixels, ballot, branch)             55 us   (list in 4 parts)
//   round 3   cull at staging time, then blend survivors only (below)                                   see LABBOOK.md section 4
// The round-2 loop was bound by its own dependent chain per entry: LDS read -> 10 VALU -> ballot -> branch -> exp -> blend, ~400
// cycles per entry for a lone wave (tools/probe/fwd_stamps.py), with a third of the issue slots used.  Now the staging thread of an
// entry tests the entry's pixel bounds (pack_record: a conservative box around {alpha >= 1/255}; outside it the entry adds exact
// zeros) against the two halves, and the survivors of each half are compacted, in list order, into an index list in LDS.  A
// wave takes an equal share of ITS half's survivors, holds their record addresses in one or two registers (lane j = j-th
// survivor) and walks them with v_readlane: no test, no ballot, no data-dependent branch in the loop, and no LDS reads for the
// ~45 % of a tile's entries that do not reach a given half.  Sums are added in list order inside a part and the parts in order:
// deterministic; a culled entry would have added +0.
//   groups    per-group survivor lists, one DPP broadcast per trip (below)                                see LABBOOK.md section 23
// A wave used to evaluate every survivor of its half on all 128 pixels, while a recorded box averages 12.4 x 10.5 px: most lanes
// of most trips added zeros.  Now each of the wave's four 16-lane DPP rows owns a 32-pixel group of the half.  The staging thread
// tests the box against the 8 groups of the tile; the half's survivors (the OR of its groups: the same S, the same parts) carry
// their four group bits in the survivor word.  A wave ballots each bit over its <= 128 survivors into four wave-private lists
// of record offsets and walks max(list length) trips: every 16 trips a lane loads one entry of its own group's list, and trip
// t hands lane t's entry to the whole row with v_mov_b32 row_newbcast:t -- one VALU instruction where v_readlane was, no scalar
// work added.  A group whose list has run out reads a sentinel record (-log2 opacity = +inf: alpha 0, every sum + 0 * 0).  Part
// boundaries, the order inside a part and the order of the parts are what they were, and no sum can be -0, so the render is bit
// for bit the one of round 3; gps_set_raster_fwd_group_cull(0) gives every survivor all four bits (the old trips in this code).
constexpr int FWD_SPLIT = GPS_FWD_LIST_SPLIT;
constexpr int FWD_THREADS = 128 * FWD_SPLIT;
#ifndef GPS_FWD_BATCH
#define GPS_FWD_BATCH 512
#endif
GPS_TUNABLE_REPORT(GPS_FWD_BATCH, 512);
constexpr int FWD_BATCH = GPS_FWD_BATCH;         // list entries staged per batch (a thread stages FWD_TRIPS of them)
constexpr int FWD_TRIPS = (FWD_BATCH + FWD_THREADS - 1) / FWD_THREADS;
constexpr int FWD_SEGS = FWD_BATCH / 64;         // 64-entry segments of a batch (one ballot each)
constexpr int FWD_VECS = (FWD_BATCH / FWD_SPLIT + 63) / 64;   // registers that hold a part's survivor addresses
static_assert(FWD_BATCH % 64 == 0 && FWD_BATCH * 3 < 2048, "segments are whole waves; a survivor word = 11 bits of record slot + 4 group bits");
// The four 16-lane DPP rows of a wave each own one FWD_GW x FWD_GH pixel group of the wave's 16 x 8 half: 8 x 4 (two groups across,
// two down) or 4 x 8 (four across).  Group g sits at column FWD_GW * (g % FWD_GX), row FWD_GH * (g / FWD_GX) of the half; lane j of
// its row holds pixel pair j % FWD_PW of group row j / FWD_PW.
#ifndef GPS_FWD_GROUP_W
#define GPS_FWD_GROUP_W 8
#endif
GPS_TUNABLE_REPORT(GPS_FWD_GROUP_W, 8);
constexpr int FWD_GW = GPS_FWD_GROUP_W, FWD_GH = 32 / FWD_GW;   // a group's pixels, wide x high
constexpr int FWD_GX = 16 / FWD_GW, FWD_GY = 8 / FWD_GH;        // groups across / down a half
constexpr int FWD_PW = FWD_GW / 2;                              // pixel pairs (lanes) per group row
static_assert(FWD_GW == 8 || FWD_GW == 4, "four groups of 32 pixels per half");
constexpr int FWD_SEQ_STRIDE = FWD_VECS * 64 + 16;             // a group's list of a wave: <= 64 FWD_VECS entries; + 8 dwords: bank skew
// v_mov_b32_dpp row_newbcast:T -- every lane gets the value that lane T of its own 16-lane row holds
template <int T>
__device__ __forceinline__ int fwd_row_bcast(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x150 + T, 0xf, 0xf, true); }   // (every lane is written: no old value)
// the set bits of a ballot below this lane (v_mbcnt_lo / _hi)
__device__ __forceinline__ int fwd_mbcnt(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
// wave_sum over the two compose waves of a tile with the additions paired as when lane 8 r + p held pixel pair p of row r of the
// half: butterfly steps over the lane bits that hold r's bits 2, 1, 0, then p's bits 2, 1, 0.  Keeps the loss and the exposure
// gradient what they were, bit for bit, whichever group shape maps lanes to pixels.
__device__ __forceinline__ float fwd_pixel_sum(float v) {
    constexpr int order8x4[6] = {32, 8, 4, 16, 2, 1}, order4x8[6] = {8, 4, 2, 32, 16, 1};
#pragma unroll
    for (int k = 0; k < 6; k++) v += __shfl_xor(v, FWD_GW == 8 ? order8x4[k] : order4x8[k], 64);
    return v;
}
#define GPS_FWD_PK_NAME raster_ges_fwd_pk_kernel
#define GPS_FWD_PK_EXPOSURE 0
#include "splat_raster_fwd_pk.inc"
#undef GPS_FWD_PK_NAME
#undef GPS_FWD_PK_EXPOSURE
// the train step with a camera that has a row in the exposure table (compose != NULL; fc.pix2 as in the default instance)
#define GPS_FWD_PK_NAME raster_ges_fwd_pk_exposure_kernel
#define GPS_FWD_PK_EXPOSURE 1
#include "splat_raster_fwd_pk.inc"
#undef GPS_FWD_PK_NAME
#undef GPS_FWD_PK_EXPOSURE


__global__ __launch_bounds__(256) void zero_grads_kernel(int N, float* __restrict__ v_means2d,
                                                        float* __restrict__ v_conics, float* __restrict__ v_colors,
                                                        float* __restrict__ v_opacities) {
    const int stride = gridDim.x * blockDim.x;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < 4 * N; k += stride) {
        v_colors[k] = 0.f;
        if (k < 3 * N) v_conics[k] = 0.f;
        if (k < 2 * N) v_means2d[k] = 0.f;
        if (k < N) v_opacities[k] = 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Backward.  One wave64 task = 32 consecutive 32-pixel groups, as two contiguous runs of 16 (one per half-wave).
// Phase A: lanes 0..15 of each half fetch their step's group header and Gaussian record and park them in LDS --
//          ONE global round trip per task instead of one dependent chain per step.
// Phase B: 16 steps; every lane of a half reads its step's record from LDS, evaluates its pixel of the 2r x 2r box and
//          accumulates in registers.  BWD_INFLIGHT steps are evaluated before the first is accumulated; with the straight-line
//          evaluation below ONE step at a time is fastest (68 VGPRs, 7 waves per SIMD: 62.5 us against 65.5 for two steps
//          at 82 VGPRs / 5 waves and 70 for four): other waves cover the gather better than a second step in this one.  A
//          half reduces and writes its 10 sums only when the Gaussian changes.
//
// Per-pixel inputs: three gathers per pixel slot (ref_depth 4 B, v_render_colors 16 B, v_render_alphas 4 B).  Packing them into
// one 32-byte record per pixel (written by the compose kernel; 2 x dwordx4 from one sector) was built and measured SLOWER
// (84 vs 79 us at G = 668 k): the record array is 9.8 MB against 7.3 MB for the three arrays, and what limits the gathers is
// how much of the gradient image each XCD's 4 MB L2 holds, not the number of load instructions.
//
// LDS layout.  Reads are broadcasts (all 32 lanes of a half read one record: conflict free whatever the layout); the bank
// conflicts the counters show (SQ_LDS_BANK_CONFLICT) come from phase A's STORES -- 16 lanes each writing a 64-byte record.
// Records of a half are contiguous (stride 16 dwords: 8-way on a ds_write_b128); interleaving the halves per step (stride 32
// dwords) was measured worse (conflict cycles 3.1e6 -> 7.2e6 per launch), and either way they are < 3 % of the wave cycles.
//
// Flush.  Ten values x 32 lanes -> ten totals.  v_permlane16_swap exchanges the odd rows of one register with the even rows of
// another, so "swap, add" halves the lane span of TWO values at once: five swaps + five adds leave five registers whose two
// 16-lane rows hold one value each; four DPP row_shr adds per register finish the sums (lane 15 of a row); four DPP row_shl
// moves line the ten totals up in ten lanes so that ONE memory instruction writes them: ~45 VALU instead of 85 for ten full
// half-wave DPP reductions.
typedef float bwd_v4 __attribute__((ext_vector_type(4)));

template <int CTRL>
__device__ __forceinline__ float dpp_row_add(float v) {  // v + (v moved by a row-local DPP shift; lanes without a source add 0)
    const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true);
    return v + __int_as_float(moved);
}
__device__ __forceinline__ float row_total_to_lane15(float v) {
    v = dpp_row_add<0x111>(v);  // row_shr:1
    v = dpp_row_add<0x112>(v);  // row_shr:2
    v = dpp_row_add<0x114>(v);  // row_shr:4
    v = dpp_row_add<0x118>(v);  // row_shr:8
    return v;
}
// rows of the result: {a over rows 0+1, b over rows 0+1, a over rows 2+3, b over rows 2+3} -- per half-wave: row 0 = a, row 1 = b
__device__ __forceinline__ float pair_rows(float a, float b) {
    const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(a), __float_as_uint(b), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
// lane 15 of each row -> lane 15 - K of the same row (row_shl:K), merged into `packed` there
template <int K>
__device__ __forceinline__ float place(float packed, float v, int lane16) {
    const int moved = __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x100 + K, 0xF, 0xF, true);
    return lane16 == 15 - K ? __int_as_float(moved) : packed;
}

struct Acc { float c0, c1, c2, c3, ka, kb, kc, mx, my, op; };

// Reduce the half-wave's 10 partial sums and add them to Gaussian g's gradient rows.
//   exclusive = this half-wave saw every pixel group of g (the segment neither touches the start nor the end of the
//   half's 16-group run) and the arrays were zeroed by this launch: a plain store, no read-modify-write at the L2.
//   otherwise: float atomics (another half-wave may hold the rest of g, or the caller accumulates across launches).
__device__ __forceinline__ void flush_acc(Acc& a, int g, int hl, bool exclusive, float* __restrict__ v_means2d,
                                          float* __restrict__ v_conics, float* __restrict__ v_colors,
                                          float* __restrict__ v_opacities) {
    const int lane16 = hl & 15, row = hl >> 4;
    // value index 2 j + row sits in register j: (c0,c1) (c2,c3) (ka,kb) (kc,mx) (my,op)
    float v = row_total_to_lane15(pair_rows(a.c0, a.c1));
    v = place<1>(v, row_total_to_lane15(pair_rows(a.c2, a.c3)), lane16);
    v = place<2>(v, row_total_to_lane15(pair_rows(a.ka, a.kb)), lane16);
    v = place<3>(v, row_total_to_lane15(pair_rows(a.kc, a.mx)), lane16);
    v = place<4>(v, row_total_to_lane15(pair_rows(a.my, a.op)), lane16);
    const int j = 15 - lane16;
    if (g >= 0 && j < 5) {
        const int k = 2 * j + row;  // which total this lane holds
        float* dst = k < 4 ? v_colors + 4 * (size_t)g + k
                   : k < 7 ? v_conics + 3 * (size_t)g + (k - 4)
                   : k < 9 ? v_means2d + 2 * (size_t)g + (k - 7)
                           : v_opacities + g;
        if (exclusive) *dst = v;
        else if (v != 0.f) atomicAdd(dst, v);
    }
    a.c0 = a.c1 = a.c2 = a.c3 = a.ka = a.kb = a.kc = a.mx = a.my = a.op = 0.f;
}

struct __attribute__((aligned(16))) BwdRec {
    float x, y, ca, cb;      // xy, conic a, b
    float cc, opac, r, g;    // conic c, opacity, colour r, g
    float b, depth;          // colour b, depth channel
    int gs_id, pid0;         // Gaussian id (-1 = no group), first pixel slot of the group inside the box
    int x0, y0, bw;          // x_min + 1, y_min + 1, box width 2r (y_max = y0 + bw - 1)
    float inv_bw;            // 1 / bw: (pid + 0.5) * inv_bw truncates to pid / bw exactly for pid < 2^16
};

#ifndef GPS_BWD_INFLIGHT
#define GPS_BWD_INFLIGHT 1
#endif
GPS_TUNABLE_REPORT(GPS_BWD_INFLIGHT, 1);
constexpr int BWD_INFLIGHT = GPS_BWD_INFLIGHT;
struct BwdPix { bool on; float alpha, vis, dx, dy, cut; float4 vc; float va; };

struct BwdPixArgs {  // kernel arguments
    const float* ref_depth;
    const float4* v_render_colors;
    const float* v_render_alphas;
    float delta_depth;
};
struct BwdPixSrc {  // the three per-pixel arrays as buffer resources (W * H elements each)
    __amdgpu_buffer_rsrc_t ref_depth, v_render_colors, v_render_alphas;
    float delta_depth;
};
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pixel_buffer(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, 0x00020000);  // raw dword buffer, stride 0
}

// Straight-line on purpose.  With the gathers under the alpha-test branch and their use under bwd_accum's branch, the
// compiler cannot tell at the loop's back edge whether a gather is still pending and guards the next step's address
// registers with s_waitcnt vmcnt(0) -- which (vmcnt counts in order) also waits for the gathers the previous step has just
// issued: one full memory round trip per step, SQ_WAIT_ANY 55 %.  Here every lane always loads (slots that fail the test
// read pixel 0: one extra address per wave), and bwd_landed() makes the arrival of a step's three values an unconditional
// point of the loop, so two steps' gathers are really in flight together.
__device__ __forceinline__ void bwd_eval(const BwdRec& R, int hl, int W, int H, const BwdPixSrc& src, BwdPix& o) {
    const uint32_t pid = (uint32_t)R.pid0 + (uint32_t)hl;
    const int q = (int)(((float)pid + 0.5f) * R.inv_bw);  // pid / bw
    const int j = R.x0 + ((int)pid - q * R.bw);
    const int i = R.y0 + q;
    const bool inside = (R.gs_id >= 0) && (i < H) && (j < W) && (i >= 0) && (j >= 0) && (q < R.bw);
    const float px = (float)j + 0.5f, py = (float)i + 0.5f;
    o.dx = R.x - px; o.dy = R.y - py;
    const float sigma = 0.5f * (R.ca * o.dx * o.dx + R.cc * o.dy * o.dy) + R.cb * o.dx * o.dy;
    o.vis = __expf(-sigma);
    o.alpha = fminf(0.999f, R.opac * o.vis);
    // the {alpha >= 1/255} ellipse fills 45 % of the 2r x 2r box the groups enumerate (tools/raster_bench.py)
    o.on = inside && !((sigma < 0.f) || (o.alpha < 1.f / 255.f));
    // raw buffer loads: a 32-bit byte offset per lane instead of three 64-bit addresses, and a slot that fails the test
    // passes an out-of-range offset -- the load returns 0 without touching memory
    const uint32_t pix = o.on ? (uint32_t)(i * W + j) : 0x0FFFFFFFu;
    o.cut = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(src.ref_depth, pix * 4u, 0, 0));  // (tested in bwd_accum)
    o.vc = __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(src.v_render_colors, pix * 16u, 0, 0));
    o.va = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(src.v_render_alphas, pix * 4u, 0, 0));
}

__device__ __forceinline__ void bwd_landed(BwdPix& p) {
    asm volatile("" : "+v"(p.cut), "+v"(p.va), "+v"(p.vc.x), "+v"(p.vc.y), "+v"(p.vc.z), "+v"(p.vc.w));
}

__device__ __forceinline__ void bwd_accum(const BwdRec& R, const BwdPix& p, float delta_depth, Acc& acc) {
    if (!p.on || R.depth > p.cut + delta_depth) return;
    acc.c0 += p.alpha * p.vc.x; acc.c1 += p.alpha * p.vc.y; acc.c2 += p.alpha * p.vc.z; acc.c3 += p.alpha * p.vc.w;
    const float v_alpha = R.r * p.vc.x + R.g * p.vc.y + R.b * p.vc.z + R.depth * p.vc.w + p.va;
    if (R.opac * p.vis <= 0.999f) {
        const float v_sigma = -R.opac * p.vis * v_alpha;
        acc.ka += 0.5f * v_sigma * p.dx * p.dx;
        acc.kb += v_sigma * p.dx * p.dy;
        acc.kc += 0.5f * v_sigma * p.dy * p.dy;
        acc.mx += v_sigma * (R.ca * p.dx + R.cb * p.dy);
        acc.my += v_sigma * (R.cb * p.dx + R.cc * p.dy);
        acc.op += p.vis * v_alpha;
    }
}

__global__ __launch_bounds__(256) void raster_ges_bwd_gs_kernel(
    const int32_t* __restrict__ group_gs_ids, const int32_t* __restrict__ group_starts,
    const float2* __restrict__ means2d, const float* __restrict__ conics, const float4* __restrict__ colors,
    const float* __restrict__ opacities, const int32_t* __restrict__ radiis, BwdPixArgs pix_args,
    const int64_t* __restrict__ counts, int W, int H, float* __restrict__ v_means2d, float* __restrict__ v_conics,
    float* __restrict__ v_colors, float* __restrict__ v_opacities, int plain_ok) {
    __shared__ BwdRec recs[4][2][16];  // [wave][half][step]
    const uint32_t n_px = (uint32_t)(W * H);
    const BwdPixSrc src = {pixel_buffer(pix_args.ref_depth, n_px * 4u), pixel_buffer(pix_args.v_render_colors, n_px * 16u),
                           pixel_buffer(pix_args.v_render_alphas, n_px * 4u), pix_args.delta_depth};
    const int n_groups = (int)counts[1];
    const int n_tasks = (n_groups + 31) >> 5;
    const int lane = threadIdx.x & 63, wave_in_wg = threadIdx.x >> 6;
    const int half = lane >> 5, hl = lane & 31;
    // Workgroups are dealt to the 8 XCDs round-robin (blockIdx % 8); give each XCD ONE contiguous eighth of the task
    // list instead of a stride-8 comb through all of it: Gaussians with neighbouring ids cover neighbouring pixels, so
    // an XCD then gathers from one band of the gradient image, which its 4 MB L2 can hold.
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, wgs_per_xcd = gridDim.x >> 3;   // gridDim.x % 8 == 0
    const int per_xcd = (n_tasks + 7) >> 3;
    const int xcd_lo = xcd * per_xcd, xcd_hi = min(n_tasks, xcd_lo + per_xcd);
    const int wave_in_xcd = slot * 4 + wave_in_wg, waves_per_xcd = wgs_per_xcd * 4;
    BwdRec* my = recs[wave_in_wg][half];

    for (int task = xcd_lo + wave_in_xcd; task < xcd_hi; task += waves_per_xcd) {
        // ---- phase A: one record per step, fetched by lanes 0..15 of each half
        if (hl < 16) {
            const int gid = task * 32 + half * 16 + hl;
            BwdRec R;
            R.gs_id = -1;
            if (gid < n_groups) {
                const int g = group_gs_ids[gid];
                const int gstart = group_starts[gid];
                const float2 xy = means2d[g];
                const float4 c = colors[g];
                const int r = radiis[g];
                R.x = xy.x; R.y = xy.y;
                R.ca = conics[3 * g]; R.cb = conics[3 * g + 1]; R.cc = conics[3 * g + 2];
                R.opac = opacities[g];
                R.r = c.x; R.g = c.y; R.b = c.z; R.depth = c.w;
                R.gs_id = g;
                R.pid0 = (gid - gstart) * 32;
                R.x0 = (int)xy.x - r + 1; R.y0 = (int)xy.y - r + 1; R.bw = 2 * r; R.inv_bw = 1.0f / (float)(2 * r);
            }
            my[hl] = R;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        // ---- phase B
        Acc acc;
        acc.c0 = acc.c1 = acc.c2 = acc.c3 = acc.ka = acc.kb = acc.kc = acc.mx = acc.my = acc.op = 0.f;
        int cur_g = -1;
        bool first_seg = true;  // the current segment began at step 0 of the run (it may continue a neighbour's)
        for (int s = 0; s < 16; s += BWD_INFLIGHT) {
            BwdPix p[BWD_INFLIGHT];
#pragma unroll
            for (int u = 0; u < BWD_INFLIGHT; ++u) bwd_eval(my[s + u], hl, W, H, src, p[u]);
#pragma unroll
            for (int u = 0; u < BWD_INFLIGHT; ++u) {
                const BwdRec R = my[s + u];
                if (R.gs_id != cur_g) {
                    // the segment that ends here started after step 0 and ends before the run does
                    if (cur_g >= 0)
                        flush_acc(acc, cur_g, hl, plain_ok && !first_seg, v_means2d, v_conics, v_colors, v_opacities);
                    first_seg = cur_g < 0;  // still no Gaussian seen (cannot happen after a real segment)
                    cur_g = R.gs_id;
                }
                bwd_landed(p[u]);
                bwd_accum(R, p[u], src.delta_depth, acc);
            }
        }
        if (cur_g >= 0) flush_acc(acc, cur_g, hl, false, v_means2d, v_conics, v_colors, v_opacities);
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace

// gps_set_raster_fwd_group_cull: 1 (default) -> a pixel group of the record forward walks only the entries whose box touches it;
// 0 -> every group walks its half's whole list (the trip structure before the group lists, in the same code: A/B and test lever)
static int g_raster_fwd_group_cull = 1;

namespace gps {

int raster_ges_fwd_rec_launch(int N, const float* records, const float* ref_depth_map, int width, int height,
                              const int32_t* tile_offsets, const int32_t* flatten_ids, const int64_t* counts, float delta_depth,
                              float* render_colors, float* render_alphas, const FwdCompose* compose, gps_stream stream,
                              const int32_t* tile_order, const FwdExposure* exposure) {
    GPS_ENTER();
    GPS_REQUIRE(N >= 0 && width > 0 && height > 0);
    GPS_REQUIRE(ref_depth_map && tile_offsets && flatten_ids && counts && render_colors && render_alphas);
    GPS_REQUIRE(N == 0 || records);
    FwdCompose fc = {};
    if (compose) {
        fc = *compose;
        GPS_REQUIRE(fc.base_color && fc.gt_rgb && fc.rgb && fc.loss && fc.v_render_colors && fc.v_render_alphas);
    }
    const int tw = gps_div_up(width, 16), th = gps_div_up(height, 16);
    // (experiment, gps_set_frame_chain_reserve bit 1: 14 KB of unused dynamic LDS on top of the 26.7 KB the kernel declares -> 3
    // workgroups of 8 waves per compute unit instead of the 4 that fill every wave slot)
    const size_t pad = (gps::frame_chain_reserve_bits() & 2) ? 14 * 1024 : 0;
    const int group_cull = __atomic_load_n(&g_raster_fwd_group_cull, __ATOMIC_RELAXED);
    if (exposure) {
        GPS_REQUIRE(compose && exposure->row && exposure->slab);
        launch_kernel(TK_RASTER_FWD, 1, raster_ges_fwd_pk_exposure_kernel, dim3(tw * th), dim3(FWD_THREADS), pad, (hipStream_t)stream,
                      (const float4*)records, ref_depth_map, width, height, tw, th, tile_offsets, flatten_ids, counts, delta_depth,
                      (float4*)render_colors, render_alphas, fc, *exposure, tile_order, group_cull);
    } else {
        launch_kernel(TK_RASTER_FWD, compose ? 1 : 0, raster_ges_fwd_pk_kernel, dim3(tw * th), dim3(FWD_THREADS), pad, (hipStream_t)stream,
                      (const float4*)records, ref_depth_map, width, height, tw, th, tile_offsets, flatten_ids, counts, delta_depth,
                      (float4*)render_colors, render_alphas, fc, tile_order, group_cull);
    }
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int raster_ges_bwd_gs_launch(int N, const float* means2d, const float* conics, const float* colors, const float* opacities,
                             const int32_t* radii, const float* ref_depth_map, int width, int height,
                             const int32_t* group_gs_ids, const int32_t* group_starts, const int64_t* counts, float delta_depth,
                             const float* v_render_colors, const float* v_render_alphas, float* v_means2d, float* v_conics,
                             float* v_colors, float* v_opacities, int zero_mode, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(N >= 0 && width > 0 && height > 0);
    if (N == 0) return GPS_OK;
    GPS_REQUIRE(means2d && conics && colors && opacities && radii && ref_depth_map && group_gs_ids && group_starts &&
                counts && v_render_colors && v_render_alphas && v_means2d && v_conics && v_colors && v_opacities);
    hipStream_t s = (hipStream_t)stream;
    if (zero_mode == 0)
        zero_grads_kernel<<<min(2048, gps_div_up(4 * (int64_t)N, 256)), 256, 0, s>>>(N, v_means2d, v_conics, v_colors,
                                                                                     v_opacities);
#ifndef GPS_BWD_BLOCKS
#define GPS_BWD_BLOCKS 4096
#endif
    constexpr int bwd_blocks = GPS_BWD_BLOCKS;  // multiple of 8 (one contiguous task range per XCD), 16 workgroups per CU
    BwdPixArgs src = {ref_depth_map, (const float4*)v_render_colors, v_render_alphas, delta_depth};
    // plain stores where a half-wave owns a Gaussian: only if the buffers are known to be zero (filled here or by the caller)
    raster_ges_bwd_gs_kernel<<<bwd_blocks, 256, 0, s>>>(group_gs_ids, group_starts, (const float2*)means2d, conics,
                                                        (const float4*)colors, opacities, radii, src, counts, width, height,
                                                        v_means2d, v_conics, v_colors, v_opacities, zero_mode == 1 ? 0 : 1);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

}  // namespace gps

extern "C" {

void gps_set_raster_fwd_group_cull(int on) { __atomic_store_n(&g_raster_fwd_group_cull, on ? 1 : 0, __ATOMIC_RELAXED); }

int gps_raster_ges_fwd(int N, const float* means2d, const float* conics, const float* colors, const float* opacities,
                       const float* ref_depth_map, int width, int height, int tile_size, const int32_t* tile_offsets,
                       const int32_t* flatten_ids, const int64_t* counts, float delta_depth, float* render_colors,
                       float* render_alphas, int32_t* last_ids, gps_stream stream) {
    GPS_ENTER();
    GPS_REQUIRE(N >= 0 && width > 0 && height > 0);
    GPS_REQUIRE(tile_size == 16);  // every shipped config uses 16 (raw_gs_model.h); other sizes are rejected loudly
    GPS_REQUIRE(ref_depth_map && tile_offsets && flatten_ids && counts && render_colors && render_alphas);
    GPS_REQUIRE(N == 0 || (means2d && conics && colors && opacities));
    const int tw = gps_div_up(width, tile_size), th = gps_div_up(height, tile_size);
    raster_ges_fwd_kernel<16><<<tw * th, TILE_THREADS, 0, (hipStream_t)stream>>>(
        (const float2*)means2d, conics, (const float4*)colors, opacities, ref_depth_map, width, height, tw, th,
        tile_offsets, flatten_ids, counts, delta_depth, (float4*)render_colors, render_alphas, last_ids);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int gps_raster_ges_fwd_rec(int N, const float* records, const float* ref_depth_map, int width, int height,
                           const int32_t* tile_offsets, const int32_t* flatten_ids, const int64_t* counts,
                           float delta_depth, float* render_colors, float* render_alphas, gps_stream stream) {
    return gps::raster_ges_fwd_rec_launch(N, records, ref_depth_map, width, height, tile_offsets, flatten_ids, counts,
                                          delta_depth, render_colors, render_alphas, nullptr, stream);
}

int gps_raster_ges_fwd_rec_ordered(int N, const float* records, const float* ref_depth_map, int width, int height,
                                   const int32_t* tile_offsets, const int32_t* flatten_ids, const int64_t* counts,
                                   float delta_depth, float* render_colors, float* render_alphas, const int32_t* tile_order,
                                   gps_stream stream) {
    return gps::raster_ges_fwd_rec_launch(N, records, ref_depth_map, width, height, tile_offsets, flatten_ids, counts,
                                          delta_depth, render_colors, render_alphas, nullptr, stream, tile_order);
}

int gps_raster_ges_bwd_gs(int N, const float* means2d, const float* conics, const float* colors,
                          const float* opacities, const int32_t* radii, const float* ref_depth_map, int width,
                          int height, const int32_t* group_gs_ids, const int32_t* group_starts, const int64_t* counts,
                          float delta_depth, const float* v_render_colors, const float* v_render_alphas,
                          float* v_means2d, float* v_conics, float* v_colors, float* v_opacities, int accumulate,
                          gps_stream stream) {
    return gps::raster_ges_bwd_gs_launch(N, means2d, conics, colors, opacities, radii, ref_depth_map, width, height,
                                         group_gs_ids, group_starts, counts, delta_depth, v_render_colors, v_render_alphas,
                                         v_means2d, v_conics, v_colors, v_opacities, accumulate ? 1 : 0, stream);
}

}  // extern "C"

// build-time tunables defined inside functions above (gps_build_flags)
GPS_TUNABLE_REPORT(GPS_BWD_BLOCKS, 4096);
