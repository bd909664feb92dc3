// The record forward's per-tile kernel (splat_raster.hip), included twice: GPS_FWD_PK_EXPOSURE 0 -> raster_ges_fwd_pk_kernel, the
// default instance; 1 -> raster_ges_fwd_pk_exposure_kernel, whose compose epilogue applies the camera's exposure row and writes the
// tile's d loss / d E into ex.slab (per-frame exposure, use_exposure).  A preprocessor instance rather than a template, so that the
// default kernel is the same code, instruction for instruction, as before the exposure instance existed.
__global__ __launch_bounds__(FWD_THREADS) __attribute__((amdgpu_num_sgpr(96))) void GPS_FWD_PK_NAME(
    const float4* __restrict__ recs, const float* __restrict__ ref_depth, int W, int H, int tw, int th,
    const int32_t* __restrict__ tile_offsets, const int32_t* __restrict__ flatten_ids,
    const int64_t* __restrict__ counts, float delta_depth, float4* __restrict__ render_colors,
    float* __restrict__ render_alphas, gps::FwdCompose fc,
#if GPS_FWD_PK_EXPOSURE
    gps::FwdExposure ex,
#endif
    const int32_t* __restrict__ tile_order, int group_cull, gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    // 48-byte records {mx, my, 0.5*ca*log2e, cb*log2e | 0.5*cc*log2e, -log2(opac), depth, r | g, b, -, -}; after the last batch the
    // same memory carries the parts' partial sums; behind the records, in a slot of its own, the sentinel record (below)
    constexpr int PART_FLOATS = (FWD_SPLIT - 1) * 128 * 10;
    constexpr int REC_FLOATS = FWD_BATCH * 12;
    static_assert(PART_FLOATS <= REC_FLOATS, "the sentinel stays clear of the partial sums");
    __shared__ float4 lds_rec[REC_FLOATS / 4 + 3];
    // per pixel half: the batch's surviving entries in list order, bits 0-10 the record's byte offset / 16, bits 11-14 the groups
    // of the half that the entry's box touches
    __shared__ uint16_t sidx[2][FWD_BATCH];
    __shared__ int scnt[2][FWD_SEGS];          // survivors per staging wave
    // per wave and group: the byte offsets of the records this group evaluates, list order (the row stride keeps the four rows of a
    // chunk read on different banks)
    __shared__ uint16_t seq[2 * FWD_SPLIT][4][FWD_SEQ_STRIDE];
    FWD_STAMP(0);
    const int tile_id = tile_order ? tile_order[blockIdx.x] : (int)blockIdx.x;   // (longest lists first when the binning provides the order)
    const int ty = tile_id / tw, tx = tile_id - ty * tw;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: loop bounds below)
    const int list_part = wave >> 1, pix_half = wave & 1;
    // a DPP row of 16 lanes = one FWD_GW x FWD_GH pixel group of the half, a lane = two horizontally adjacent pixels of it
    const int grp = lane >> 4, gl = lane & 15;
    const int row = ty * 16 + pix_half * 8 + FWD_GH * (grp / FWD_GX) + gl / FWD_PW;
    const int col = tx * 16 + FWD_GW * (grp % FWD_GX) + 2 * (gl % FWD_PW);
    const bool in0 = (row < H) && (col < W), in1 = (row < H) && (col + 1 < W);
    const v2f px = {(float)col + 0.5f, (float)col + 1.5f};
    const float py = (float)row + 0.5f;
    const float cut0 = in0 ? ref_depth[row * W + col] + delta_depth : -3.0e38f;
    const float cut1 = in1 ? ref_depth[row * W + col + 1] + delta_depth : -3.0e38f;
    v2f o0 = {0.f, 0.f}, o1 = o0, o2 = o0, o3 = o0, ws = o0;
    const int n_isects = (int)counts[0];
    const int range_start = tile_offsets[tile_id];
    const int range_end = (tile_id == tw * th - 1) ? n_isects : tile_offsets[tile_id + 1];
    constexpr float LOG2E = 1.4426950408889634f;
    // the sentinel: what a group reads once its own list has run out.  exp2(-inf) = 0 and the alpha test fails, so every sum gets + 0 * 0
    constexpr int SENTINEL = 16 * 3 * FWD_BATCH;
    if (tid == 0) {
        lds_rec[3 * FWD_BATCH] = make_float4(0.f, 0.f, 0.f, 0.f);
        lds_rec[3 * FWD_BATCH + 1] = make_float4(0.f, __builtin_inff(), 0.f, 0.f);
        lds_rec[3 * FWD_BATCH + 2] = make_float4(0.f, 0.f, 0.f, 0.f);
    }

    for (int batch_start = range_start; batch_start < range_end; batch_start += FWD_BATCH) {
        __syncthreads();   // the previous batch's records and lists are consumed
        int h0[FWD_TRIPS], h1[FWD_TRIPS];   // the groups of half 0 / 1 that the entry's box touches (0: no survivor of that half)
        int r0[FWD_TRIPS], r1[FWD_TRIPS];   // rank among the segment's survivors
#pragma unroll
        for (int u = 0; u < FWD_TRIPS; u++) {
            const int k = u * FWD_THREADS + tid;   // slot in the batch; segment k >> 6 = u * (FWD_THREADS / 64) + wave
            const int idx = batch_start + k;
            h0[u] = 0; h1[u] = 0;
            if (k < FWD_BATCH && idx < range_end) {
                const size_t g = (size_t)flatten_ids[idx];
                const float4 a = recs[3 * g], b = recs[3 * g + 1], c = recs[3 * g + 2];
                lds_rec[3 * k] = make_float4(a.x, a.y, 0.5f * LOG2E * a.z, LOG2E * a.w);
                lds_rec[3 * k + 1] = make_float4(0.5f * LOG2E * b.x, -__log2f(b.y), b.z, b.w);
                lds_rec[3 * k + 2] = make_float4(c.x, c.y, 0.f, 0.f);
                const int xb = __float_as_int(c.z), yb = __float_as_int(c.w);
                const int x_lo = (int)(short)(xb & 0xffff), x_hi = xb >> 16, y_lo = (int)(short)(yb & 0xffff), y_hi = yb >> 16;
                // the box against the tile's columns of groups and rows of groups; a half's survivors are the entries that touch
                // one of its groups, which is the box against the half
                int xm = 0, ym = 0;
                if (x_lo <= x_hi && y_lo <= y_hi) {
#pragma unroll
                    for (int c = 0; c < FWD_GX; c++)
                        if (x_lo <= tx * 16 + FWD_GW * c + FWD_GW - 1 && x_hi >= tx * 16 + FWD_GW * c) xm |= 1 << c;
#pragma unroll
                    for (int r = 0; r < 2 * FWD_GY; r++)
                        if (y_lo <= ty * 16 + FWD_GH * r + FWD_GH - 1 && y_hi >= ty * 16 + FWD_GH * r) ym |= 1 << r;
                }
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    if (((xm >> (g % FWD_GX)) & 1) && ((ym >> (g / FWD_GX)) & 1)) h0[u] |= 1 << g;
                    if (((xm >> (g % FWD_GX)) & 1) && ((ym >> (FWD_GY + g / FWD_GX)) & 1)) h1[u] |= 1 << g;
                }
                if (!group_cull) { h0[u] = h0[u] ? 15 : 0; h1[u] = h1[u] ? 15 : 0; }   // (every group walks the half's whole list)
            }
            const unsigned long long m0 = __ballot(h0[u] != 0), m1 = __ballot(h1[u] != 0);
            r0[u] = fwd_mbcnt(m0); r1[u] = fwd_mbcnt(m1);
            const int seg = u * (FWD_THREADS / 64) + wave;
            if (lane == 0 && seg < FWD_SEGS) { scnt[0][seg] = __popcll(m0); scnt[1][seg] = __popcll(m1); }
        }
        FWD_STAMP(1);
        __syncthreads();
        // exclusive prefix of the segments' survivor counts, per half (wave-uniform values); S = all survivors of the half this
        // wave will EVALUATE
        int pre0[FWD_SEGS + 1], pre1[FWD_SEGS + 1];
        pre0[0] = 0; pre1[0] = 0;
#pragma unroll
        for (int w = 0; w < FWD_SEGS; w++) { pre0[w + 1] = pre0[w] + scnt[0][w]; pre1[w + 1] = pre1[w] + scnt[1][w]; }
        int S = pix_half ? pre1[FWD_SEGS] : pre0[FWD_SEGS];
#pragma unroll
        for (int u = 0; u < FWD_TRIPS; u++) {
            const int k = u * FWD_THREADS + tid;
            int b0 = 0, b1 = 0;
#pragma unroll
            for (int w = 0; w < FWD_SEGS; w++)   // (the segment index is wave-uniform: a scalar select)
                if (w == u * (FWD_THREADS / 64) + wave) { b0 = pre0[w]; b1 = pre1[w]; }
            if (h0[u]) sidx[0][b0 + r0[u]] = (uint16_t)(3 * k | h0[u] << 11);
            if (h1[u]) sidx[1][b1 + r1[u]] = (uint16_t)(3 * k | h1[u] << 11);
        }
        __syncthreads();
        FWD_STAMP(2);
        S = __builtin_amdgcn_readfirstlane(S);
        const int lo = list_part * S / FWD_SPLIT, cnt = (list_part + 1) * S / FWD_SPLIT - lo;   // this wave's survivors
        // the wave's survivors, split by group: ballot each group bit and rank with mbcnt -> seq[wave][g] holds, in list order, the
        // record byte offsets of the entries whose box touches group g; ng[g] of them (scalars).  The lists are the wave's own: a
        // wave-level fence orders its writes before its reads, no workgroup barrier
        uint16_t* sq = &seq[wave][0][0];
        int ng[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < FWD_VECS; k++) {
            if (64 * k < cnt) {   // wave-uniform
                const int word = (64 * k + lane < cnt) ? (int)sidx[pix_half][lo + 64 * k + lane] : 0;
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const bool f = (word >> (11 + g)) & 1;
                    const unsigned long long m = __ballot(f);
                    if (f) sq[g * FWD_SEQ_STRIDE + ng[g] + fwd_mbcnt(m)] = (uint16_t)(16 * (word & 0x7ff));
                    ng[g] += __popcll(m);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        FWD_STAMP(6);
        const int T = max(max(ng[0], ng[1]), max(ng[2], ng[3]));            // trips: the longest group list
        const int my_n = grp == 0 ? ng[0] : grp == 1 ? ng[1] : grp == 2 ? ng[2] : ng[3];
        const char* rec_bytes = reinterpret_cast<const char*>(lds_rec);
        auto blend = [&](int byte_off) {
            const float4 a = *reinterpret_cast<const float4*>(rec_bytes + byte_off);
            const float4 b = *reinterpret_cast<const float4*>(rec_bytes + byte_off + 16);
            const float2 c = *reinterpret_cast<const float2*>(rec_bytes + byte_off + 32);
            const float dy = a.y - py;
            const v2f dx = a.x - px;
            const float cdy2 = b.x * dy * dy, bdy = a.w * dy;
            const v2f w = a.z * dx + bdy;
            const v2f sig = w * dx + cdy2;        // sigma * log2(e)
            const v2f e = sig + b.y;              // sigma' - log2(opacity)
            float al0 = fminf(0.999f, __builtin_amdgcn_exp2f(-e.x));
            float al1 = fminf(0.999f, __builtin_amdgcn_exp2f(-e.y));
            const bool hit0 = !(b.z > cut0) && !(sig.x < 0.f) && !(al0 < 1.f / 255.f);
            const bool hit1 = !(b.z > cut1) && !(sig.y < 0.f) && !(al1 < 1.f / 255.f);
            const v2f al = {hit0 ? al0 : 0.f, hit1 ? al1 : 0.f};
            o0 += b.w * al; o1 += c.x * al; o2 += c.y * al; o3 += b.z * al; ws += al;
        };
        // 16 trips per chunk: lane j of row g loads entry 16 c + j of its group's list (the sentinel past the list's end), trip t
        // broadcasts lane t's value inside each row (v_mov_b32 row_newbcast:t) as the record's LDS address.  Two entries per trip:
        // their records leave LDS together; an odd T ends on a trip whose second entry is the sentinel in every group
        for (int c = 0; 16 * c < T; c++) {
            const int e = 16 * c + gl;
            const int mine = (int)sq[grp * FWD_SEQ_STRIDE + e];
            const int off = e < my_n ? mine : SENTINEL;
            const int n = T - 16 * c;   // wave-uniform
#define FWD_TRIP_PAIR(t) if ((t) < n) { const int t0 = fwd_row_bcast<(t)>(off), t1 = fwd_row_bcast<(t) + 1>(off); blend(t0); blend(t1); }
            FWD_TRIP_PAIR(0) FWD_TRIP_PAIR(2) FWD_TRIP_PAIR(4) FWD_TRIP_PAIR(6)
            FWD_TRIP_PAIR(8) FWD_TRIP_PAIR(10) FWD_TRIP_PAIR(12) FWD_TRIP_PAIR(14)
#undef FWD_TRIP_PAIR
        }
    }
    // list parts 1.. -> LDS (over the records) -> part 0 adds them in order and stores
    FWD_STAMP(3);
    __syncthreads();   // every wave is done with the records
    float* part = reinterpret_cast<float*>(lds_rec);
    const int slot = (pix_half * 64 + lane) * 10;
    if (list_part) {
        float* q = part + (list_part - 1) * 1280 + slot;
        q[0] = o0.x; q[1] = o1.x; q[2] = o2.x; q[3] = o3.x; q[4] = ws.x;
        q[5] = o0.y; q[6] = o1.y; q[7] = o2.y; q[8] = o3.y; q[9] = ws.y;
    }
    __syncthreads();
    FWD_STAMP(4);
#if GPS_FWD_PK_EXPOSURE
    float ve[12];   // this lane's d loss / d E
#pragma unroll
    for (int k = 0; k < 12; k++) ve[k] = 0.f;
#endif
    float lsum = 0.f;   // compose waves: the wave's sum of |gt - rgb|
    if (!list_part) {
        const int pix = row * W + col;
#pragma unroll
        for (int k = 0; k < FWD_SPLIT - 1; k++) {
            const float* q = part + k * 1280 + slot;
            o0.x += q[0]; o1.x += q[1]; o2.x += q[2]; o3.x += q[3]; ws.x += q[4];
            o0.y += q[5]; o1.y += q[6]; o2.y += q[7]; o3.y += q[8]; ws.y += q[9];
        }
        const float4 c0 = make_float4(o0.x, o1.x, o2.x, o3.x);
        const float4 c1 = make_float4(o0.y, o1.y, o2.y, o3.y);
        const float w0 = ws.x, w1 = ws.y;
        if (in0) { render_colors[pix] = c0; render_alphas[pix] = w0; }
        if (in1) { render_colors[pix + 1] = c1; render_alphas[pix + 1] = w1; }
        if (fc.base_color) {
            // compose + L1 + image gradients of the two pixels
#if GPS_FWD_PK_EXPOSURE
            float E[12];
            gps::exposure_load(ex.row, E);
            if (in0) lsum += compose_l1_pixel<true>(fc, E, ve, pix, c0, w0, cut0);
            if (in1) lsum += compose_l1_pixel<true>(fc, E, ve, pix + 1, c1, w1, cut1);
#else
            float none[1];
            if (in0) lsum += compose_l1_pixel<false>(fc, none, none, pix, c0, w0, cut0);
            if (in1) lsum += compose_l1_pixel<false>(fc, none, none, pix + 1, c1, w1, cut1);
#endif
            lsum = fwd_pixel_sum(lsum);
        }
    }
    // the tile's share of the loss: wave 1 -> LDS -> wave 0 adds and issues ONE atomicAdd per tile.  Every one of them goes to the
    // same word and the memory side takes them one after the other (about 21 ns each, measured): with one per compose wave, 2,400 a
    // launch at 640x480, the launch could not end before ~50 us whatever the waves did (LABBOOK.md section 23)
    if (fc.base_color) {
        float* tile_loss = reinterpret_cast<float*>(&scnt[0][0]);   // (free since the last batch's prefix)
        if (wave == 1 && lane == 0) *tile_loss = lsum;
        __syncthreads();
        if (wave == 0 && lane == 0) atomicAdd(fc.loss, (lsum + *tile_loss) * fc.inv_count);
    }
#if GPS_FWD_PK_EXPOSURE
    // the tile's d loss / d E: butterfly sums inside the two compose waves, then wave 1 -> LDS -> wave 0 adds and stores the tile's
    // row of the slab (fixed order, no atomics: bit-reproducible)
    if (!list_part) {
#pragma unroll
        for (int k = 0; k < 12; k++) ve[k] = fwd_pixel_sum(ve[k]);
    }
    __syncthreads();   // part 0 is done reading the partial sums out of LDS
    if (wave == 1 && lane == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) part[k] = ve[k];
    }
    __syncthreads();
    if (wave == 0 && lane == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) ex.slab[(size_t)tile_id * 12 + k] = ve[k] + part[k];
    }
#endif
    FWD_STAMP(5);
}
