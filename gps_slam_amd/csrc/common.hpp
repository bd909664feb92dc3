// Shared host/device helpers for the gfx950 kernels (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <time.h>

#include "../../include/gps_slam_hip.h"

#define GPS_WAVE 64

// Every C-ABI entry point returns GPS_OK or a negative error; launches are checked
// with hipGetLastError so a bad configuration is reported, never silently skipped.
#define GPS_LAUNCH_CHECK()                                   \
    do {                                                     \
        hipError_t e__ = hipGetLastError();                  \
        if (e__ != hipSuccess) {                             \
            fprintf(stderr, "[gps_slam_hip] %s:%d launch failed: %s\n", __FILE__, __LINE__, hipGetErrorString(e__)); \
            return GPS_ERR_LAUNCH;                           \
        }                                                    \
    } while (0)

// hipGetLastError() is per-thread and shared with every other HIP user in the process (e.g. torch);
// clear whatever was left behind so GPS_LAUNCH_CHECK only reports our own launches.
#define GPS_ENTER() (void)hipGetLastError()

#define GPS_REQUIRE(cond)                 \
    do {                                  \
        if (!(cond)) return GPS_ERR_ARG;  \
    } while (0)

static inline int gps_div_up(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// ---- build-time probe switches (gps_build_flags) ----
// The kernels keep a few compile-time tunables (-DGPS_...=n) for A/B builds (tools/probe/variant.py).  Every translation unit
// reports the ones it was compiled with: a tunable whose value differs from the shipped default, or a defined probe switch,
// lands in the string gps_build_flags() returns.  The shipped library reports "" -- tests/test_abi_cpu.py and
// __graft_entry__.smoke() assert it.
namespace gps {
void report_build_flag(const char* name, long value);   // splat_project.hip
struct BuildFlag {
    BuildFlag(const char* name, long value, long shipped) { if (value != shipped) report_build_flag(name, value); }
};
}  // namespace gps
#define GPS_TUNABLE_REPORT(name, shipped) static const gps::BuildFlag gps_build_flag_##name(#name, (long)(name), (long)(shipped))
#define GPS_SWITCH_REPORT(name) static const gps::BuildFlag gps_build_flag_##name(#name, 1L, 0L)

// ---- wave64 reductions (DPP-free, shuffle based; all 64 lanes active) ----
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ unsigned long long lanemask_lt() {
    return (1ull << (threadIdx.x & 63)) - 1ull;
}

// ---- integer prefix sums (exact in any association; every thread of the wave / workgroup takes part) ----
// inclusive scan across the 64 lanes of a wave
__device__ __forceinline__ int wave_incl_scan_i(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        int t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
// exclusive scan across the wave, the sum of all 64 lanes to `total`
__device__ __forceinline__ int wave_excl_scan_i(int v, int& total) {
    const int incl = wave_incl_scan_i(v);
    total = __shfl(incl, 63, 64);
    return incl - v;
}
// exclusive scan of one int per thread over the NT threads of the workgroup (a multiple of 64, <= 1024), their sum to `total`;
// ws: NT / 64 + 1 ints of LDS, free again on return
template <int NT>
__device__ __forceinline__ int block_excl_scan(int v, int* ws, int& total) {
    static_assert(NT % 64 == 0 && NT <= 1024, "whole waves, at most 16 of them");
    constexpr int NW = NT / 64;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = wave_incl_scan_i(v);
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        const int sv = lane < NW ? ws[lane] : 0;
        const int si = wave_incl_scan_i(sv);
        if (lane < NW) ws[lane] = si - sv;
        if (lane == 63) ws[NW] = si;
    }
    __syncthreads();
    const int r = ws[wave] + incl - v;
    total = ws[NW];
    __syncthreads();
    return r;
}
// the same for FOUR consecutive values per thread of a 256-thread workgroup (thread-major: thread t owns elements 4t .. 4t+3 of
// 1,024), as the ordered sweeps over the hash slots use it; ws: 5 ints of LDS
__device__ __forceinline__ void block_excl_scan_4(const int (&v)[4], int* ws, int (&excl)[4], int& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mine = v[0] + v[1] + v[2] + v[3];
    const int incl = wave_incl_scan_i(mine);
    if (lane == 63) ws[wave] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int a = ws[0], b = ws[1], c = ws[2], d = ws[3];
        ws[0] = 0; ws[1] = a; ws[2] = a + b; ws[3] = a + b + c; ws[4] = a + b + c + d;
    }
    __syncthreads();
    excl[0] = ws[wave] + incl - mine;
    excl[1] = excl[0] + v[0]; excl[2] = excl[1] + v[1]; excl[3] = excl[2] + v[2];
    total = ws[4];
    __syncthreads();
}
// ONE workgroup of NT threads: in-place exclusive scan of arr[0 .. n) (per-workgroup counts of an earlier launch; every thread
// sums a contiguous slice, block scan, running prefix written back) -> the sum of all n; ws as for block_excl_scan<NT>
template <int NT>
__device__ __forceinline__ int block_scan_counts(int32_t* __restrict__ arr, int n, int* ws) {
    const int per = (n + NT - 1) / NT;
    const int lo = min(n, (int)threadIdx.x * per), hi = min(n, lo + per);
    int sum = 0;
    for (int k = lo; k < hi; k++) sum += arr[k];
    int total;
    int run = block_excl_scan<NT>(sum, ws, total);
    for (int k = lo; k < hi; k++) { const int v = arr[k]; arr[k] = run; run += v; }
    return total;
}

// host milliseconds on the monotonic clock (launch-cost diagnostics)
static inline double wall_ms() {
    timespec t; clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}
