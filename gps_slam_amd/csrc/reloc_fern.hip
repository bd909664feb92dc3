// Keyframe relocaliser on the device (gps_reloc_*): InfiniTAM's FernRelocLib -- Relocaliser::ProcessFrame (Relocaliser.h:48-84)
// with its image chain (PixelUtils.h), fern code (FernConservatory.cpp:31-47), nearest-code search (RelocDatabase.cpp:24-71) and
// keyframe harvesting (Relocaliser.h:72-78) -- on the float depth image that view building leaves in HBM.  The reference does all
// of this on the CPU after downloading the depth image; here a frame is four stream-ordered launches and nothing is read back
// unless the caller asks for the result record:
//
//   reloc_pyramid_kernel    one workgroup per pixel of the 1/16 image: the four hole-aware 2x2 subsamples of its 16x16 block,
//                           level by level through LDS in the reference's summation order (the floats are the reference's)
//   reloc_blur_code_kernel  one workgroup: separable hole-aware Gaussian (x then y, 17 taps at sigma 2.5) in LDS, then one
//                           thread per fern compares the blurred image against the fern's thresholds
//   reloc_search_kernel     a fixed grid of waves over the stored codes: equal bytes per entry, best four of every wave as
//                           order-preserving packed keys (distance first, LATER entry first among equals)
//   reloc_finish_kernel     one wave: merges the waves' keys into the k nearest, decides the harvest, appends code + pose,
//                           writes the result record
//
// Everything that feeds a threshold comparison is the plain IEEE sequence of the reference: this file is compiled with
// -ffp-contract=off (_build.py) and carries the pragma below, and `/` on float is the correctly rounded division.
// The database is a flat uint8[capacity, numFerns] matrix: the reference's inverted lists (one id list per fern and code value)
// give the same similarity counts and exist here only in the text format host/relocaliser.cpp reads and writes (frames.txt).
#include <math.h>
#include <string.h>

#include <vector>

#include "common.hpp"
#include "launch_timing.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int RL_MAX_TAPS = 32;        // 17 at the reference's sigma
constexpr int RL_MAX_SMALL = 4096;     // pixels of the 1/16 image held in LDS by the blur (1024 x 1024 input)
constexpr int RL_SEARCH_BLOCKS_MAX = 64, RL_SEARCH_THREADS = 256, RL_WAVES_PER_BLOCK = RL_SEARCH_THREADS / 64;
constexpr unsigned long long RL_NO_KEY = ~0ull;
constexpr int RL_BLUR_THREADS = 1024;   // one workgroup: 1,200 pixels at 640 x 480
constexpr int RL_GUARD = 256, RL_GUARD_BYTE = 0xA5;

struct Taps { int n; float c[RL_MAX_TAPS]; };
struct Pose32 { float m[32]; };

// smaller key = nearer; among equal distances the larger id is the smaller key (RelocDatabase.cpp:45-51 shifts equal distances
// behind the newcomer, and entries arrive in ascending id)
__device__ __forceinline__ unsigned long long pack_key(int differing, int id) {
    return ((unsigned long long)(unsigned)differing << 32) | (unsigned)(0x7fffffff - id);
}
__device__ __forceinline__ int key_id(unsigned long long k) { return 0x7fffffff - (int)(unsigned)(k & 0xffffffffull); }
__device__ __forceinline__ int key_differing(unsigned long long k) { return (int)(k >> 32); }

__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int o) {
    const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffull), o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = shfl_xor_u64(v, o);
        v = t < v ? t : v;
    }
    return v;
}

// filterSubsample (PixelUtils.h:168-199) of one output pixel: contributors are v > 0 only, in the order (x,y) (x+1,y) (x,y+1)
// (x+1,y+1); sum / count, or 0 without one
__device__ __forceinline__ float subsample4(float a, float b, float c, float d) {
    int num = 0;
    float sum = 0.0f;
    if (a > 0.0f) { num++; sum += a; }
    if (b > 0.0f) { num++; sum += b; }
    if (c > 0.0f) { num++; sum += c; }
    if (d > 0.0f) { num++; sum += d; }
    return num > 0 ? sum / (float)num : 0.0f;
}

// Pixel (X, Y) of the fourth level reads input pixels 16X .. 16X+15, 16Y .. 16Y+15 only: every level's size is the floor of half
// the previous one, so a dropped odd last row / column is never inside a surviving block, and 16 * (w >> 4) <= w.
__global__ __launch_bounds__(256) void reloc_pyramid_kernel(int w, int w4, const float* __restrict__ depth, float* __restrict__ small,
                                                            gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    __shared__ float l0[256], l1[64], l2[16], l3[4];
    const int t = threadIdx.x, X = blockIdx.x % w4, Y = blockIdx.x / w4;
    l0[t] = depth[(size_t)(16 * Y + (t >> 4)) * w + 16 * X + (t & 15)];
    __syncthreads();
    if (t < 64) {
        const int x = 2 * (t & 7), y = 2 * (t >> 3);
        l1[t] = subsample4(l0[y * 16 + x], l0[y * 16 + x + 1], l0[(y + 1) * 16 + x], l0[(y + 1) * 16 + x + 1]);
    }
    __syncthreads();
    if (t < 16) {
        const int x = 2 * (t & 3), y = 2 * (t >> 2);
        l2[t] = subsample4(l1[y * 8 + x], l1[y * 8 + x + 1], l1[(y + 1) * 8 + x], l1[(y + 1) * 8 + x + 1]);
    }
    __syncthreads();
    if (t < 4) {
        const int x = 2 * (t & 1), y = 2 * (t >> 1);
        l3[t] = subsample4(l2[y * 4 + x], l2[y * 4 + x + 1], l2[(y + 1) * 4 + x], l2[(y + 1) * 4 + x + 1]);
    }
    __syncthreads();
    if (t == 0) small[blockIdx.x] = subsample4(l3[0], l3[1], l3[2], l3[3]);
}

// filterSeparable_x / _y (PixelUtils.h:15-48, 87-119): taps outside the image and holes (v <= 0) are skipped
__device__ __forceinline__ float blur_tap_sum(const float* img, int base, int stride, int pos, int extent, int n_taps, const float* coeff) {
    const int s2 = n_taps / 2;
    float sum_v = 0.0f, sum_c = 0.0f;
    for (int i = 0; i < n_taps; ++i) {
        const int p = pos + i - s2;
        if (p < 0) continue;
        if (p >= extent) continue;
        const float v = img[base + p * stride];
        if (v <= 0.0f) continue;
        sum_c += coeff[i];
        sum_v += coeff[i] * v;
    }
    return sum_c > 0.0f ? sum_v / sum_c : 0.0f;
}

__global__ __launch_bounds__(RL_BLUR_THREADS) void reloc_blur_code_kernel(int w4, int h4, Taps taps, const float* __restrict__ small,
                                                              int num_ferns, int num_dec, const int* __restrict__ fern_xy,
                                                              const float* __restrict__ fern_thr, uint8_t* __restrict__ code,
                                                              float* __restrict__ dbg_blurred, uint8_t* __restrict__ dbg_code,
                                                              gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    __shared__ float a[RL_MAX_SMALL], b[RL_MAX_SMALL], coeff[RL_MAX_TAPS];
    const int n = w4 * h4;
    // (the coefficients go to LDS: indexing the by-value argument with a loop counter put it into scratch memory, and the launch
    // took 21 us inside the tracked schedule)
    if (threadIdx.x < RL_MAX_TAPS) coeff[threadIdx.x] = threadIdx.x < taps.n ? taps.c[threadIdx.x] : 0.0f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) a[i] = small[i];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int y = i / w4, x = i - y * w4;
        b[i] = blur_tap_sum(a, y * w4, 1, x, w4, taps.n, coeff);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int y = i / w4, x = i - y * w4;
        const float v = blur_tap_sum(b, x, w4, y, h4, taps.n, coeff);
        a[i] = v;   // (thread i is the only reader of a[i] since the first barrier)
        if (dbg_blurred) dbg_blurred[i] = v;
    }
    __syncthreads();
    // FernConservatory::computeCode (FernConservatory.cpp:31-47); locations were checked against w4 x h4 by gps_reloc_set_ferns
    for (int f = threadIdx.x; f < num_ferns; f += blockDim.x) {
        unsigned c = 0;
        for (int d = 0; d < num_dec; ++d) {
            const int e = f * num_dec + d;
            const float val = a[fern_xy[2 * e] + fern_xy[2 * e + 1] * w4];
            c |= ((val < fern_thr[e]) ? 0u : 1u) << d;
        }
        code[f] = (uint8_t)c;
        if (dbg_code) dbg_code[f] = (uint8_t)c;
    }
}

// keeps k0 <= k1 <= k2 <= k3 (wave-uniform values)
__device__ __forceinline__ void keep4(unsigned long long key, unsigned long long (&best)[4]) {
    if (key >= best[3]) return;
    best[3] = key;
#pragma unroll
    for (int j = 3; j > 0; --j)
        if (best[j] < best[j - 1]) { const unsigned long long t = best[j]; best[j] = best[j - 1]; best[j - 1] = t; }
}

// One wave per entry at a time, entries strided over all waves of the (fixed) grid; the number of entries is read on the device.
// Every wave leaves its four best keys in partial[wave * 4 ..] (RL_NO_KEY where it has fewer).
__global__ __launch_bounds__(RL_SEARCH_THREADS) void reloc_search_kernel(int num_ferns, const uint8_t* __restrict__ codes,
                                                                        const int* __restrict__ count, const uint8_t* __restrict__ code,
                                                                        unsigned long long* __restrict__ partial, gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    const int wave = (int)(blockIdx.x * RL_WAVES_PER_BLOCK + (threadIdx.x >> 6)), n_waves = (int)gridDim.x * RL_WAVES_PER_BLOCK;
    const int lane = threadIdx.x & 63, n = *count;
    unsigned long long best[4] = {RL_NO_KEY, RL_NO_KEY, RL_NO_KEY, RL_NO_KEY};
    for (int e = wave; e < n; e += n_waves) {
        const uint8_t* row = codes + (size_t)e * num_ferns;
        int same = 0;
        for (int f = lane; f < num_ferns; f += 64) same += row[f] == code[f] ? 1 : 0;
        same = wave_sum_i(same);
        keep4(pack_key(num_ferns - same, e), best);
    }
    if (lane < 4) partial[(size_t)wave * 4 + lane] = lane == 0 ? best[0] : lane == 1 ? best[1] : lane == 2 ? best[2] : best[3];
}

// gps_reloc_result as the device writes it
struct ResultRec { int32_t added_id, n_found, ids[4]; float distances[4]; int32_t n_entries, overflow; };

__global__ __launch_bounds__(64) void reloc_finish_kernel(int num_ferns, int capacity, int n_partial, int k, int harvest,
                                                          float harvest_threshold, int scene_id, Pose32 pose,
                                                          const unsigned long long* __restrict__ partial, const uint8_t* __restrict__ code,
                                                          uint8_t* __restrict__ codes, float* __restrict__ poses, int* __restrict__ scene_ids,
                                                          int* __restrict__ count, int* __restrict__ overflow, ResultRec* __restrict__ result,
                                                          gps::LaunchStamp stamp) {
    gps::StampScope timed(stamp);
    const int lane = threadIdx.x;
    // the k smallest keys, one per round: keys are distinct (they carry the id), so "the smallest above the previous" is exact
    unsigned long long prev = 0, sel[4];
    bool first = true;
    int n_found = 0;
    for (int r = 0; r < 4; ++r) {
        sel[r] = RL_NO_KEY;
        if (r >= k) continue;
        unsigned long long m = RL_NO_KEY;
        for (int i = lane; i < n_partial; i += 64) {
            const unsigned long long key = partial[i];
            if ((first || key > prev) && key < m) m = key;
        }
        m = wave_min_u64(m);
        if (m == RL_NO_KEY) break;
        sel[r] = m; prev = m; first = false; n_found = r + 1;
    }
    for (int r = n_found; r < 4; ++r) sel[r] = RL_NO_KEY;
    // distance = ((float)codeLength - (float)similarity) / (float)codeLength (RelocDatabase.cpp:42); the difference is exact
    float dist[4];
    int ids[4];
    for (int r = 0; r < 4; ++r) {
        const bool have = r < n_found;
        ids[r] = have ? key_id(sel[r]) : -1;
        dist[r] = have ? (float)key_differing(sel[r]) / (float)num_ferns : 1.0f;
    }
    const int n = *count;
    int added = -1, n_after = n, over = *overflow;
    if (harvest && (n_found == 0 || dist[0] > harvest_threshold)) {   // Relocaliser.h:72-78
        if (n < capacity) {
            added = n;
            n_after = n + 1;
            for (int f = lane; f < num_ferns; f += 64) codes[(size_t)added * num_ferns + f] = code[f];
            if (lane < 32) poses[(size_t)added * 32 + lane] = pose.m[lane];
            if (lane == 0) scene_ids[added] = scene_id;
        } else {
            over += 1;   // a full database adds nothing and never writes past the matrix
        }
    }
    if (lane == 0) {
        *count = n_after;
        *overflow = over;
        result->added_id = added;
        result->n_found = n_found;
        for (int r = 0; r < 4; ++r) { result->ids[r] = r < k ? ids[r] : -1; result->distances[r] = r < k ? dist[r] : 1.0f; }
        result->n_entries = n_after;
        result->overflow = over;
    }
}

// splitmix64 (public domain, Vigna): the library's own generator for the default fern table
inline uint64_t splitmix64(uint64_t& s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
inline float uniform01(uint64_t& s) { return (float)(splitmix64(s) >> 40) * (1.0f / 16777216.0f); }   // [0, 1)

}  // namespace

struct gps_reloc_state {
    int width, height, w4, h4, num_ferns, num_dec, capacity, search_blocks;
    float range_min, range_max, harvest_threshold;
    Taps taps;
    std::vector<int32_t> host_xy;
    std::vector<float> host_thr;
    // device memory (one allocation)
    char* dev;
    float* small;
    int32_t* fern_xy;
    float* fern_thr;
    uint8_t* code;
    uint8_t* codes;
    float* poses;
    int32_t* scene_ids;
    unsigned long long* partial;
    int32_t* count;      // [0] entries, [1] overflow
    ResultRec* result;
    float* dbg_blurred;
    uint8_t* dbg_code;
};

static_assert(sizeof(ResultRec) == sizeof(gps_reloc_result), "gps_reloc_result layout");

static bool reloc_dims_ok(int width, int height, int num_ferns, int num_dec) {
    return width >= 32 && height >= 32 && (int64_t)(width >> 4) * (height >> 4) <= RL_MAX_SMALL && num_ferns > 0 &&
           num_ferns <= 65536 && num_dec >= 1 && num_dec <= 7;
}

extern "C" {

int gps_reloc_gaussian_taps(float sigma, int max_taps, float* coeff, int* n_taps) {
    GPS_REQUIRE(coeff && n_taps && sigma > 0.0f);
    // filterGaussian / createGaussianFilter (PixelUtils.h:9-13, 158-163)
    int filtersize = (int)(2.0f * 3.5f * sigma);
    if ((filtersize & 1) == 0) filtersize += 1;
    GPS_REQUIRE(filtersize <= max_taps && filtersize <= RL_MAX_TAPS);
    const int half = filtersize / 2;
    for (int i = 0; i < filtersize; ++i) coeff[i] = expf(-(i - half) * (i - half) / (2.0f * sigma * sigma));
    *n_taps = filtersize;
    return GPS_OK;
}

int gps_reloc_default_ferns(int width, int height, int num_ferns, int num_decisions, float range_min, float range_max,
                            uint64_t seed, int32_t* xy, float* thresholds) {
    GPS_REQUIRE(reloc_dims_ok(width, height, num_ferns, num_decisions) && xy && thresholds && range_max >= range_min);
    // FernConservatory.cpp:19-23 with Relocaliser.h:29-30's image size: locations are drawn in imgSize / 32 although the code is
    // computed on the imgSize / 16 image -- the ferns only look at the upper left quarter.  Kept, so that a table of ours and a
    // table of the reference's are samples of the same distribution.  (Uniforms are in [0, 1): the reference's can be 1.0.)
    const int lw = width / 32, lh = height / 32;
    uint64_t s = seed;
    for (int e = 0; e < num_ferns * num_decisions; ++e) {
        xy[2 * e] = (int)floorf(uniform01(s) * (float)lw);
        xy[2 * e + 1] = (int)floorf(uniform01(s) * (float)lh);
        thresholds[e] = uniform01(s) * (range_max - range_min) + range_min;
    }
    return GPS_OK;
}

int gps_reloc_create(gps_reloc_state** out, int width, int height, int num_ferns, int num_decisions, float range_min,
                     float range_max, float harvest_threshold, int capacity, uint64_t seed) {
    GPS_REQUIRE(out);
    *out = nullptr;
    GPS_REQUIRE(reloc_dims_ok(width, height, num_ferns, num_decisions) && capacity > 0 && range_max >= range_min);
    GPS_REQUIRE((int64_t)capacity * num_ferns <= ((int64_t)1 << 31));
    GPS_ENTER();
    gps_reloc_state* s = new gps_reloc_state();
    s->width = width; s->height = height; s->w4 = width >> 4; s->h4 = height >> 4;
    s->num_ferns = num_ferns; s->num_dec = num_decisions; s->capacity = capacity;
    s->range_min = range_min; s->range_max = range_max; s->harvest_threshold = harvest_threshold;
    s->search_blocks = gps_div_up(capacity, RL_WAVES_PER_BLOCK * 4);   // ~4 entries per wave before the grid stops growing
    if (s->search_blocks > RL_SEARCH_BLOCKS_MAX) s->search_blocks = RL_SEARCH_BLOCKS_MAX;
    s->dbg_blurred = nullptr; s->dbg_code = nullptr;
    int n_taps = 0;
    gps_reloc_gaussian_taps(2.5f, RL_MAX_TAPS, s->taps.c, &n_taps);   // Relocaliser.h:56
    s->taps.n = n_taps;
    const int n_dec = num_ferns * num_decisions;
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_small = up(sizeof(float) * s->w4 * s->h4), b_xy = up(8 * (size_t)n_dec), b_thr = up(4 * (size_t)n_dec),
                 b_code = up(num_ferns), b_codes = up((size_t)capacity * num_ferns + RL_GUARD), b_poses = up((size_t)capacity * 128 + RL_GUARD),
                 b_scene = up((size_t)capacity * 4 + RL_GUARD), b_partial = up((size_t)s->search_blocks * RL_WAVES_PER_BLOCK * 4 * 8),
                 b_count = 256, b_result = 256;
    const size_t total = b_small + b_xy + b_thr + b_code + b_codes + b_poses + b_scene + b_partial + b_count + b_result;
    if (hipMalloc(reinterpret_cast<void**>(&s->dev), total) != hipSuccess) { delete s; (void)hipGetLastError(); return GPS_ERR_LAUNCH; }
    char* p = s->dev;
    s->small = reinterpret_cast<float*>(p); p += b_small;
    s->fern_xy = reinterpret_cast<int32_t*>(p); p += b_xy;
    s->fern_thr = reinterpret_cast<float*>(p); p += b_thr;
    s->code = reinterpret_cast<uint8_t*>(p); p += b_code;
    s->codes = reinterpret_cast<uint8_t*>(p); p += b_codes;
    s->poses = reinterpret_cast<float*>(p); p += b_poses;
    s->scene_ids = reinterpret_cast<int32_t*>(p); p += b_scene;
    s->partial = reinterpret_cast<unsigned long long*>(p); p += b_partial;
    s->count = reinterpret_cast<int32_t*>(p); p += b_count;
    s->result = reinterpret_cast<ResultRec*>(p);
    // RL_GUARD bytes of a fixed pattern directly behind each of the three per-entry arrays (gps_reloc_check_guards)
    if (hipMemset(s->dev, 0, total) != hipSuccess || hipMemset(s->codes + (size_t)capacity * num_ferns, RL_GUARD_BYTE, RL_GUARD) != hipSuccess ||
        hipMemset(s->poses + (size_t)capacity * 32, RL_GUARD_BYTE, RL_GUARD) != hipSuccess ||
        hipMemset(s->scene_ids + capacity, RL_GUARD_BYTE, RL_GUARD) != hipSuccess) {
        (void)hipFree(s->dev); delete s; return GPS_ERR_LAUNCH;
    }
    s->host_xy.resize(2 * (size_t)n_dec);
    s->host_thr.resize(n_dec);
    gps_reloc_default_ferns(width, height, num_ferns, num_decisions, range_min, range_max, seed, s->host_xy.data(), s->host_thr.data());
    if (hipMemcpy(s->fern_xy, s->host_xy.data(), 8 * (size_t)n_dec, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(s->fern_thr, s->host_thr.data(), 4 * (size_t)n_dec, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(s->dev); delete s; return GPS_ERR_LAUNCH;
    }
    if (hipStreamSynchronize(nullptr) != hipSuccess) { (void)hipFree(s->dev); delete s; return GPS_ERR_LAUNCH; }
    *out = s;
    return GPS_OK;
}

int gps_reloc_destroy(gps_reloc_state* s) {
    GPS_REQUIRE(s);
    const bool ok = hipFree(s->dev) == hipSuccess;
    delete s;
    return ok ? GPS_OK : GPS_ERR_LAUNCH;
}

int gps_reloc_info(const gps_reloc_state* s, int32_t* info) {
    GPS_REQUIRE(s && info);
    info[0] = s->width; info[1] = s->height; info[2] = s->w4; info[3] = s->h4;
    info[4] = s->num_ferns; info[5] = s->num_dec; info[6] = s->capacity; info[7] = s->taps.n;
    return GPS_OK;
}

int gps_reloc_set_ferns(gps_reloc_state* s, const int32_t* xy, const float* thresholds, int count, gps_stream stream) {
    GPS_REQUIRE(s && xy && thresholds);
    GPS_REQUIRE(count == s->num_ferns * s->num_dec);   // size mismatch
    for (int e = 0; e < count; ++e)   // the code kernel indexes the 1/16 image with these
        GPS_REQUIRE(xy[2 * e] >= 0 && xy[2 * e] < s->w4 && xy[2 * e + 1] >= 0 && xy[2 * e + 1] < s->h4);
    hipStream_t st = (hipStream_t)stream;
    // (the caller's arrays are pageable: the state's own copy is the source of the asynchronous upload, and the stream is
    // drained before that copy may change again)
    if (hipStreamSynchronize(st) != hipSuccess) return GPS_ERR_LAUNCH;
    memcpy(s->host_xy.data(), xy, 8 * (size_t)count);
    memcpy(s->host_thr.data(), thresholds, 4 * (size_t)count);
    if (hipMemcpyAsync(s->fern_xy, s->host_xy.data(), 8 * (size_t)count, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(s->fern_thr, s->host_thr.data(), 4 * (size_t)count, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return GPS_ERR_LAUNCH;
    return GPS_OK;
}

int gps_reloc_get_ferns(const gps_reloc_state* s, int32_t* xy, float* thresholds, int count) {
    GPS_REQUIRE(s && xy && thresholds && count == s->num_ferns * s->num_dec);
    memcpy(xy, s->host_xy.data(), 8 * (size_t)count);
    memcpy(thresholds, s->host_thr.data(), 4 * (size_t)count);
    return GPS_OK;
}

int gps_reloc_set_debug_outputs(gps_reloc_state* s, float* blurred, uint8_t* code) {
    GPS_REQUIRE(s);
    s->dbg_blurred = blurred;
    s->dbg_code = code;
    return GPS_OK;
}

int gps_reloc_process_frame(gps_reloc_state* s, const float* depth_f32, const float* pose_M, const float* pose_invM, int scene_id,
                            int k, int harvest, gps_stream stream) {
    GPS_REQUIRE(s && depth_f32 && pose_M && pose_invM);
    GPS_REQUIRE(k >= 1 && k <= GPS_RELOC_MAX_K);
    GPS_ENTER();
    hipStream_t st = (hipStream_t)stream;
    Pose32 pose;
    memcpy(pose.m, pose_M, 64);
    memcpy(pose.m + 16, pose_invM, 64);
    gps::launch_kernel(gps::TK_RELOC_PYRAMID, 0, reloc_pyramid_kernel, dim3(s->w4 * s->h4), dim3(256), 0, st, s->width, s->w4, depth_f32,
                       s->small);
    gps::launch_kernel(gps::TK_RELOC_BLUR_CODE, 0, reloc_blur_code_kernel, dim3(1), dim3(RL_BLUR_THREADS), 0, st, s->w4, s->h4, s->taps,
                       (const float*)s->small, s->num_ferns, s->num_dec, (const int*)s->fern_xy, (const float*)s->fern_thr, s->code,
                       s->dbg_blurred, s->dbg_code);
    gps::launch_kernel(gps::TK_RELOC_SEARCH, 0, reloc_search_kernel, dim3(s->search_blocks), dim3(RL_SEARCH_THREADS), 0, st, s->num_ferns,
                       (const uint8_t*)s->codes, (const int*)s->count, (const uint8_t*)s->code, s->partial);
    gps::launch_kernel(gps::TK_RELOC_FINISH, 0, reloc_finish_kernel, dim3(1), dim3(64), 0, st, s->num_ferns, s->capacity,
                       s->search_blocks * RL_WAVES_PER_BLOCK * 4, k, harvest ? 1 : 0, s->harvest_threshold, scene_id, pose,
                       (const unsigned long long*)s->partial, (const uint8_t*)s->code, s->codes, s->poses, (int*)s->scene_ids, (int*)s->count,
                       (int*)(s->count + 1), s->result);
    GPS_LAUNCH_CHECK();
    return GPS_OK;
}

int gps_reloc_read_result(gps_reloc_state* s, gps_reloc_result* out, gps_stream stream) {
    GPS_REQUIRE(s && out);
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(out, s->result, sizeof(gps_reloc_result), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return GPS_ERR_LAUNCH;
    return GPS_OK;
}

static int reloc_read_count(gps_reloc_state* s, hipStream_t st, int32_t* two) {
    if (hipMemcpyAsync(two, s->count, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return GPS_ERR_LAUNCH;
    return GPS_OK;
}

int gps_reloc_retrieve_pose(gps_reloc_state* s, int id, float* pose_M, float* pose_invM, int32_t* scene_id, gps_stream stream) {
    GPS_REQUIRE(s && pose_M && pose_invM && id >= 0 && id < s->capacity);
    hipStream_t st = (hipStream_t)stream;
    int32_t cnt[2];
    if (reloc_read_count(s, st, cnt) != GPS_OK) return GPS_ERR_LAUNCH;
    GPS_REQUIRE(id < cnt[0]);
    float m[32];
    int32_t sc = 0;
    if (hipMemcpyAsync(m, s->poses + (size_t)id * 32, 128, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&sc, s->scene_ids + id, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return GPS_ERR_LAUNCH;
    memcpy(pose_M, m, 64);
    memcpy(pose_invM, m + 16, 64);
    if (scene_id) *scene_id = sc;
    return GPS_OK;
}

int gps_reloc_export(gps_reloc_state* s, int max_entries, uint8_t* codes, float* poses, int32_t* scene_ids, int32_t* n_entries,
                     int32_t* overflow, gps_stream stream) {
    GPS_REQUIRE(s && n_entries && max_entries >= 0);
    hipStream_t st = (hipStream_t)stream;
    int32_t cnt[2];
    if (reloc_read_count(s, st, cnt) != GPS_OK) return GPS_ERR_LAUNCH;
    *n_entries = cnt[0];
    if (overflow) *overflow = cnt[1];
    if (!codes && !poses && !scene_ids) return GPS_OK;   // the count alone
    if (cnt[0] > max_entries) return GPS_ERR_CAPACITY;
    const size_t n = (size_t)cnt[0];
    if (n == 0) return GPS_OK;
    if ((codes && hipMemcpyAsync(codes, s->codes, n * s->num_ferns, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (poses && hipMemcpyAsync(poses, s->poses, n * 128, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        (scene_ids && hipMemcpyAsync(scene_ids, s->scene_ids, n * 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return GPS_ERR_LAUNCH;
    return GPS_OK;
}

int gps_reloc_check_guards(gps_reloc_state* s, gps_stream stream) {
    GPS_REQUIRE(s);
    hipStream_t st = (hipStream_t)stream;
    uint8_t g[3][RL_GUARD];
    if (hipMemcpyAsync(g[0], s->codes + (size_t)s->capacity * s->num_ferns, RL_GUARD, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(g[1], s->poses + (size_t)s->capacity * 32, RL_GUARD, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(g[2], s->scene_ids + s->capacity, RL_GUARD, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return GPS_ERR_LAUNCH;
    for (int a = 0; a < 3; ++a)
        for (int i = 0; i < RL_GUARD; ++i)
            if (g[a][i] != RL_GUARD_BYTE) return GPS_ERR_CAPACITY;
    return GPS_OK;
}

int gps_reloc_import(gps_reloc_state* s, int n_entries, const uint8_t* codes, const float* poses, const int32_t* scene_ids,
                     gps_stream stream) {
    GPS_REQUIRE(s && n_entries >= 0);
    if (n_entries > s->capacity) return GPS_ERR_CAPACITY;
    GPS_REQUIRE(n_entries == 0 || (codes && poses && scene_ids));
    hipStream_t st = (hipStream_t)stream;
    const size_t n = (size_t)n_entries;
    const int32_t cnt[2] = {n_entries, 0};
    if ((n && (hipMemcpyAsync(s->codes, codes, n * s->num_ferns, hipMemcpyHostToDevice, st) != hipSuccess ||
               hipMemcpyAsync(s->poses, poses, n * 128, hipMemcpyHostToDevice, st) != hipSuccess ||
               hipMemcpyAsync(s->scene_ids, scene_ids, n * 4, hipMemcpyHostToDevice, st) != hipSuccess)) ||
        hipMemcpyAsync(s->count, cnt, 8, hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return GPS_ERR_LAUNCH;
    return GPS_OK;
}

}  // extern "C"
