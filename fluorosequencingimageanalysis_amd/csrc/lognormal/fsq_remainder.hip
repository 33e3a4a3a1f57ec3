// fsq_remainder.hip - the remainder correction of track photometries (include/fsq_remainder.h): MCsimlib._remainder_adjust_2
// (:3434-3472) and _remainder_adjust (:3398-3431), with numpy's bits.  Four kernels on one stream:
//
// krm_tracks, one wavefront per track (:3441-3446, :3402-3408): finds the track's segment (a binary search of seg_off) and
//   notes it for krm_apply.  A remainder (all F category bits set) takes a slot of its segment from an atomic counter, which
//   is n_remainders itself, and lane f writes the track's value at frame f to the workspace, segment by segment and frame by
//   frame: ws[F * seg_off[s] + f * cap + slot], cap the segment's tracks.  In RATIO mode the value is (I_f - m) / m with m the
//   track's median: every lane ranks its intensity against the others' (ties by lane) with F wave shuffles, so nothing is
//   indexed at run time and nothing goes to scratch.
// krm_medians, one 256-thread block per (segment, frame) (:3454, :3414): the exact median of the R values, on their
//   order-preserving 64-bit keys.  Up to FSQ_REMAINDER_LDS_MAX values sit in LDS and every thread ranks its own against all.
//   Above, a radix select of eight 8-bit passes over the workspace (a 256-bin LDS histogram of the keys that share the prefix
//   found so far, then one wavefront scans it) finds the lower middle key and how many keys are at most it; where the upper
//   middle is another key, a ninth pass takes the least key above.  A NaN among the values gives NaN; R = 0 gives NaN.
// krm_finish, one thread per segment: kept (:3450, :3412) and, in ADDITIVE mode, median_f - median_0 (:3416).
// krm_apply, one thread per value (:3468, :3427): 8 bytes read, 8 written.
//
// Bounds: a segment is used only where 0 <= seg_off[s] <= seg_off[s + 1] <= n; a slot only below the segment's capacity.  With
// that every workspace index is below n * F, whatever seg_off holds.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../fsq_common.h"
#include "../../../include/fsq_remainder.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int TRACKS_PER_BLOCK = THREADS / WAVE;
constexpr int LDS_MAX = FSQ_REMAINDER_LDS_MAX;
static_assert(FSQ_REMAINDER_MAX_FRAMES <= WAVE, "one lane per frame");
static_assert(LDS_MAX % THREADS == 0, "whole rounds of the block");

typedef unsigned long long u64;

// the key orders as the double does: negative numbers reversed below the positive ones, -0.0 just below +0.0
__device__ __forceinline__ u64 key_of(double x)
{
    const u64 u = (u64)__double_as_longlong(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double value_of(u64 k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// np.median's mean of its one or two middle values.  np.mean is np.add.reduce over the count, and the reduction is
// a[0] + (0.0 + a[1] + ...): the sum of the others starts from +0.0.  That only shows on zeros: a median of -0.0 is +0.0.
__device__ __forceinline__ double middle_mean(double a, double b, bool odd)
{
    return odd ? a + 0.0 : (a + (0.0 + b)) / 2.0;
}

// the segment of track i, or -1: seg_off[s] <= i < seg_off[s + 1] with both inside 0 .. n
__device__ __forceinline__ long long segment_of(const long long* __restrict__ seg_off, long long S, long long n, long long i,
                                                long long* off, long long* cap)
{
    long long a = 0, b = S + 1;                                    // c = #{j <= S : seg_off[j] <= i}
    while (a < b) {
        const long long mid = a + ((b - a) >> 1);
        if (seg_off[mid] <= i) a = mid + 1; else b = mid;
    }
    const long long s = a - 1;
    if (s < 0 || s >= S) return -1;
    const long long o = seg_off[s], e = seg_off[s + 1];
    if (o < 0 || e > n || !(o <= i && i < e)) return -1;
    *off = o;
    *cap = e - o;
    return s;
}

__global__ void __launch_bounds__(THREADS)
krm_tracks(const double* __restrict__ intensity, const u64* __restrict__ category, const long long* __restrict__ seg_off,
           long long n, int F, long long S, int mode, int* __restrict__ n_remainders, double* __restrict__ ws_values,
           int* __restrict__ ws_segment)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long i = (long long)blockIdx.x * TRACKS_PER_BLOCK + (threadIdx.x / WAVE);
    if (i >= n) return;                                            // (uniform over the wavefront; the kernel has no barrier)
    long long off = 0, cap = 0;
    const long long s = segment_of(seg_off, S, n, i, &off, &cap);
    if (lane == 0) ws_segment[i] = (int)s;
    const u64 all_on = F == 64 ? ~0ull : ((1ull << F) - 1ull);
    if (s < 0 || (category[i] & all_on) != all_on) return;
    const bool live = lane < F;
    const double x = live ? intensity[i * F + lane] : 0.0;
    double v = x;
    if (mode == FSQ_REMAINDER_RATIO) {
        int rank = 0;                                              // #{g : I_g < I_f, or equal and g < f}
        for (int g = 0; g < F; g++) {
            const double xg = __shfl(x, g, WAVE);
            rank += (xg < x || (xg == x && g < lane)) ? 1 : 0;
        }
        const u64 lo = __ballot(live && rank == (F - 1) / 2), hi = __ballot(live && rank == F / 2);
        double m = __builtin_nan("");                              // (no lane holds a rank among NaNs)
        if (lo && hi) m = middle_mean(__shfl(x, __ffsll((long long)lo) - 1, WAVE), __shfl(x, __ffsll((long long)hi) - 1, WAVE), F & 1);
        v = (x - m) / m;
    }
    int slot = 0;
    if (lane == 0) slot = atomicAdd(&n_remainders[s], 1);
    slot = __shfl(slot, 0, WAVE);
    if (live && slot < cap) ws_values[(long long)F * off + lane * cap + slot] = v;
}

// R of segment s and where its tracks start and how many they are; R = 0 for a segment that is not well formed
__device__ __forceinline__ int remainders_of(const long long* __restrict__ seg_off, const int* __restrict__ n_remainders,
                                             long long n, long long s, long long* off, long long* cap)
{
    const long long o = seg_off[s], e = seg_off[s + 1];
    *off = 0;
    *cap = 0;
    if (o < 0 || e > n || e < o) return 0;
    *off = o;
    *cap = e - o;
    const long long r = n_remainders[s];
    return (int)(r < e - o ? r : e - o);
}

__global__ void __launch_bounds__(THREADS)
krm_medians(const double* __restrict__ ws_values, const long long* __restrict__ seg_off, const int* __restrict__ n_remainders,
            long long n, int F, double* __restrict__ median)
{
    __shared__ u64 s_key[LDS_MAX];
    __shared__ int s_hist[256];
    __shared__ u64 s_pick[2];
    __shared__ int s_digit, s_below, s_equal;
    const int tid = threadIdx.x;
    const long long s = blockIdx.x / F;
    const int f = (int)(blockIdx.x % F);
    long long off, cap;
    const int R = remainders_of(seg_off, n_remainders, n, s, &off, &cap);
    const double* v = ws_values + (long long)F * off + f * cap;    // the R values of (segment s, frame f)
    double* out = median + s * F + f;
    if (R <= 0) {                                                  // (every exit below is uniform over the block)
        if (tid == 0) *out = __builtin_nan("");
        return;
    }
    const int k1 = (R - 1) / 2, k2 = R / 2;
    if (R <= LDS_MAX) {
        int nan = 0;
        for (int e = tid; e < R; e += THREADS) {
            const double x = v[e];
            nan |= x != x;
            s_key[e] = key_of(x);
        }
        if (__syncthreads_or(nan)) {
            if (tid == 0) *out = __builtin_nan("");
            return;
        }
        for (int e = tid; e < R; e += THREADS) {
            const u64 k = s_key[e];
            int rank = 0;                                          // #{j : key_j < key_e, or equal and j < e}
            for (int j = 0; j < R; j++) {
                const u64 kj = s_key[j];
                rank += (kj < k || (kj == k && j < e)) ? 1 : 0;
            }
            if (rank == k1) s_pick[0] = k;
            if (rank == k2) s_pick[1] = k;
        }
        __syncthreads();
        if (tid == 0) *out = middle_mean(value_of(s_pick[0]), value_of(s_pick[1]), R & 1);
        return;
    }
    // ---- radix select of the k1-th key, the most significant byte first ----
    u64 prefix = 0;
    int below = 0;                                                 // keys less than every key with this prefix
    for (int shift = 56; shift >= 0; shift -= 8) {
        s_hist[tid] = 0;
        __syncthreads();
        int nan = 0;
        for (int e = tid; e < R; e += THREADS) {
            const double x = v[e];
            nan |= x != x;
            const u64 k = key_of(x);
            if (shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&s_hist[(int)((k >> shift) & 255)], 1);
        }
        if (__syncthreads_or(shift == 56 ? nan : 0)) {
            if (tid == 0) *out = __builtin_nan("");
            return;
        }
        if (tid < WAVE) {                                          // lane l owns bins 4l .. 4l + 3
            int c[4], tot = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) { c[q] = s_hist[4 * tid + q]; tot += c[q]; }
            int incl = tot;
#pragma unroll
            for (int d = 1; d < WAVE; d <<= 1) {
                const int up = __shfl_up(incl, d, WAVE);
                if (tid >= d) incl += up;
            }
            int before = incl - tot;
            const int want = k1 - below;                           // 0 <= want < the keys with this prefix
            if (before <= want && want < incl) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (before <= want && want < before + c[q]) { s_digit = 4 * tid + q; s_below = before; s_equal = c[q]; }
                    before += c[q];
                }
            }
        }
        __syncthreads();
        prefix |= (u64)s_digit << shift;
        below += s_below;
        __syncthreads();                                           // (s_digit is read before the next pass writes it)
    }
    u64 upper = prefix;                                            // the k2-th key
    const int at_most = below + s_equal;                           // #{key <= prefix}; s_equal is the last pass's
    if (k2 >= at_most) {                                           // (uniform: below and s_equal are the block's)
        if (tid == 0) s_pick[0] = ~0ull;
        __syncthreads();
        u64 least = ~0ull;
        for (int e = tid; e < R; e += THREADS) {
            const u64 k = key_of(v[e]);
            if (k > prefix && k < least) least = k;
        }
        atomicMin(&s_pick[0], least);
        __syncthreads();
        upper = s_pick[0];
    }
    if (tid == 0) *out = middle_mean(value_of(prefix), value_of(upper), R & 1);
}

__global__ void __launch_bounds__(THREADS)
krm_finish(const long long* __restrict__ seg_off, const int* __restrict__ n_remainders, long long n, int F, long long S, int mode,
           int minimum, double* __restrict__ adjustment, unsigned char* __restrict__ kept)
{
    const long long s = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (s >= S) return;
    long long off, cap;
    const int R = remainders_of(seg_off, n_remainders, n, s, &off, &cap);
    kept[s] = (R >= minimum && (mode == FSQ_REMAINDER_RATIO || R >= 1)) ? 1 : 0;
    if (mode == FSQ_REMAINDER_ADDITIVE) {
        const double m0 = adjustment[s * F];
        for (int f = 0; f < F; f++) adjustment[s * F + f] = adjustment[s * F + f] - m0;
    }
}

__global__ void __launch_bounds__(THREADS)
krm_apply(const double* __restrict__ intensity, const int* __restrict__ ws_segment, const double* __restrict__ adjustment,
          const unsigned char* __restrict__ kept, long long total, int F, int mode, double* __restrict__ adjusted)
{
    const long long base = (long long)blockIdx.x * THREADS;        // (uniform: the 64-bit division is the block's, not the lane's)
    const long long i0 = base / F;
    const unsigned t = (unsigned)(base - i0 * F) + threadIdx.x;    // < F + THREADS
    const long long idx = base + threadIdx.x;
    if (idx >= total) return;
    const long long i = i0 + t / (unsigned)F;
    const int f = (int)(t % (unsigned)F);
    const int s = ws_segment[i];
    double r = 0.0;
    if (s >= 0 && kept[s]) {
        const double a = adjustment[(long long)s * F + f], x = intensity[idx];
        r = mode == FSQ_REMAINDER_RATIO ? x * (1.0 - a) : x - a;
    }
    adjusted[idx] = r;
}

bool shape_ok(int64_t n, int F, int64_t S)
{
    return n >= 0 && n < (1ll << 31) && F >= 1 && F <= FSQ_REMAINDER_MAX_FRAMES && S >= 0 && S * (int64_t)F < (1ll << 31);
}

}  // namespace

extern "C" int64_t fsq_remainder_workspace_bytes(int64_t n_tracks, int n_frames, int64_t n_segments)
{
    if (!shape_ok(n_tracks, n_frames, n_segments)) return FSQ_EINVAL;
    return 8 + n_tracks * (int64_t)n_frames * (int64_t)sizeof(double) + n_tracks * (int64_t)sizeof(int);
}

extern "C" int fsq_remainder_adjust(const double* intensity, const uint64_t* category, const int64_t* seg_off, int64_t n, int F,
                                    int64_t S, const FsqRemainderParams* prm, double* adjustment, int32_t* n_remainders,
                                    uint8_t* kept, double* adjusted, void* ws, int64_t ws_bytes, void* stream_)
{
    if (F > FSQ_REMAINDER_MAX_FRAMES) return FSQ_ENOTIMPL;
    if (!shape_ok(n, F, S) || !prm || !seg_off) return FSQ_EINVAL;
    if (prm->mode != FSQ_REMAINDER_RATIO && prm->mode != FSQ_REMAINDER_ADDITIVE) return FSQ_EINVAL;
    if (n > 0 && (!intensity || !category || !adjusted)) return FSQ_EINVAL;
    if (S > 0 && (!adjustment || !n_remainders || !kept)) return FSQ_EINVAL;
    if (!ws || ((uintptr_t)ws & 7) || ws_bytes < fsq_remainder_workspace_bytes(n, F, S)) return FSQ_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    double* ws_values = (double*)ws;
    int* ws_segment = (int*)(ws_values + n * F);
    const int mode = prm->mode;
    if (S > 0) FSQ_HIP_CHECK(hipMemsetAsync(n_remainders, 0, (size_t)S * sizeof(int32_t), stream));
    if (n > 0) {
        hipLaunchKernelGGL(krm_tracks, dim3((unsigned)((n + TRACKS_PER_BLOCK - 1) / TRACKS_PER_BLOCK)), dim3(THREADS), 0, stream,
                           intensity, (const u64*)category, (const long long*)seg_off, (long long)n, F, (long long)S, mode,
                           (int*)n_remainders, ws_values, ws_segment);
        FSQ_HIP_CHECK(hipGetLastError());
    }
    if (S > 0) {
        hipLaunchKernelGGL(krm_medians, dim3((unsigned)(S * F)), dim3(THREADS), 0, stream, (const double*)ws_values,
                           (const long long*)seg_off, (const int*)n_remainders, (long long)n, F, adjustment);
        FSQ_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(krm_finish, dim3((unsigned)((S + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream,
                           (const long long*)seg_off, (const int*)n_remainders, (long long)n, F, (long long)S, mode,
                           (int)prm->minimum_r_per_field, adjustment, (unsigned char*)kept);
        FSQ_HIP_CHECK(hipGetLastError());
    }
    if (n > 0) {
        const long long total = (long long)n * F;
        hipLaunchKernelGGL(krm_apply, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, intensity,
                           (const int*)ws_segment, (const double*)adjustment, (const unsigned char*)kept, total, F, mode, adjusted);
        FSQ_HIP_CHECK(hipGetLastError());
    }
    return FSQ_OK;
}
