// fsq_select_median.h - the exact np.median of R float64 values by one 256-thread block, shared by fsq_remainder.hip
// (krm_medians) and fsq_lognormal_chain.hip (kch_key_medians, kch_median_of_medians).  On the values' order-preserving 64-bit
// keys: up to FSQ_REMAINDER_LDS_MAX values sit in LDS and every thread ranks its own against all.  Above, a radix select of
// eight 8-bit passes over the values (a 256-bin LDS histogram of the keys that share the prefix found so far, then one wavefront
// scans it) finds the lower middle key and how many keys are at most it; where the upper middle is another key, a ninth pass
// takes the least key above.  A NaN among the values gives NaN; R <= 0 gives NaN.
#ifndef FSQ_SELECT_MEDIAN_H
#define FSQ_SELECT_MEDIAN_H
#include <hip/hip_runtime.h>

#include "../../../include/fsq_remainder.h"

namespace {

constexpr int SELECT_THREADS = 256;                                // the block select_median is called by
constexpr int SELECT_WAVE = 64;
constexpr int SELECT_LDS_MAX = FSQ_REMAINDER_LDS_MAX;
static_assert(SELECT_LDS_MAX % SELECT_THREADS == 0, "whole rounds of the block");

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

struct SelectShared {
    u64 key[SELECT_LDS_MAX];
    int hist[256];
    u64 pick[2];
    int digit, below, equal;
};

// *out = the median of v[0 .. R - 1].  Called by every thread of a SELECT_THREADS block with the same v, R and out (R is the
// block's: every exit is uniform over the block); `sh` is the block's.  v is only read.
__device__ __forceinline__ void select_median(const double* __restrict__ v, int R, double* __restrict__ out, SelectShared& sh)
{
    const int tid = threadIdx.x;
    if (R <= 0) {                                                  // (every exit below is uniform over the block)
        if (tid == 0) *out = __builtin_nan("");
        return;
    }
    const int k1 = (R - 1) / 2, k2 = R / 2;
    if (R <= SELECT_LDS_MAX) {
        int nan = 0;
        for (int e = tid; e < R; e += SELECT_THREADS) {
            const double x = v[e];
            nan |= x != x;
            sh.key[e] = key_of(x);
        }
        if (__syncthreads_or(nan)) {
            if (tid == 0) *out = __builtin_nan("");
            return;
        }
        for (int e = tid; e < R; e += SELECT_THREADS) {
            const u64 k = sh.key[e];
            int rank = 0;                                          // #{j : key_j < key_e, or equal and j < e}
            for (int j = 0; j < R; j++) {
                const u64 kj = sh.key[j];
                rank += (kj < k || (kj == k && j < e)) ? 1 : 0;
            }
            if (rank == k1) sh.pick[0] = k;
            if (rank == k2) sh.pick[1] = k;
        }
        __syncthreads();
        if (tid == 0) *out = middle_mean(value_of(sh.pick[0]), value_of(sh.pick[1]), R & 1);
        return;
    }
    // ---- radix select of the k1-th key, the most significant byte first ----
    u64 prefix = 0;
    int below = 0;                                                 // keys less than every key with this prefix
    for (int shift = 56; shift >= 0; shift -= 8) {
        sh.hist[tid] = 0;
        __syncthreads();
        int nan = 0;
        for (int e = tid; e < R; e += SELECT_THREADS) {
            const double x = v[e];
            nan |= x != x;
            const u64 k = key_of(x);
            if (shift == 56 || (k >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sh.hist[(int)((k >> shift) & 255)], 1);
        }
        if (__syncthreads_or(shift == 56 ? nan : 0)) {
            if (tid == 0) *out = __builtin_nan("");
            return;
        }
        if (tid < SELECT_WAVE) {                                   // lane l owns bins 4l .. 4l + 3
            int c[4], tot = 0;
#pragma unroll
            for (int q = 0; q < 4; q++) { c[q] = sh.hist[4 * tid + q]; tot += c[q]; }
            int incl = tot;
#pragma unroll
            for (int d = 1; d < SELECT_WAVE; d <<= 1) {
                const int up = __shfl_up(incl, d, SELECT_WAVE);
                if (tid >= d) incl += up;
            }
            int before = incl - tot;
            const int want = k1 - below;                           // 0 <= want < the keys with this prefix
            if (before <= want && want < incl) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (before <= want && want < before + c[q]) { sh.digit = 4 * tid + q; sh.below = before; sh.equal = c[q]; }
                    before += c[q];
                }
            }
        }
        __syncthreads();
        prefix |= (u64)sh.digit << shift;
        below += sh.below;
        __syncthreads();                                           // (sh.digit is read before the next pass writes it)
    }
    u64 upper = prefix;                                            // the k2-th key
    const int at_most = below + sh.equal;                          // #{key <= prefix}; sh.equal is the last pass's
    if (k2 >= at_most) {                                           // (uniform: below and sh.equal are the block's)
        if (tid == 0) sh.pick[0] = ~0ull;
        __syncthreads();
        u64 least = ~0ull;
        for (int e = tid; e < R; e += SELECT_THREADS) {
            const u64 k = key_of(v[e]);
            if (k > prefix && k < least) least = k;
        }
        atomicMin(&sh.pick[0], least);
        __syncthreads();
        upper = sh.pick[0];
    }
    if (tid == 0) *out = middle_mean(value_of(prefix), value_of(upper), R & 1);
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

// where segment s's tracks start and how many they are, and `count` clamped to that: 0 for a segment that is not well formed
__device__ __forceinline__ int clamped_count(const long long* __restrict__ seg_off, long long n, long long s, long long count,
                                             long long* off, long long* cap)
{
    const long long o = seg_off[s], e = seg_off[s + 1];
    *off = 0;
    *cap = 0;
    if (o < 0 || e > n || e < o) return 0;
    *off = o;
    *cap = e - o;
    return (int)(count < e - o ? count : e - o);
}

}  // namespace
#endif
