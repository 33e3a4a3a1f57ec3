// fsq_binsearch.hip - the histogram bin search of the lognormal chain (include/fsq_binsearch.h): Shimazaki & Shinomoto's
// cost of np.histogram(a, bins=np.linspace(lo, hi, nb + 1)) for many bin counts nb in one launch, with numpy's bits.
//
// kbs_costs, one 256-thread block per bin count:
//   1. a pivot table of the sorted data (every S-th element, at most 1024) goes into LDS;
//   2. the threads stride over the nb + 1 edges; each edge is two roundings ((double)j * step, + lo) and one lower bound:
//      10 steps in the pivot table, then log2(S) dependent global loads inside one stride.  The ranks stay in LDS as int32;
//   3. np.add.reduce's order without recursion: thread t owns slot t & 127 of a depth-7 binary tree over chunk t >> 7 (8192
//      elements).  It walks numpy's splits (n2 = n / 2, n2 -= n2 % 8) along the bits of its slot until at most 128 elements
//      are left; the thread whose remaining bits are zero owns that leaf and sums it with numpy's 8 accumulators straight
//      from the ranks.  Seven barrier-separated steps then add each right child to its left sibling, deepest level first;
//   4. thread 0 adds the chunk sums left to right and writes the cost; its divisor is glibc's pow(step, 2.0)
//      (libm/fsq_glibc_pow.h), which is what the reference's `bin_size**2` on a numpy scalar calls.
// Every LDS index is below nb + 1 <= FSQ_BINSEARCH_MAX_BINS + 1 and every global index below n; a bin count outside
// 1 .. FSQ_BINSEARCH_MAX_BINS leaves NaN and touches nothing else.
// kbs_costs<true> (fsq_histogram_costs_sorted) reads lo and hi from sorted[0] and sorted[n - 1] instead of taking them from
// the host, and applies the host's refusals to them itself: bounds the host would refuse leave NaN in every cost.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../libm/fsq_glibc_pow.h"
#include "../stepfit/fsq_pairwise.h"
#include "../../../include/fsq_binsearch.h"

namespace {

constexpr int THREADS = 256;
constexpr int PIVOTS = 1024;
constexpr int CHUNK = 8192;                 // np.add.reduce sums a long array in chunks of this many elements
constexpr int TREE_DEPTH = 7;               // splits of one chunk down to leaves of at most 128 (fsq_pairwise.h)
constexpr int SLOTS = 1 << TREE_DEPTH;
static_assert(FSQ_BINSEARCH_MAX_BINS <= (THREADS / SLOTS) * CHUNK, "one slot tree per chunk");
static_assert(sizeof(int) * (FSQ_BINSEARCH_MAX_BINS + 1) + sizeof(double) * (PIVOTS + THREADS) <= 64 * 1024, "static LDS");

// np.linspace's edge j < nb: two roundings, never an fma
__device__ __forceinline__ double edge_of(int j, double step, double lo)
{
    return __dadd_rn(__dmul_rn((double)j, step), lo);
}

// #{i in [first, last) : a[i] < e} + first, a ascending: np.searchsorted(a, e, 'left')
__device__ __forceinline__ long long lower_bound(const double* a, long long first, long long last, double e)
{
    while (first < last) {
        const long long mid = first + ((last - first) >> 1);
        if (a[mid] < e) first = mid + 1; else last = mid;
    }
    return first;
}

// what the host refuses of a pair of bounds: hi <= lo, a non-finite bound or span, a span whose smallest step underflows to 0
__host__ __device__ __forceinline__ bool bounds_ok(double lo, double hi)
{
    if (!isfinite(lo) || !isfinite(hi) || !(hi > lo)) return false;
    const double span = hi - lo;
    return isfinite(span) && span / (double)FSQ_BINSEARCH_MAX_BINS > 0.0;
}

template <bool BOUNDS_FROM_DATA>
__global__ void __launch_bounds__(THREADS)
kbs_costs(const double* __restrict__ sorted, long long n, double lo, double hi, const int* __restrict__ bin_counts, int n_counts,
          double* __restrict__ cost)
{
    __shared__ int s_rank[FSQ_BINSEARCH_MAX_BINS + 1];
    __shared__ double s_pivot[PIVOTS];
    __shared__ double s_val[THREADS];
    const int tid = threadIdx.x;
    const int which = n_counts - 1 - (int)blockIdx.x;              // an ascending array: the largest counts start first
    const int nb = bin_counts[which];
    if (BOUNDS_FROM_DATA) { lo = sorted[0]; hi = sorted[n - 1]; }  // (ascending: the least and the greatest, a NaN last)
    if (nb < 1 || nb > FSQ_BINSEARCH_MAX_BINS || (BOUNDS_FROM_DATA && !bounds_ok(lo, hi))) {   // (uniform over the block, before any barrier)
        if (tid == 0) cost[which] = __builtin_nan("");
        return;
    }
    // ---- 1. pivots: s_pivot[k] = sorted[k * S], k < np <= PIVOTS ----
    const long long S = (n + PIVOTS - 1) / PIVOTS;
    const int np = (int)((n + S - 1) / S);
    for (int k = tid; k < np; k += THREADS) s_pivot[k] = sorted[k * S];
    __syncthreads();
    // ---- 2. ranks ----
    const double step = (hi - lo) / (double)nb;
    for (int j = tid; j <= nb; j += THREADS) {
        long long r = n;                                           // the last edge is hi and its bin is closed
        if (j < nb) {
            const double e = edge_of(j, step, lo);
            int a = 0, b = np;                                     // c = #{k : s_pivot[k] < e}
            while (a < b) {
                const int mid = (a + b) >> 1;
                if (s_pivot[mid] < e) a = mid + 1; else b = mid;
            }
            if (a == 0) {
                r = 0;
            } else {                                               // sorted[(a - 1) * S] < e, and a == np or sorted[a * S] >= e
                const long long last = (long long)a * S < n ? (long long)a * S : n;
                r = lower_bound(sorted, (long long)(a - 1) * S + 1, last, e);
            }
        }
        s_rank[j] = (int)r;
    }
    __syncthreads();
    // ---- 3. the sum of squared deviations in np.add.reduce's order ----
    const double mean = (double)n / (double)nb;
    const int slot = tid & (SLOTS - 1);
    int off = (tid / SLOTS) * CHUNK;
    int len = nb - off < CHUNK ? nb - off : CHUNK;                 // <= 0: this chunk does not exist
    unsigned internal = 0;                                         // bit d: the node of depth d on this slot's path is split
    int d = 0;
    for (; d < TREE_DEPTH && len > 128; d++) {
        internal |= 1u << d;
        int n2 = len / 2;
        n2 -= n2 % 8;
        if ((slot >> (TREE_DEPTH - 1 - d)) & 1) { off += n2; len -= n2; } else { len = n2; }
    }
    double v = 0.0;
    if (len > 0 && (slot & ((1 << (TREE_DEPTH - d)) - 1)) == 0)
        v = pw_leaf([mean](int j) {
                const double dev = (double)(s_rank[j + 1] - s_rank[j]) - mean;
                return __dmul_rn(dev, dev);
            }, off, len);
    s_val[tid] = v;
    for (int lvl = TREE_DEPTH - 1; lvl >= 0; lvl--) {
        __syncthreads();
        if (((internal >> lvl) & 1u) && (slot & ((1 << (TREE_DEPTH - lvl)) - 1)) == 0)
            s_val[tid] = s_val[tid] + s_val[tid + (1 << (TREE_DEPTH - 1 - lvl))];
    }
    __syncthreads();
    // ---- 4. the cost ----
    if (tid == 0) {
        double sum = 0.0;                                          // np.add.reduce starts from the identity
        for (int c = 0; c * CHUNK < nb; c++) sum = sum + s_val[c * SLOTS];
        const double var = sum / (double)nb;
        // bin_size ** 2 of a numpy float64 scalar is libm's pow(bin_size, 2.0): within an ulp of, not always equal to, the product
        cost[which] = __dsub_rn(__dmul_rn(2.0, mean), var) / sf_pow<2, true>(step);
    }
}

__global__ void __launch_bounds__(THREADS)
kbs_counts(const double* __restrict__ sorted, long long n, double lo, double hi, int nb, long long* __restrict__ hist)
{
    const int j = (int)(blockIdx.x * THREADS + threadIdx.x);
    if (j >= nb) return;
    const double step = (hi - lo) / (double)nb;
    const long long r0 = lower_bound(sorted, 0, n, edge_of(j, step, lo));
    const long long r1 = j + 1 < nb ? lower_bound(sorted, 0, n, edge_of(j + 1, step, lo)) : n;
    hist[j] = r1 - r0;
}

bool range_ok(int64_t n, double lo, double hi)
{
    return n >= 1 && n < (1ll << 31) && bounds_ok(lo, hi);
}

}  // namespace

extern "C" int fsq_histogram_costs(const double* d_sorted, int64_t n, double lo, double hi, const int32_t* d_bin_counts,
                                   int n_counts, double* d_cost, void* stream)
{
    if (!range_ok(n, lo, hi) || n_counts < 0) return FSQ_EINVAL;
    if (n_counts == 0) return FSQ_OK;
    if (!d_sorted || !d_bin_counts || !d_cost) return FSQ_EINVAL;
    hipLaunchKernelGGL(kbs_costs<false>, dim3((unsigned)n_counts), dim3(THREADS), 0, (hipStream_t)stream, d_sorted, (long long)n,
                       lo, hi, (const int*)d_bin_counts, n_counts, d_cost);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_histogram_costs_sorted(const double* d_sorted, int64_t n, const int32_t* d_bin_counts, int n_counts,
                                          double* d_cost, void* stream)
{
    if (n < 1 || n >= (1ll << 31) || n_counts < 0) return FSQ_EINVAL;
    if (n_counts == 0) return FSQ_OK;
    if (!d_sorted || !d_bin_counts || !d_cost) return FSQ_EINVAL;
    hipLaunchKernelGGL(kbs_costs<true>, dim3((unsigned)n_counts), dim3(THREADS), 0, (hipStream_t)stream, d_sorted, (long long)n,
                       0.0, 0.0, (const int*)d_bin_counts, n_counts, d_cost);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_histogram_counts(const double* d_sorted, int64_t n, double lo, double hi, int n_bins, int64_t* d_hist,
                                    void* stream)
{
    if (!range_ok(n, lo, hi) || n_bins < 1 || n_bins > FSQ_BINSEARCH_MAX_BINS) return FSQ_EINVAL;
    if (!d_sorted || !d_hist) return FSQ_EINVAL;
    hipLaunchKernelGGL(kbs_counts, dim3((unsigned)((n_bins + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream,
                       d_sorted, (long long)n, lo, hi, n_bins, (long long*)d_hist);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
