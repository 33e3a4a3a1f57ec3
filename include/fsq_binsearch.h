/* fsq_binsearch.h - C ABI of the histogram bin search of the lognormal chain (libfsq_hip.so, gfx950).
 *
 * MCsimlib.optimal_bin_size (:3888-3909): Shimazaki & Shinomoto's cost of a histogram of nb equal bins over [lo, hi],
 * for many bin counts in one launch, with the bits of the reference's numpy calls (np.linspace, np.histogram with
 * explicit edges, np.mean, np.var).  Conventions are those of fsq_lognormal.h: every entry enqueues on `stream` and does
 * not synchronise, buffers are the caller's, return codes are those of include/fsq.h.
 *
 * The arithmetic, all in float64 with every product and sum rounded on its own (no fma); pow is glibc 2.35's (x86-64, FMA),
 * which the reference's `bin_size**2` on a numpy float64 scalar calls and which is not always the rounded product:
 *   step    = (hi - lo) / (double)nb
 *   edge[j] = (double)j * step + lo  (j < nb),  edge[nb] = hi
 *   rank[j] = #{x < edge[j]}         (j < nb),  rank[nb] = n        (the last bin is closed)
 *   hist[j] = rank[j + 1] - rank[j]
 *   mean    = (double)n / (double)nb
 *   var     = (0.0 + S) / (double)nb, S the sum of (hist[j] - mean)^2 in np.add.reduce's order: consecutive chunks of
 *             8192 elements, each summed pairwise (128-element leaves of 8 accumulators), the chunk sums added left to right
 *   cost    = (2.0 * mean - var) / pow(step, 2.0) */
#ifndef FSQ_BINSEARCH_H
#define FSQ_BINSEARCH_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Largest bin count.  One block holds the nb + 1 ranks of a bin count as int32 in LDS next to a pivot table of the data
 * (8 KiB) and 256 partial sums (2 KiB): 50 256 bytes as the compiler lays them out, of the 64 KiB a block may declare
 * statically, and the pairwise sum is laid out for at most two chunks of 8192 (nb <= 16384).  The reference's own widest
 * search (_get_m0Dm1) ends at 10000. */
#define FSQ_BINSEARCH_MAX_BINS 10000

/* d_cost[i] = the cost of d_bin_counts[i] bins, i < n_counts.
 *   d_sorted      double [n]         the data in ascending order, finite; 1 <= n < 2^31
 *   lo, hi        its first and last element; finite, hi > lo, hi - lo finite and (hi - lo) / FSQ_BINSEARCH_MAX_BINS > 0
 *   d_bin_counts  int32  [n_counts]  in any order, repeats allowed; each in 1 .. FSQ_BINSEARCH_MAX_BINS.  The array lives on
 *                                    the device, so the host cannot refuse a bad entry: its cost comes back as NaN and nothing
 *                                    else is touched.  1 <= n_counts < 2^31 (0: nothing is launched)
 *   d_cost        double [n_counts]
 * One block per bin count. */
int fsq_histogram_costs(const double* d_sorted, int64_t n, double lo, double hi, const int32_t* d_bin_counts, int n_counts,
                        double* d_cost, void* stream);

/* fsq_histogram_costs with lo = d_sorted[0] and hi = d_sorted[n - 1] read on the device, for a caller that has the data on
 * the device only and will not wait for it.  The host still refuses n and the pointers; what it would refuse of lo and hi
 * (see above) it cannot see, so the kernel checks them: then every cost comes back as NaN and nothing else is touched.  As an
 * ascending sort puts NaN last, that covers non-finite data and all-equal data too. */
int fsq_histogram_costs_sorted(const double* d_sorted, int64_t n, const int32_t* d_bin_counts, int n_counts, double* d_cost,
                               void* stream);

/* d_hist[j] = hist[j] of n_bins bins, j < n_bins: np.histogram(a, bins=np.linspace(lo, hi, n_bins + 1))[0].
 * Arguments as above; n_bins in 1 .. FSQ_BINSEARCH_MAX_BINS. */
int fsq_histogram_counts(const double* d_sorted, int64_t n, double lo, double hi, int n_bins, int64_t* d_hist, void* stream);

#ifdef __cplusplus
}
#endif
#endif
