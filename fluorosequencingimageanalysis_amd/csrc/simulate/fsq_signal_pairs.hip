// fsq_signal_pairs.hip - match_diagnostic's incompatibility loop over signal pairs (jupyter_development.py:838-889), the C ABI
// of include/fsq_signal_sweep.h's fsq_signal_pair_best and fsq_signal_pair_extremes.
//
//   kpr_pair_best      one wavefront per pair (i, j) of candidate signals, lanes strided over the points: each lane scores its
//                      points with fsq_score_term.h - kss_scores' arithmetic over the two keys - and keeps its best as
//                      (result, point); the wavefront then reduces (result, point) lexicographically, so the lowest point wins
//                      among equal results whatever the reduction's shape, and the lane that owns the winning point writes
//                      the factor and the two distances it kept.  The two rows of d_fit are read coalesced.
//   kpr_pair_extremes  one wavefront per candidate: its n_sel - 1 distances through the closed-form pair index, reduced to a
//                      maximum or a minimum with NaN skipped.
// No atomics, no lane reads another lane's store, every loop is bounded by n_points or n_sel.
#include <vector>

#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_signal_sweep.h"
#include "../libm/fsq_glibc_log.h"
#include "../libm/fsq_glibc_pow.h"
#include "fsq_score_term.h"

namespace {

constexpr int WAVE = 64;
constexpr int PAIR_WAVES = 4;                   // pairs of a block
constexpr int NO_POINT = 0x7fffffff;

// the first pair of candidate i: i (2 n - i - 1) / 2
__device__ __forceinline__ int pair_offset(const int i, const int n) { return (int)(((long long)i * (2 * n - i - 1)) / 2); }

// (i, j) of pair t: the root of i^2 - (2 n - 1) i + 2 t = 0 in fp64 (exact to well within one for n <= 2048), then at most
// two steps either way
__device__ __forceinline__ void pair_of_index(const int t, const int n, int* pi, int* pj)
{
    const double b = (double)(2 * n - 1);
    int i = (int)((b - sqrt(b * b - 8.0 * (double)t)) * 0.5);
    i = i < 0 ? 0 : i > n - 2 ? n - 2 : i;
    for (int s = 0; s < 2; ++s)
        if (i > 0 && pair_offset(i, n) > t) --i;
    for (int s = 0; s < 2; ++s)
        if (i < n - 2 && pair_offset(i + 1, n) <= t) ++i;
    *pi = i;
    *pj = t - pair_offset(i, n) + i + 1;
}

// a is better than b: (result, point) in lexicographic order; a point of NO_POINT has no result
__device__ __forceinline__ bool better(const double ra, const int ka, const double rb, const int kb, const bool reverse)
{
    if (ka == NO_POINT) return false;
    if (kb == NO_POINT) return true;
    if (ra != rb) return reverse ? ra > rb : ra < rb;
    return ka < kb;
}

__global__ void __launch_bounds__(WAVE * PAIR_WAVES)
kpr_pair_best(const long long* __restrict__ g_obs, const uint8_t* __restrict__ g_in_obs, const uint8_t* __restrict__ g_admitted,
              const long long* __restrict__ g_fit, const long long* __restrict__ g_fit_total, const int P, const FsqScoreParams prm,
              const int32_t* __restrict__ g_rows, const int n_sel, const int K, const bool reverse,
              const double* __restrict__ g_heat_factor, const int32_t* __restrict__ g_heat_status, int32_t* __restrict__ g_best_point,
              double* __restrict__ g_result, double* __restrict__ g_factor, double* __restrict__ g_dist,
              int32_t* __restrict__ g_error_point, int32_t* __restrict__ g_error_status)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int t = blockIdx.x * PAIR_WAVES + (threadIdx.x >> 6);                     // the wavefront's pair
    if (t >= K) return;
    const double nan = __builtin_nan("");
    const int metric = prm.metric;
    int row[2];
    pair_of_index(t, n_sel, &row[0], &row[1]);
    row[0] = g_rows[row[0]];
    row[1] = g_rows[row[1]];
    long long obs[2];
    bool adm[2], in_obs[2];
    for (int m = 0; m < 2; ++m) {
        const bool any = row[m] >= 0;
        obs[m] = any ? g_obs[row[m]] : 0;
        adm[m] = any && g_admitted[row[m]];
        in_obs[m] = any && g_in_obs[row[m]];
    }
    const long long n_obs = prm.n_observed;

    double best_r = 0.0, best_f = nan, best_d0 = nan, best_d1 = nan;
    int best_k = NO_POINT, err_k = NO_POINT, err_s = 0;
    for (int k = lane; k < P; k += WAVE) {
        long long fit[2];
        bool pr[2];
        long long sum_o = 0, sum_f = 0;
        int n_paired = 0;
        for (int m = 0; m < 2; ++m) {
            fit[m] = adm[m] ? g_fit[(long long)row[m] * P + k] : 0;
            pr[m] = score_paired(prm, adm[m], in_obs[m], obs[m], fit[m]);
            if (pr[m]) { sum_o += obs[m]; sum_f += fit[m]; ++n_paired; }
        }
        // the factor (:331-358), as kss_scores takes it
        double factor = 1.0;
        int status = FSQ_SCORE_OK;
        if ((prm.normalization & FSQ_SCORE_NORMALIZE_COUNTS) && n_paired > 0 && sum_f > 0) {
            factor = (double)sum_o / (double)sum_f;
        } else if (prm.normalization & FSQ_SCORE_HEATMAP_NORMALIZE_COUNTS) {
            if (g_heat_status[k] == FSQ_SCORE_DIVZERO) status = FSQ_SCORE_DIVZERO;
            else factor = g_heat_factor[k];
        }
        double result = 0.0, d[2] = {nan, nan};
        if (status == FSQ_SCORE_OK && n_paired == 0) status = FSQ_SCORE_EMPTY;
        if (status == FSQ_SCORE_OK) {
            const long long n_fit = g_fit_total[k];
            double acc = 0.0;
            int n_contrib = 0;
            bool divzero = false, domain = false;
            for (int m = 0; m < 2; ++m) {
                if (!pr[m]) continue;
                const ScoreTerm term = score_term(metric, obs[m], fit[m], factor, n_obs, n_fit);
                divzero |= term.divzero;
                domain |= term.domain;
                if (!term.have) continue;
                ++n_contrib;
                d[m] = term.c;
                acc = score_accumulate(acc, term);
            }
            if (domain || divzero) status = domain ? FSQ_SCORE_DOMAIN : FSQ_SCORE_DIVZERO;
            else if (!score_result(metric, acc, n_contrib, &result)) status = FSQ_SCORE_DOMAIN;
        }
        if (status == FSQ_SCORE_OK) {
            if (better(result, k, best_r, best_k, reverse)) { best_r = result; best_k = k; best_f = factor; best_d0 = d[0]; best_d1 = d[1]; }
        } else if (status != FSQ_SCORE_EMPTY && err_k == NO_POINT) {
            err_k = k;                                                              // (k ascends: the lane's lowest)
            err_s = status;
        }
    }
    // the wavefront's best (result, point) and lowest error point: every lane ends with both
    double all_r = best_r;
    int all_k = best_k, all_e = err_k;
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const double r = __shfl_xor(all_r, off, WAVE);
        const int k = __shfl_xor(all_k, off, WAVE), e = __shfl_xor(all_e, off, WAVE);
        if (better(r, k, all_r, all_k, reverse)) { all_r = r; all_k = k; }
        all_e = e < all_e ? e : all_e;
    }
    // the winning point is its own lane's best: that lane kept the factor and the distances
    if (all_k == NO_POINT) {
        if (lane == 0) {
            g_best_point[t] = -1;
            g_result[t] = nan;
            g_factor[t] = nan;
            g_dist[2 * t] = nan;
            g_dist[2 * t + 1] = nan;
        }
    } else if (all_k == best_k) {
        g_best_point[t] = best_k;
        g_result[t] = best_r;
        g_factor[t] = best_f;
        g_dist[2 * t] = best_d0;
        g_dist[2 * t + 1] = best_d1;
    }
    if (all_e == NO_POINT) {
        if (lane == 0) { g_error_point[t] = -1; g_error_status[t] = 0; }
    } else if (all_e == err_k) {
        g_error_point[t] = err_k;
        g_error_status[t] = err_s;
    }
}

__global__ void __launch_bounds__(WAVE)
kpr_pair_extremes(const double* __restrict__ g_dist, const int n_sel, const bool reverse, double* __restrict__ g_score,
                  int32_t* __restrict__ g_n)
{
    const int s = blockIdx.x, lane = threadIdx.x;
    double ext = __builtin_nan("");
    int n = 0;
    for (int o = lane; o < n_sel; o += WAVE) {
        if (o == s) continue;
        const int i = o < s ? o : s, j = o < s ? s : o;
        const double d = g_dist[2 * (pair_offset(i, n_sel) + j - i - 1) + (o < s ? 1 : 0)];
        if (d != d) continue;
        ++n;
        if (ext != ext || (reverse ? d < ext : d > ext)) ext = d;
    }
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const double d = __shfl_xor(ext, off, WAVE);
        n += __shfl_xor(n, off, WAVE);
        if (d == d && (ext != ext || (reverse ? d < ext : d > ext))) ext = d;
    }
    if (lane == 0) {
        g_score[s] = ext;
        g_n[s] = n;
    }
}

bool sel_ok(int32_t n_sel) { return n_sel >= 2 && n_sel <= FSQ_SIGNAL_PAIR_MAX_SEL; }

}  // namespace

extern "C" int fsq_signal_pair_best(const int64_t* d_observed, const uint8_t* d_in_observed, const uint8_t* d_admitted,
                                    const int64_t* d_fit, const int64_t* d_fit_total, int32_t n_keys, int32_t n_points,
                                    const FsqScoreParams* prm, const int32_t* d_rows, int32_t n_sel, int32_t reverse_order,
                                    const double* d_heat_factor, const int32_t* d_heat_status, int32_t* d_best_point, double* d_result,
                                    double* d_factor, double* d_dist, int32_t* d_error_point, int32_t* d_error_status, void* stream)
{
    if (!prm || n_keys < 0 || n_points < 1 || !sel_ok(n_sel)) return FSQ_EINVAL;
    if (prm->metric < 0 || prm->metric >= FSQ_SCORE_N_METRICS || (prm->normalization & ~3)) return FSQ_EINVAL;
    if (prm->n_observed < 0 || prm->n_observed > 2147483647ll) return FSQ_EINVAL;
    if (prm->has_cutoff && prm->small_count_cutoff != prm->small_count_cutoff) return FSQ_EINVAL;
    if (!d_fit_total || !d_rows || !d_best_point || !d_result || !d_factor || !d_dist || !d_error_point || !d_error_status) return FSQ_EINVAL;
    if (n_keys > 0 && (!d_observed || !d_in_observed || !d_admitted || !d_fit)) return FSQ_EINVAL;
    if ((prm->normalization & FSQ_SCORE_HEATMAP_NORMALIZE_COUNTS) && (!d_heat_factor || !d_heat_status)) return FSQ_EINVAL;
    // the rows index d_fit: they are checked here, where a bad one can still be refused
    std::vector<int32_t> rows((size_t)n_sel);
    FSQ_HIP_CHECK(hipMemcpyAsync(rows.data(), d_rows, sizeof(int32_t) * (size_t)n_sel, hipMemcpyDeviceToHost, (hipStream_t)stream));
    FSQ_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    for (int32_t r : rows)
        if (r < -1 || r >= n_keys) return FSQ_EINVAL;
    const int K = n_sel * (n_sel - 1) / 2;
    hipLaunchKernelGGL(kpr_pair_best, dim3((unsigned)((K + PAIR_WAVES - 1) / PAIR_WAVES)), dim3(WAVE * PAIR_WAVES), 0, (hipStream_t)stream,
                       (const long long*)d_observed, d_in_observed, d_admitted, (const long long*)d_fit, (const long long*)d_fit_total,
                       (int)n_points, *prm, d_rows, (int)n_sel, K, reverse_order != 0, d_heat_factor, d_heat_status, d_best_point,
                       d_result, d_factor, d_dist, d_error_point, d_error_status);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_signal_pair_extremes(const double* d_dist, int32_t n_sel, int32_t reverse_order, double* d_score,
                                        int32_t* d_n_distances, void* stream)
{
    if (!sel_ok(n_sel) || !d_dist || !d_score || !d_n_distances) return FSQ_EINVAL;
    hipLaunchKernelGGL(kpr_pair_extremes, dim3((unsigned)n_sel), dim3(WAVE), 0, (hipStream_t)stream, d_dist, (int)n_sel,
                       reverse_order != 0, d_score, d_n_distances);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
