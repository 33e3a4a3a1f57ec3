// fsq_score_term.h - the arithmetic of one term of signal_correlation (jupyter_development.py:279-578), shared by kss_scores
// (fsq_signal_sweep.hip: every admitted key of a point) and kss_pair_best (fsq_signal_pairs.hip: two keys of a point), so
// that a pair's result has fsq_signal_scores' bits by construction.  The including file brings fsq_devmath.h, the libm
// restatements and include/fsq_signal_sweep.h.
#pragma once

// A key is paired for a point when it is admitted, stands in the observed dict or the point's fit dict, and passes the cutoff
// (:288-326).
__device__ __forceinline__ bool score_paired(const FsqScoreParams& prm, const bool admitted, const bool in_obs, const long long o,
                                             const long long f)
{
    if (!admitted || !(in_obs || f > 0)) return false;
    return !prm.has_cutoff || ((double)o >= prm.small_count_cutoff && (double)f >= prm.small_count_cutoff);
}

struct ScoreTerm {
    double c;                       // the contribution, read when have
    bool have;                      // the metric takes the key (not: observed == 0 in the two `normalized` metrics, an error)
    bool is_max;                    // the metric is a maximum of its terms, not a sum
    bool divzero, domain;           // the reference raises ZeroDivisionError / ValueError at this key
};

// The contribution of a paired key with observed count oi and fit count fi under `factor` (:364-503).
__device__ __forceinline__ ScoreTerm score_term(const int metric, const long long oi, const long long fi, const double factor,
                                                const long long n_obs, const long long n_fit)
{
    const double o = (double)oi, f = (double)fi * factor;
    ScoreTerm t = {0.0, true, false, false, false};
    switch (metric) {
    case FSQ_SCORE_NAIVE:
        t.c = o * f;
        break;
    case FSQ_SCORE_MY_EUCLIDEAN:
        t.c = sf_pow<2, true>(f - o);
        break;
    case FSQ_SCORE_NORMALIZED_EUCLIDEAN:
        if (oi > 0) t.c = sf_pow<2, true>((f - o) / o);
        else t.have = false;
        break;
    case FSQ_SCORE_MY_STD_NORMALIZED_EUCLIDEAN:
    case FSQ_SCORE_MY_STD_NORMALIZED_CHEBYSHEV: {
        double sd = 1.0;
        if (oi > 0) {
            if (n_obs == 0) { t.divzero = true; t.have = false; break; }
            const double v = (double)(oi * (n_obs - oi)) / (double)n_obs;
            if (v < 0.0) { t.domain = true; t.have = false; break; }
            sd = sqrt(v);
        }
        if (sd == 0.0) { t.divzero = true; t.have = false; break; }
        if (metric == FSQ_SCORE_MY_STD_NORMALIZED_EUCLIDEAN) t.c = sf_pow<2, true>((f - o) / sd);
        else { t.c = fabs(o - f) / sd; t.is_max = true; }
        break;
    }
    case FSQ_SCORE_MY_SIM_STD_NORMALIZED_EUCLIDEAN: {
        double sd = 1.0;
        if (f > 0.0) {
            const double v = f * ((double)n_fit - f) / (double)n_fit;
            if (v < 0.0) { t.domain = true; t.have = false; break; }
            sd = sqrt(v);
        }
        if (sd == 0.0) { t.divzero = true; t.have = false; break; }
        t.c = sf_pow<2, true>((f - o) / sd);
        break;
    }
    case FSQ_SCORE_LOG_RMSD:
        t.c = sf_pow<2, true>(ln_log((double)(oi + 1)) - ln_log(f + 1.0));
        break;
    case FSQ_SCORE_MY_CANBERRA: {
        const double den = fabs(o) + fabs(f);
        if (den == 0.0) { t.divzero = true; t.have = false; break; }
        t.c = fabs(o - f) / den;
        break;
    }
    case FSQ_SCORE_MY_CHEBYSHEV:
        t.c = fabs(o - f);
        t.is_max = true;
        break;
    default:                                                                        // FSQ_SCORE_MY_NORMALIZED_CHEBYSHEV
        if (oi > 0) { t.c = fabs(o - f) / o; t.is_max = true; }
        else t.have = false;
        break;
    }
    return t;
}

// acc with one more term
__device__ __forceinline__ double score_accumulate(const double acc, const ScoreTerm& t)
{
    if (t.is_max) return t.c > acc ? t.c : acc;
    return acc + t.c;
}

// The result of n_contrib accumulated terms; false: the reference raises ValueError (a maximum of nothing).
__device__ __forceinline__ bool score_result(const int metric, const double acc, const int n_contrib, double* result)
{
    switch (metric) {
    case FSQ_SCORE_NAIVE:
    case FSQ_SCORE_MY_CANBERRA:
    case FSQ_SCORE_MY_CHEBYSHEV:
    case FSQ_SCORE_MY_STD_NORMALIZED_CHEBYSHEV:
        *result = acc;
        return true;
    case FSQ_SCORE_MY_NORMALIZED_CHEBYSHEV:
        if (n_contrib == 0) return false;
        *result = acc;
        return true;
    case FSQ_SCORE_LOG_RMSD:
        *result = sqrt(acc / (double)n_contrib);
        return true;
    default:
        *result = sqrt(acc);
        return true;
    }
}
