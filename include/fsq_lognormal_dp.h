/* fsq_lognormal_dp.h - C ABI of the lognormal fluor-count fit by exact dynamic programme (libfsq_hip.so, gfx950).
 *
 * The same winner as the enumerating fit of include/fsq_lognormal.h - MCsimlib._intensities_to_signal_lognormal_v8
 * (:5387-5466): the first sequence in the reference's order (largest count first) whose left-to-right product of per-frame
 * densities is strictly the greatest - found in O(max_frames * max_possible^2) per track without enumerating a sequence.
 * So no track is over a budget, and allow_upsteps (the reference's itertools.product, (max_possible + 1)^T sequences) is
 * served as well.
 *
 * Why it is exact.  The total is a left-to-right product of non-negative doubles, and IEEE multiplication by a
 * non-negative factor is monotone: a >= b >= 0 and s >= 0 give fl(a * s) >= fl(b * s).
 *   forward   P[f][v], the greatest rounded prefix product over the admissible prefixes that end with count v at frame f,
 *             obeys P[f][v] = fl(max_u P[f-1][u] * S[f][v]) over the counts u that v may follow; B = max_v P[T-1][v] is the
 *             reference's best_score, bit for bit.
 *   backward  the best total a prefix ending in (f, v) with product p can still reach is non-decreasing in p, so "can
 *             reach B" is p >= N[f][v] for one threshold per (f, v): N[T-1][v] = B, N[f][u] = min over allowed v of
 *             Q[f+1][v], where Q[f][v] is the least double p >= 0 with fl(p * S[f][v]) >= N[f][v] (0 where N <= 0, +inf
 *             where no finite p does it).  Q is found exactly: non-negative doubles are ordered like their bit patterns,
 *             so N / S and its two neighbours are tried and a search over the bit pattern (at most 63 multiplications) is
 *             the fallback.
 *   winner    from p = 1, at each frame the largest allowed count v with fl(p * S[f][v]) >= N[f][v]: the first sequence in
 *             lexicographic order, largest count first, whose total is B - the reference's strict `>` in the order of
 *             combinations_with_replacement and of product alike.
 * v may follow u when v <= u (any v with allow_upsteps), and without multi-drop in addition u - v <= 1.
 *
 * Refused (FSQ_EINVAL, before any launch): a density above 1 whose product over max_frames frames could overflow.  With
 * peak = 1 / (sqrt(2 pi) * beta_sigma), the greatest density, the call is refused when
 *     peak > 1  and  max_frames * log(peak) >= 700.
 * Below that no prefix product reaches inf, so inf * 0 = NaN cannot arise and the monotonicity above holds.  It is a
 * condition on the parameters, not a measurement of the data.
 *
 * Conventions are those of fsq_lognormal.h. */
#ifndef FSQ_LOGNORMAL_DP_H
#define FSQ_LOGNORMAL_DP_H
#include "fsq_lognormal.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace fsq_lognormal_fit_dp needs (0: none), -1 for an invalid shape. */
int64_t fsq_lognormal_dp_workspace_bytes(int64_t n_tracks, int32_t max_frames);

/* The fit of n_tracks ragged tracks, one wavefront per track.  Arguments as fsq_lognormal_fit, and
 *   allow_upsteps  0: counts never rise (combinations_with_replacement); else any count may follow any (product)
 * prm->budget is ignored.  d_status is FSQ_LOGNORMAL_FOUND, _NONE or _INVALID, never _OVER_BUDGET.  d_n_surviving is the
 * exact number of sequences that pass the category, multi-drop and deviation rules under the mode's transition rule,
 * saturating at FSQ_LOGNORMAL_MAX_BUDGET; a saturated count does not change the status.  Every element of every output
 * row is written, with fsq_lognormal_fit's padding: frames beyond n_frames and tracks without a winner get count 0, frame
 * score 0 and best score -1. */
int fsq_lognormal_fit_dp(const double* d_intensity, const uint64_t* d_category, const int32_t* d_n_frames, int64_t n_tracks,
                         int32_t max_frames, const FsqLognormalParams* prm, int32_t* d_status, uint8_t* d_best_seq,
                         double* d_best_score, double* d_frame_score, int64_t* d_n_surviving, int32_t allow_upsteps,
                         void* d_ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
