/* fsq_lognormal.h - C ABI of the lognormal fluor-count fit of track photometries (libfsq_hip.so, gfx950).
 *
 * MCsimlib._intensities_to_signal_lognormal_v8 (:5387-5466, allow_upsteps=False) for a batch of tracks: of all
 * non-increasing fluor-count sequences over max_possible .. 0, the first one in the reference's order (largest count
 * first) whose product of per-frame normal densities of log(intensity) is strictly the greatest.  Conventions are those
 * of fsq_chisq.h: every entry enqueues on `stream` and does not synchronise, buffers are the caller's, rows are
 * [n_tracks][max_frames], return codes are those of include/fsq.h. */
#ifndef FSQ_LOGNORMAL_H
#define FSQ_LOGNORMAL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_LOGNORMAL_MAX_FRAMES 64         /* frames of one track: one bit each in the category word */
#define FSQ_LOGNORMAL_MAX_POSSIBLE 15       /* largest fluor count */
#define FSQ_LOGNORMAL_MAX_BUDGET (1ll << 59) /* counts saturate here */
#define FSQ_LOGNORMAL_DEFAULT_BUDGET (1ll << 22)

#define FSQ_LOGNORMAL_FOUND 0               /* best_seq / best_score / frame_score hold the winner */
#define FSQ_LOGNORMAL_NONE 1                /* no sequence passes the rules (the reference's best_seq is None) */
#define FSQ_LOGNORMAL_OVER_BUDGET 2         /* more surviving sequences than `budget`, or a saturated count: counted, not enumerated */
#define FSQ_LOGNORMAL_INVALID 3             /* n_frames < 1 or > max_frames */

typedef struct {
    double log_fluor_means[FSQ_LOGNORMAL_MAX_POSSIBLE + 2];   /* [v - 1] is the mean of log(intensity) at count v; max_possible + 2 given, as in the reference */
    double beta_sigma;                      /* finite, > 0 */
    double max_deviation;                   /* in units of beta_sigma; not NaN */
    int64_t budget;                         /* 1 .. FSQ_LOGNORMAL_MAX_BUDGET: most surviving sequences enumerated for one track */
    int32_t max_possible;                   /* 1 .. FSQ_LOGNORMAL_MAX_POSSIBLE */
    int32_t allow_multidrop;                /* 0: consecutive counts differ by at most 1 */
} FsqLognormalParams;

/* Bytes of device workspace fsq_lognormal_fit needs (0: none), -1 for an invalid shape. */
int64_t fsq_lognormal_workspace_bytes(int64_t n_tracks, int32_t max_frames);

/* The fit of n_tracks ragged tracks, one wavefront per track.
 *   d_intensity   double [n_tracks][max_frames]  row t holds d_n_frames[t] frames; log(I) for I > 0, else -10000 (:5423)
 *   d_category    uint64 [n_tracks]              bit f set when frame f is ON
 *   d_n_frames    int32  [n_tracks]              1 .. max_frames (max_frames <= FSQ_LOGNORMAL_MAX_FRAMES)
 *   d_status      int32  [n_tracks]              FSQ_LOGNORMAL_*
 *   d_best_seq    uint8  [n_tracks][max_frames]  the winning counts
 *   d_best_score  double [n_tracks]              the winning product; -1 without a winner, as the reference leaves it
 *   d_frame_score double [n_tracks][max_frames]  the winner's per-frame densities (1.0 at count 0)
 *   d_n_surviving int64  [n_tracks]              sequences that pass the category, multi-drop and deviation rules, counted
 *                                                exactly before anything is enumerated (saturating at FSQ_LOGNORMAL_MAX_BUDGET)
 * Every element of every output row is written: frames beyond n_frames and tracks without a winner get count 0,
 * frame score 0 and best score -1.  A track costs O(max_frames * max_possible^2) for the count plus O(max_frames) per
 * surviving sequence, and at most `budget` sequences. */
int fsq_lognormal_fit(const double* d_intensity, const uint64_t* d_category, const int32_t* d_n_frames, int64_t n_tracks,
                      int32_t max_frames, const FsqLognormalParams* prm, int32_t* d_status, uint8_t* d_best_seq,
                      double* d_best_score, double* d_frame_score, int64_t* d_n_surviving, void* d_ws, int64_t ws_bytes,
                      void* stream);

/* d_out[i] = log(d_x[i]) as glibc 2.35 (x86-64, FMA) rounds it, for every double (log(0) = -inf, log(x < 0) = NaN). */
int fsq_lognormal_log(const double* d_x, double* d_out, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif
