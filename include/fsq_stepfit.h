/* fsq_stepfit.h - C ABI of the spot-trace step fit (libfsq_hip.so, gfx950).
 *
 * Trace.stepfit_photometries (flexlibrary.py:1380-1462) for a batch of photometry traces: mirror
 * (stepfitting_library.py:1703-1719), optional Chung-Kennedy filter (:1081-1274), sliding-window Welch t-test step
 * finder (sliding_t_fitter, :929-1078), plateau refit (refit_plateaus, :1322), t-test plateau merging (t_test_filter,
 * :1328-1480) and unmirroring (:1721-1746).  Every entry enqueues on `stream` and does not synchronise.
 * Return codes are those of include/fsq.h (FSQ_OK, FSQ_EINVAL, FSQ_EHIP, ...). */
#ifndef FSQ_STEPFIT_H
#define FSQ_STEPFIT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_STEPFIT_MAX_WINDOWS 16
#define FSQ_STEPFIT_MAX_MIRRORED 8192       /* frames after mirroring: numpy's buffered reduction changes order beyond */

/* Per-trace status values written to d_status. */
#define FSQ_STEPFIT_OK 0
#define FSQ_STEPFIT_UNSUPPORTED 1           /* a t-filter pass sorted >= 64 pairs with a NaN p: CPython's merge sort order */
#define FSQ_STEPFIT_INVALID 2               /* length < 1, > max_frames, mirrored > 8192, or CK on <= 2 mirrored frames */

typedef struct {
    int32_t mirror_start;                   /* frames mirrored in front (mirror_photometries) */
    int32_t chung_kennedy;                  /* > 0: one CK pass of the unfiltered mirrored sequence (flexlibrary.py:1432-1436) */
    int32_t n_windows;                      /* CK window lengths (<= FSQ_STEPFIT_MAX_WINDOWS, each 1..64) */
    int32_t window_lengths[FSQ_STEPFIT_MAX_WINDOWS];
    int32_t M;                              /* CK comparison window (1..64) */
    int32_t p;                              /* CK weight exponent: 2 only */
    int32_t window_radius;                  /* sliding_t_fitter: radii range(5, window_radius), window_radius <= 64 */
    int32_t drop_sort;                      /* t_test_filter drop_sort */
    double p_threshold;
    int32_t has_photometry_min;             /* photometries become max(photometry_min, v) */
    double photometry_min;
} FsqStepfitParams;

/* Bytes of device workspace fsq_stepfit_traces needs for n_traces traces of at most max_frames frames. */
int64_t fsq_stepfit_workspace_bytes(int64_t n_traces, int32_t max_frames, const FsqStepfitParams* prm);

/* Trace.stepfit_photometries (flexlibrary.py:1380-1462) for n_traces traces at once.
 *   d_phot     double [n_traces][max_frames]   photometries (None spots as 0); row t holds d_len[t] frames
 *   d_len      int32  [n_traces]
 *   d_ck       double [n_traces][max_frames]   unmirrored CK-filtered sequence (the clamped photometries when chung_kennedy == 0)
 *   d_pl_*     plateaus of sliding_t_fitter refitted on the unfiltered sequence, unmirrored: int32 start / stop, double
 *              height, [n_traces][max_frames]; d_pl_n int32 [n_traces] counts
 *   d_tf_*     the same after t_test_filter (no_merge_start = mirror_start)
 *   d_status   int32  [n_traces]               FSQ_STEPFIT_*
 *   d_p        double [n_traces][n_radii][Lmax] or NULL: sliding-window p of every radius and mirrored frame, where
 *              n_radii = max(window_radius - 5, 0) and Lmax = max_frames + min(mirror_start, max_frames)
 *   d_pair_p   double [n_traces][pair_cap] or NULL: p of every t-filter pair test in the order run (passes stop at the
 *              first pass that merges nothing); d_pair_n int32 [n_traces] counts them (entries beyond pair_cap are not stored)
 * Rows are written up to each trace's length / count only. */
int fsq_stepfit_traces(const double* d_phot, const int32_t* d_len, int64_t n_traces, int32_t max_frames,
                       const FsqStepfitParams* prm, double* d_ck, int32_t* d_pl_start, int32_t* d_pl_stop, double* d_pl_h,
                       int32_t* d_pl_n, int32_t* d_tf_start, int32_t* d_tf_stop, double* d_tf_h, int32_t* d_tf_n,
                       int32_t* d_status, double* d_p, double* d_pair_p, int32_t* d_pair_n, int32_t pair_cap,
                       void* d_ws, int64_t ws_bytes, void* stream);

/* Bytes of device workspace fsq_stepfit_ttest_filter needs. */
int64_t fsq_stepfit_ttest_filter_workspace_bytes(int64_t n_traces, int32_t max_frames);

/* stepfitting_library.t_test_filter (:1441-1480, single pass :1328-1438) on caller-given plateaus, one trace per row:
 *   d_lum      double [n_traces][max_frames]   luminosities; d_len int32 [n_traces]
 *   d_in_*     int32 start / stop, double height [n_traces][max_frames], d_in_n int32 [n_traces]: consecutive plateaus
 *              (stop_i + 1 == start_{i+1}, 0 <= start_0, stop_last < len); otherwise the trace's status is FSQ_STEPFIT_INVALID
 *   d_tf_*     filtered plateaus, same layout; unmerged plateaus keep the given heights, merged ones are refitted
 *   d_status, d_pair_p, d_pair_n, pair_cap as for fsq_stepfit_traces. */
int fsq_stepfit_ttest_filter(const double* d_lum, const int32_t* d_len, int64_t n_traces, int32_t max_frames,
                             const int32_t* d_in_start, const int32_t* d_in_stop, const double* d_in_h, const int32_t* d_in_n,
                             double p_threshold, int32_t drop_sort, int32_t no_merge_start, int32_t* d_tf_start,
                             int32_t* d_tf_stop, double* d_tf_h, int32_t* d_tf_n, int32_t* d_status, double* d_pair_p,
                             int32_t* d_pair_n, int32_t pair_cap, void* d_ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
