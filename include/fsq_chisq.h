/* fsq_chisq.h - C ABI of the chi-squared step fitter and the plateau merge filters (libfsq_hip.so, gfx950).
 *
 * stepfitting_library.chi_squared_step_fitter (:342-505, helpers :67-339: the Kerssemakers et al. best-fit / counter-fit
 * algorithm), filter_upsteps (:732-799), filter_small_steps (:802-926) and stepfit_r_squared (:1483-1503) for a batch of
 * traces.  Conventions are those of fsq_stepfit.h: every entry enqueues on `stream` and does not synchronise, buffers
 * are the caller's, rows are [n_traces][max_frames], d_status holds FSQ_STEPFIT_* per trace, return codes are those of
 * include/fsq.h. */
#ifndef FSQ_CHISQ_H
#define FSQ_CHISQ_H
#include <stdint.h>

#include "fsq_stepfit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_CHISQ_MAX_FRAMES 1024           /* frames of one trace in fsq_chisq_step_fit (max_frames, the row stride, may be larger) */

#define FSQ_MERGE_UPSTEPS 0                 /* fsq_stepfit_merge_filter mode: filter_upsteps */
#define FSQ_MERGE_SMALL_STEPS 1             /* filter_small_steps */

typedef struct {
    int32_t num_steps;                      /* > 0: explicit; 0: min(ceil(num_steps_multiplier * len), len - 2) per trace (:443-446) */
    int32_t min_step_length;
    int32_t ignore_counterfits;             /* != 0: the longest fit instead of the one with the largest S */
    int32_t reserved;
    double num_steps_multiplier;            /* in (0, 1] */
    double min_step_magnitude;
} FsqChisqParams;

/* Bytes of device workspace fsq_chisq_step_fit needs. */
int64_t fsq_chisq_workspace_bytes(int64_t n_traces, int32_t max_frames);

/* chi_squared_step_fitter for n_traces ragged traces.
 *   d_lum        double [n_traces][max_frames]  luminosities; row t holds d_len[t] frames (no NaN)
 *   d_len        int32  [n_traces]
 *   d_fit_*      the returned fit: int32 start / stop, double height [n_traces][max_frames]; d_fit_n int32 [n_traces]
 *   d_n_fits     int32  [n_traces]              plateau counts p = 1 .. n_fits tried (entries of plateau_fits)
 *   d_best_res, d_counter_res, d_S double, d_counter_n int32, each [n_traces][fit_cap] or all NULL: for p = i + 1 the
 *                best-fit residual sum, the counter-fit residual sum, S (1e10 when the best-fit residual is 0) and the
 *                number of counter-fit plateaus; entries beyond fit_cap are not stored
 *   d_status     int32  [n_traces]  FSQ_STEPFIT_OK; FSQ_STEPFIT_INVALID for a length < 1 or > FSQ_CHISQ_MAX_FRAMES or
 *                > max_frames, an explicit num_steps outside 0 < num_steps < len, or a derived num_steps < 0 (len 1);
 *                FSQ_STEPFIT_UNSUPPORTED when the best fit reaches len plateaus, where the reference raises ValueError
 *                (its counter-fit asks for len + 1 plateaus, :306)
 * A FSQ_STEPFIT_INVALID trace leaves every other output row of its own untouched; a FSQ_STEPFIT_UNSUPPORTED trace leaves its
 * fit rows, d_fit_n and d_n_fits untouched (its per-p rows hold the fits tried before the reference would have raised). */
int fsq_chisq_step_fit(const double* d_lum, const int32_t* d_len, int64_t n_traces, int32_t max_frames,
                       const FsqChisqParams* prm, int32_t* d_fit_start, int32_t* d_fit_stop, double* d_fit_h,
                       int32_t* d_fit_n, int32_t* d_n_fits, double* d_best_res, double* d_counter_res,
                       int32_t* d_counter_n, double* d_S, int32_t fit_cap, int32_t* d_status, void* d_ws, int64_t ws_bytes,
                       void* stream);

/* Bytes of device workspace fsq_stepfit_merge_filter needs. */
int64_t fsq_stepfit_merge_filter_workspace_bytes(int64_t n_traces, int32_t max_frames);

/* filter_upsteps (mode FSQ_MERGE_UPSTEPS) or filter_small_steps (FSQ_MERGE_SMALL_STEPS) on caller-given plateaus.
 *   d_lum, d_len, d_in_*, d_in_n   as for the t-test filter of fsq_stepfit.h, with the same plateau checks (FSQ_STEPFIT_INVALID otherwise)
 *   has_min_magnitude / min_magnitude, has_min_noise_ratio / min_noise_ratio   the two criteria of filter_small_steps,
 *                each applied only when its flag is set (None in the reference); ignored by FSQ_MERGE_UPSTEPS
 *   d_out_*      filtered plateaus, same layout; unmerged plateaus keep the given heights, merged ones are refitted
 * len(plateaus) - 1 passes, fewer once a pass merges nothing. */
int fsq_stepfit_merge_filter(const double* d_lum, const int32_t* d_len, int64_t n_traces, int32_t max_frames,
                             const int32_t* d_in_start, const int32_t* d_in_stop, const double* d_in_h, const int32_t* d_in_n,
                             int32_t mode, int32_t has_min_magnitude, double min_magnitude, int32_t has_min_noise_ratio,
                             double min_noise_ratio, int32_t* d_out_start, int32_t* d_out_stop, double* d_out_h,
                             int32_t* d_out_n, int32_t* d_status, void* d_ws, int64_t ws_bytes, void* stream);

/* Bytes of device workspace fsq_stepfit_r_squared needs (0: none). */
int64_t fsq_stepfit_r_squared_workspace_bytes(int64_t n_traces, int32_t max_frames);

/* stepfit_r_squared on caller-given plateaus: d_r2 double [n_traces] (written for FSQ_STEPFIT_OK traces only). */
int fsq_stepfit_r_squared(const double* d_lum, const int32_t* d_len, int64_t n_traces, int32_t max_frames,
                          const int32_t* d_in_start, const int32_t* d_in_stop, const double* d_in_h, const int32_t* d_in_n,
                          double* d_r2, int32_t* d_status, void* d_ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
