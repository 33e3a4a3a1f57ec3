/* fsq_timetrace.h - C ABI of the timetrace experiment table (libfsq_hip.so, gfx950).
 *
 * What TimetraceExperiment.save_experiment_as_csv (flexlibrary.py:3550-3709) computes per trace and frame - the plateau
 * that holds the frame, PlateauTrace.last_step_info, Trace.coefficient_of_determination (:1476-1514) - for a batch of
 * traces, and the glue between fsq_centroid_tracking, fsq_mexican_hat and fsq_stepfit_traces that keeps a whole
 * experiment on the device.  Conventions are those of fsq_stepfit.h and fsq_chisq.h: every entry enqueues on `stream` and
 * does not synchronise, buffers are the caller's, rows are [n_traces][max_frames] with max_frames <=
 * FSQ_STEPFIT_MAX_MIRRORED, d_status holds one word per trace, return codes are those of include/fsq.h. */
#ifndef FSQ_TIMETRACE_H
#define FSQ_TIMETRACE_H
#include <stdint.h>

#include "fsq_stepfit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_TIMETRACE_ZERO_TSS 3            /* d_status: the trace's total sum of squares is 0 (the reference divides by it) */

/* The experiment table of n_traces ragged traces and their step fits.
 *   d_phot       double [n_traces][max_frames]  photometries; row t holds d_len[t] frames
 *   d_len        int32  [n_traces]
 *   d_sf_*       the step fit: int32 start / stop, double height [n_traces][max_frames]; d_sf_n int32 [n_traces]
 * per frame f of trace t, in the plateau k that holds it:
 *   d_plateau_index   int32   k
 *   d_plateau_height  double  h_k
 *   d_plateau_length  int32   stop_k - start_k + 1
 *   d_step_num        int32   PlateauTrace.last_step_info at the plateau's first frame, which hands the PLATEAUS to
 *   d_step_size       double  stepfitting_library.last_step_info as if they were steps: k >= 1 gives (k - 1, h_{k-1}) - the
 *                             previous plateau's height, not a difference; k == 0 gives (0, h_0) when there is one plateau
 *                             or stop_0 == 0, else None: d_step_num -1, d_step_size 0.0
 * per trace:
 *   d_rss        double  Python's left-to-right sum over all frames of pow(p_f - h_k(f), 2.0)
 *   d_tss        double  the same sum of pow(p_f - mean, 2.0), mean = np.mean(p) (numpy's pairwise sum / n)
 *   d_r2         double  1.0 - rss / tss
 *   d_status     int32   FSQ_STEPFIT_OK; FSQ_STEPFIT_INVALID unless 1 <= len <= max_frames, 1 <= n <= len and the plateaus are
 *                consecutive (start_i <= stop_i, stop_i + 1 == start_{i+1}) with start_0 == 0 and stop_last == len - 1;
 *                FSQ_TIMETRACE_ZERO_TSS when tss == 0: the per-frame rows, d_rss and d_tss are written, d_r2 is left alone
 * A FSQ_STEPFIT_INVALID trace leaves every other output row of its own untouched.  n_traces == 0 launches nothing. */
int fsq_timetrace_table(const double* d_phot, const int32_t* d_len, int64_t n_traces, int32_t max_frames,
                        const int32_t* d_sf_start, const int32_t* d_sf_stop, const double* d_sf_h, const int32_t* d_sf_n,
                        int32_t* d_plateau_index, double* d_plateau_height, int32_t* d_plateau_length, int32_t* d_step_num,
                        double* d_step_size, double* d_rss, double* d_tss, double* d_r2, int32_t* d_status, void* stream);

/* Per frame the height (and, when d_index is not NULL, the index) of the plateau that holds it, for any consecutive
 * plateau table that starts at frame 0: PlateauTrace.photometry for every frame 0 .. stop_last.  Frames beyond stop_last are
 * left alone.  d_status: FSQ_STEPFIT_OK, or FSQ_STEPFIT_INVALID (rows untouched) unless 1 <= n, start_0 == 0, the plateaus are
 * consecutive and stop_last < max_frames. */
int fsq_plateau_values(const int32_t* d_start, const int32_t* d_stop, const double* d_h, const int32_t* d_n, int64_t n_traces,
                       int32_t max_frames, double* d_height, int32_t* d_index, int32_t* d_status, void* stream);

/* fsq_centroid_tracking's output as the spot table fsq_mexican_hat / fsq_mexican_hat_u32 reads.
 *   d_hw         int32 [n_traces][n_frames][2]   (h, w) per trace and frame
 *   d_present    uint8 [n_traces][n_frames]      0: the trace has no Spot in that frame
 *   d_fhw        int32 [n_traces * n_frames][3]  (frame, h, w); an absent entry gets the trace's first present position, so
 *                that every row lies inside the frames ((0, 0) for a trace that is present nowhere) */
int fsq_timetrace_spot_rows(const int32_t* d_hw, const uint8_t* d_present, int64_t n_traces, int32_t n_frames, int32_t* d_fhw,
                            void* stream);

/* The photometries of that spot table as step-fit rows: d_rows[t][f] = d_present[t][f] ? d_values[t * n_frames + f] : 0.0
 * (a None Spot's photometry is 0), d_len[t] = n_frames.  d_rows is double [n_traces][n_frames]. */
int fsq_timetrace_photometry_rows(const double* d_values, const uint8_t* d_present, int64_t n_traces, int32_t n_frames,
                                  double* d_rows, int32_t* d_len, void* stream);

#ifdef __cplusplus
}
#endif
#endif
