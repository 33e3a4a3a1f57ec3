/* fsq_montecarlo.h - C ABI of the seeded Monte-Carlo PSF fit (libfsq_hip.so, gfx950).
 *
 * pflib._fit_2d_gaussian_monte_carlo (pflib.py:117-177) and the fit_type='monte_carlo' branch of pflib.find_peptides
 * (:441-477): n_iter random parameter sets of a circular Gaussian are tried on a 5x5 ROI and the one with the smallest
 * root of the summed squared residuals is kept.  The reference draws from an unseeded generator; here the draws are explicit
 * and everything computed from them has the reference's bits:
 *   Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (block, iteration, pixel, field); draw j of an
 *   (iteration, pixel, field) triple uses block j >> 1, even j words (0, 1), odd j words (2, 3), and is CPython's
 *   ((a >> 5) * 67108864 + (b >> 6)) / 2^53.  Every iteration starts numpy's legacy polar method with an empty cache and
 *   runs it three times: pair 0 gives H then A, pair 1 h_0 then w_0, pair 2 sigmah then sigmaw (theta is 0.0 and takes no
 *   draw: the reference's exponential draw is multiplied by zero).
 *   pixel = h * W + w of the candidate, field = first_field + its index in the stack: a result does not depend on how the
 *   candidates are batched.
 * Quirks of the reference that are kept: the model is circular (sigmaw is drawn and returned, not used); the image returned
 * is that of the LAST iteration, not of the kept one, and R^2 / rmse are taken from it; the comparison is strict, so the
 * earliest of equal residuals wins and a NaN never does.
 *
 * Every candidate gets
 *   an FsqRow   h0 = h_0 + h - 2.5, w0 = w_0 + w - 2.5, H, A, sigma_h, sigma_w, theta = 0, rmse, r2 (Python's sequential sum),
 *               s_n (on the float ROI), p2 / p3 = the kept h_0 / w_0, status = the fit status below, niter = the winning
 *               iteration (-1: none), nfev = n_iter, key_h = key_w = -1
 *   d_fit_img   double[25]: the last iteration's normalised image
 *   d_rms       double: the kept residual (the start value 250000000 * max(ROI) when no iteration won)
 *   d_status    int32: FSQ_MC_OK; FSQ_MC_NEVER_IMPROVED (the reference's UnboundLocalError: the six parameters are 0.0, the
 *               image and the metrics are still the last iteration's); FSQ_MC_NO_MAXIMUM (its IndexError, raised before the
 *               loop - the ROI holds a NaN: parameters, metrics, image and residual are 0.0, so h0 = h - 2.5)
 * Conventions are those of include/fsq.h: entries enqueue on `stream`, buffers are the caller's, bad arguments return
 * FSQ_EINVAL before any launch.  n_iter is 1 .. 2^31 - 1. */
#ifndef FSQ_MONTECARLO_H
#define FSQ_MONTECARLO_H
#include <stdint.h>

#include "fsq.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_MC_OK 0
#define FSQ_MC_NEVER_IMPROVED 1
#define FSQ_MC_NO_MAXIMUM 2

/* n stand-alone ROIs double[n][25] (any float values) with explicit ids uint32[n][2] = (pixel, field); rows get h = w = 2,
 * field = 0. */
int fsq_mc_fit_rois(const double* d_rois, const uint32_t* d_ids, int64_t n, int64_t n_iter, uint64_t seed, FsqRow* d_rows,
                    double* d_fit_img, double* d_rms, int32_t* d_status, void* stream);

/* The candidates int32[n][3] = (field, h, w) of fsq_detect on uint16[n_fields][H][W]: every ROI is normalised as the caller
 * at pflib.py:446-447 does ((v - min) / float(max - min) on integers, a constant ROI giving NaN), then fitted as above with
 * pixel = h * W + w and field = first_field + the candidate's field.  first_field + n_fields <= 2^32. */
int fsq_mc_fit_candidates(const uint16_t* d_img, int n_fields, int H, int W, const int32_t* d_cand, int64_t n, int64_t n_iter,
                          uint64_t seed, int64_t first_field, FsqRow* d_rows, double* d_fit_img, double* d_rms,
                          int32_t* d_status, void* stream);

/* pflib.find_peptides(fit_type='monte_carlo') for every field of a batch: fsq_detect -> fsq_mc_fit_candidates ->
 * fsq_consolidate -> fsq_kept_rows -> the kept candidates' images, written as the records of fsq_find_peptides
 * (FSQ_PEAK_RECORD_BYTES: row, fit_img, the 25 pixel words of the ROI as they sit in d_img - the caller rebuilds the
 * normalised sub_img from them).
 *   d_field_status  int32[n_fields] out: the fit status of the field's first failing candidate in raster order (what the
 *                   reference's loop raises), 0 if none.  Such a field has no records and d_nkeep 0, whatever its re-key
 *                   assertion says.
 * Everything else as fsq_find_peptides (FSQ_ERANGE with *n_candidates / *n_records when a capacity is too small).
 * prm->pixel_format must be FSQ_PIXELS_U16 (others: FSQ_ENOTIMPL). */
int64_t fsq_find_peptides_mc_workspace_bytes(int n_fields, int H, int W, int64_t cand_cap, int64_t record_cap);
int fsq_find_peptides_mc(const void* d_img, int n_fields, int H, int W, const FsqDetectParams* prm, double r2_threshold,
                         int radius, int py2_round, int64_t n_iter, uint64_t seed, int64_t first_field, int64_t cand_cap,
                         void* d_records, int64_t record_cap, int32_t* d_record_offsets, int32_t* d_nkeep,
                         int32_t* d_field_status, int64_t* n_candidates, int64_t* n_records, void* d_workspace,
                         int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
