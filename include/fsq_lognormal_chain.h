/* fsq_lognormal_chain.h - C ABI of the per-track steps between the two fits of the lognormal chain (libfsq_hip.so, gfx950).
 *
 * lognormal_fitter_v2.main's chain on a track table (n tracks of exactly F frames, one channel, the tracks of a field
 * contiguous): the last-drop lists of MCsimlib.last_drop_method_v2 (:5357-5384), the ON -> OFF entries of
 * jupyter_development.grab_ON_OFFS (:63-84) with their medians, and ON_OFF_adjust_photometries (:262-276).  The bin searches
 * (fsq_binsearch.h) and the fits (fsq_lognormal.h) are entries of their own.  Conventions are those of fsq_remainder.h: every
 * entry enqueues on `stream` and does not synchronise, buffers are the caller's, return codes are those of include/fsq.h.
 *
 * The arithmetic, all in float64, every operation rounded on its own (no fma), division IEEE:
 *   ON(f)        bit f of the track's category word
 *   last drop    log(I_f), glibc 2.35's log, for every f with truncate <= f < F - 1, ON(f), not ON(f + 1) and I_f > 0
 *   entry        I_f - alpha under key (segment, f) for every track with fit_status 0 (FSQ_LOGNORMAL_FOUND) and every
 *                f < F - 1 with ON(f) and not ON(f + 1)
 *   m[s, f]      np.median of the key's entries (the rule of fsq_remainder.h: the middle one a as a + 0.0, or
 *                (a + (0.0 + b)) / 2.0 of the two middle ones); NaN for a key without entries
 *   M            np.median of the m[s, f] of the keys that have entries; NaN without any
 *   adjusted     (I_f - alpha) * M / m[s, f] where f < F - 1 and the key has entries (the product first, then the quotient),
 *                else the raw I_f (as in the reference, those frames are not alpha-adjusted) */
#ifndef FSQ_LOGNORMAL_CHAIN_H
#define FSQ_LOGNORMAL_CHAIN_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_CHAIN_MAX_FRAMES 64             /* the category word, as FSQ_REMAINDER_MAX_FRAMES */

/* Shapes every entry takes: 0 <= n < 2^31, 1 <= F <= FSQ_CHAIN_MAX_FRAMES (FSQ_ENOTIMPL above), 0 <= S and
 * S * (F - 1) < 2^31.  The *_workspace_bytes functions give FSQ_EINVAL (negative) for any other; last_drops' n_segments
 * is not used. */
int64_t fsq_chain_last_drops_workspace_bytes(int64_t n_tracks, int n_frames, int64_t n_segments);
int64_t fsq_chain_on_off_medians_workspace_bytes(int64_t n_tracks, int n_frames, int64_t n_segments);
int64_t fsq_chain_on_off_adjust_workspace_bytes(int64_t n_tracks, int n_frames, int64_t n_segments);

/* The last-drop values of n tracks in (track, frame) order, in two passes with the caller's exclusive scan between them (no
 * atomic append: the order is the host list's).
 *   intensity    double  [n, F]
 *   category     uint64  [n]
 *   truncate     >= 0: frames before it give no value
 *   track_off    int64   [n]        NULL: the counting pass.  Else the writing pass: where track i's values start, the
 *                                   exclusive sum of track_count.  It lives on the device, so the host cannot vouch for it:
 *                                   a track whose values would not lie in 0 .. capacity - 1 writes nothing.
 *   track_count  int64   [n]        counting pass: how many values track i gives, 0 .. F - 1.  Not used in the writing pass.
 *   values       double  [capacity] writing pass: log(I_f) of every value; the count of all of them is the inclusive sum's
 *                                   last element, in device memory
 * One launch, one wavefront per track and one lane per frame. */
int fsq_chain_last_drops(const double* intensity, const uint64_t* category, int64_t n, int F, int truncate,
                         const int64_t* track_off, int64_t* track_count, double* values, int64_t capacity, void* ws,
                         int64_t ws_bytes, void* stream);

/* The ON -> OFF entries per (segment, frame) and their medians.
 *   intensity         double  [n, F]      the raw intensities
 *   category          uint64  [n]
 *   seg_off           int64   [S + 1]     as in fsq_remainder.h; on the device, so a track that no well-formed segment holds
 *                                         gives no entry, and nothing is read or written out of bounds
 *   fit_status        int32   [n]         fsq_lognormal_fit's status of the first fit
 *   on_off_median     double  [S, F - 1]  m, NaN for a key without entries
 *   on_off_count      int32   [S, F - 1]  the keys' entries
 *   last_beta_median  double  [1]         M
 *   ws, ws_bytes                          at least fsq_chain_on_off_medians_workspace_bytes(n, F, S), 8-byte aligned
 * Three launches on `stream` after two memsets; no host round trip between them. */
int fsq_chain_on_off_medians(const double* intensity, const uint64_t* category, const int64_t* seg_off, const int32_t* fit_status,
                             int64_t n, int F, int64_t S, double alpha, double* on_off_median, int32_t* on_off_count,
                             double* last_beta_median, void* ws, int64_t ws_bytes, void* stream);

/* adjusted double [n, F] of fsq_chain_on_off_medians' outputs, one thread per value.  A track that no well-formed segment
 * holds keeps its raw intensities. */
int fsq_chain_on_off_adjust(const double* intensity, const int64_t* seg_off, int64_t n, int F, int64_t S, double alpha,
                            const double* on_off_median, const int32_t* on_off_count, const double* last_beta_median,
                            double* adjusted, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
