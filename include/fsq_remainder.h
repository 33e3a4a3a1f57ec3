/* fsq_remainder.h - C ABI of the remainder correction of track photometries (libfsq_hip.so, gfx950).
 *
 * MCsimlib._remainder_adjust_2 (:3434-3472, what remainder_correction.py's method 4 runs) and its additive sibling
 * MCsimlib._remainder_adjust (:3398-3431): per (channel, field) and frame, the median over the field's remainders (tracks whose
 * category is ON in every frame) of a per-track quantity, and every track of the field adjusted by it.  Conventions are those of
 * fsq_binsearch.h: every entry enqueues on `stream` and does not synchronise, buffers are the caller's, return codes are those
 * of include/fsq.h.
 *
 * The arithmetic, all in float64, every operation rounded on its own (no fma), division IEEE:
 *   remainder   all F category bits set
 *   m           np.median of the track's F intensities: the middle one a as a + 0.0, or (a + (0.0 + b)) / 2.0 of the two
 *               middle ones (np.mean's sum starts from +0.0: a median of -0.0 comes out as +0.0, all else is a or (a + b) / 2)
 *   RATIO       value_f = (I_f - m) / m                                   (:3443-3446)
 *   ADDITIVE    value_f = I_f                                             (:3407-3408)
 *   median_f    np.median of the R values of the segment's remainders at frame f (:3454, :3414): NaN where any value is NaN
 *               or R = 0, else the (R-1)/2-th order statistic or the mean of the R/2-1-th and the R/2-th, as for m.  +-inf
 *               order as numbers; -0.0 orders before +0.0, which never shows: a zero in the middle gives +0.0 or, next to
 *               another value b, b / 2.0 whatever its sign
 *   RATIO       adjustment_f = median_f,            adjusted = I * (1.0 - adjustment_f)   (:3468)
 *   ADDITIVE    adjustment_f = median_f - median_0, adjusted = I - adjustment_f           (:3416, :3427)
 *   kept        R >= minimum_r_per_field (:3450, :3412); ADDITIVE also needs R >= 1 (a field without a remainder never enters
 *               remainder_values, :3403-3406) */
#ifndef FSQ_REMAINDER_H
#define FSQ_REMAINDER_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_REMAINDER_MAX_FRAMES 64         /* the category word, as FSQ_LOGNORMAL_MAX_FRAMES */
/* Up to this many values a (segment, frame) is selected in LDS (the keys of all values, 4 KiB, ranked against each other);
 * above it a radix select makes nine passes over the workspace. */
#define FSQ_REMAINDER_LDS_MAX 512

#define FSQ_REMAINDER_RATIO 0               /* _remainder_adjust_2 */
#define FSQ_REMAINDER_ADDITIVE 1            /* _remainder_adjust */

typedef struct FsqRemainderParams {
    int32_t mode;                           /* FSQ_REMAINDER_RATIO | FSQ_REMAINDER_ADDITIVE */
    int32_t minimum_r_per_field;
} FsqRemainderParams;

/* Bytes of workspace fsq_remainder_adjust needs: n_tracks * n_frames values and one segment index per track.  Negative
 * (FSQ_EINVAL) for a shape fsq_remainder_adjust refuses. */
int64_t fsq_remainder_workspace_bytes(int64_t n_tracks, int n_frames, int64_t n_segments);

/* The correction of n tracks of F frames in S segments, one segment per (channel, field).
 *   intensity     double   [n, F]   (:3441, :3402)
 *   category      uint64   [n]      bit f set when frame f is ON (:3442, :3403)
 *   seg_off       int64    [S + 1]  tracks seg_off[s] .. seg_off[s + 1] - 1 are segment s: ascending, seg_off[0] = 0,
 *                                   seg_off[S] = n.  It lives on the device, so the host cannot refuse it: a track that no
 *                                   well-formed segment holds is treated as one of a dropped segment, and nothing is read or
 *                                   written out of bounds.
 *   prm                             on the host
 *   adjustment    double   [S, F]   (:3453-3454, :3416-3419), also for the segments that are not kept
 *   n_remainders  int32    [S]      R (:3450, :3412)
 *   kept          uint8    [S]      1 or 0
 *   adjusted      double   [n, F]   (:3468, :3427); the rows of a segment that is not kept are 0
 *   ws, ws_bytes                    at least fsq_remainder_workspace_bytes(n, F, S), 8-byte aligned
 * 0 <= n < 2^31, 1 <= F <= FSQ_REMAINDER_MAX_FRAMES (FSQ_ENOTIMPL above), 0 <= S, S * F < 2^31.
 * Four launches on `stream` after one memset of n_remainders; no host round trip between them. */
int fsq_remainder_adjust(const double* intensity, const uint64_t* category, const int64_t* seg_off, int64_t n, int F, int64_t S,
                         const FsqRemainderParams* prm, double* adjustment, int32_t* n_remainders, uint8_t* kept,
                         double* adjusted, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
