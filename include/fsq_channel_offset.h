/* fsq_channel_offset.h - C ABI of the estimate of the integer offset between two colour channels (libfsq_hip.so, gfx950).
 *
 * fsq_colocalize_match (include/fsq_colocalize.h) compares the positions of two channels after each channel's integer offset
 * was added; this header estimates that offset from the positions themselves.  Like the match it is a definition of this
 * package (the reference stops at one label letter), in exact integers.  Conventions are those of fsq_colocalize.h: the
 * entries enqueue on `stream` and do not synchronise, buffers are the caller's, return codes are those of include/fsq.h.
 *
 * A (the anchor) and B (the channel whose offset is wanted) are two sets of integer positions (h, w), each cut into n_seg
 * contiguous segments, one per field, exactly as for fsq_colocalize_match.
 *   VOTES   for a half-width W, V[dh + W][dw + W] = the number of pairs (a, b) of one segment with dh = a.h - b.h,
 *           dw = a.w - b.w, |dh| <= W and |dw| <= W, summed over all segments: int64 [2W + 1][2W + 1].  The differences are
 *           taken in int64 (with |coordinate| < 2^30 one reaches 2^31 - 2).  (dh, dw) is what has to be ADDED TO B's
 *           positions to land on A: the sign of the match's offsets.
 *   SCORE   for a search range R and a tolerance tol_sq (t = isqrt(tol_sq), R + t <= W), S[o] = the sum of V[o + d] over the
 *           d with |d|^2 <= tol_sq, for every offset o of [-R, R]^2: the number of pairs that lie within the match's radius
 *           once o is applied.  int64 throughout.
 *   PEAK    the offset with the largest S; ties go to the smallest (dh^2 + dw^2, dh, dw), so a smaller shift is preferred and
 *           nothing depends on scan order.  An all-zero V gives (0, 0) with score 0. */
#ifndef FSQ_CHANNEL_OFFSET_H
#define FSQ_CHANNEL_OFFSET_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_CHANNEL_OFFSET_MAX_W 64           /* the largest half-width: a histogram of 129 x 129 bins */
#define FSQ_CHANNEL_OFFSET_RECORD 16          /* int64 words of fsq_channel_offset_peak's result */

/* The votes of n_a positions A against n_b positions B in n_seg segments.
 *   a_hw, a_seg, a_off, b_off, b_hw, n_a, n_b, n_seg   as for fsq_colocalize_match
 *   W             0 .. FSQ_CHANNEL_OFFSET_MAX_W
 *   votes         int64 [(2W + 1)^2]  V, row-major; cleared by the entry itself
 *   d_bad         int32 [1]           set to 0 by the entry, then to 1 where a_seg or the offsets are not well formed, or where
 *                                     a lane's segment holds 2^24 or more b's
 * One lane per a, 256 per block: the lane walks its segment's B range from global memory and adds its votes to the block's
 * uint32 histogram in LDS ((2W + 1)^2 words of dynamic LDS, 66 564 B at W = 64); at block end the non-zero bins are added to
 * `votes` with 64-bit integer atomics.  Integer adds commute: the result is exact and the same in every run.  No 32-bit
 * counter can wrap: a lane votes at most once per b, a lane whose segment holds 2^24 or more b's votes nothing and sets d_bad,
 * and 256 lanes x (2^24 - 1) < 2^32.
 * A lane is bad under fsq_colocalize_match's rules (its a_seg, its segment's offsets in A and in B, its own place in its A
 * range; lane s < n_seg proves segment s's offsets and the two ends): it votes nothing and sets d_bad.  Every loop runs over
 * a range that passed that test; nothing is read or written out of bounds whatever the three arrays hold.  With d_bad set
 * `votes` holds the good lanes' votes only and is not meaningful.
 * 0 <= W <= 64, 0 <= n_a, n_b, n_seg < 2^31, a_hw, b_hw, the offsets and votes 8-byte aligned; else FSQ_EINVAL, and nothing is
 * written.  Two memsets and one launch on `stream`. */
int fsq_channel_offset_votes(const int32_t* a_hw, const int32_t* a_seg, const int64_t* a_off, const int64_t* b_off,
                             const int32_t* b_hw, int64_t W, int64_t n_a, int64_t n_b, int64_t n_seg, int64_t* votes,
                             int32_t* d_bad, void* stream);

/* The peak of a histogram of votes.
 *   votes    int64 [(2W + 1)^2]   V (bins are taken as they are: sums of them must stay below 2^63)
 *   result   int64 [16]           [0] dh  [1] dw  [2] score = S at the peak
 *                                 [3] runner_up: the largest S among the offsets at Chebyshev distance > 2t from the peak,
 *                                     -1 when the window has none
 *                                 [4] total: the sum of V
 *                                 [5] at_edge: 1 when |dh| == R or |dw| == R (the true offset may lie outside the window)
 *                                 [6] n_ties: the number of offsets of the window with the peak's score
 *                                 [7 .. 15] the 3 x 3 of V around the peak, row-major, 0 where outside V
 *   scores   int64 [(2R + 1)^2]   S, row-major, or NULL
 * One block of 256 lanes: every lane scores its offsets of the window and keeps its best under the order (larger S, smaller
 * dh^2 + dw^2, smaller dh, smaller dw), the block reduces those; a second pass over the window and over V gives runner_up,
 * n_ties, total and the 3 x 3.  All sums are int64.
 * 0 <= R, 0 <= tol_sq, R + isqrt(tol_sq) <= W <= 64, votes, result and scores 8-byte aligned; else FSQ_EINVAL, and nothing is
 * written.  One launch on `stream`. */
int fsq_channel_offset_peak(const int64_t* votes, int64_t W, int64_t R, int64_t tol_sq, int64_t* result, int64_t* scores,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif
