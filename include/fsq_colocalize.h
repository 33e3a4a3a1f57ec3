/* fsq_colocalize.h - C ABI of the colocalisation of tracks between colour channels (libfsq_hip.so, gfx950).
 *
 * Which tracks of two colour channels are the same molecule: a definition of this package (the reference stops at one label
 * letter), in exact integers.  Conventions are those of fsq_remainder.h: the entry enqueues on `stream` and does not
 * synchronise, buffers are the caller's, return codes are those of include/fsq.h.
 *
 * THE MATCH of two sets A and B of integer positions (h, w), each cut into n_seg contiguous segments, one per field:
 *   d2(a, b)    = dh * dh + dw * dw in int64; with |coordinate| < 2^30 it is below 2^63
 *   best_b(a)   the b of a's segment with the smallest (d2, index of b) among those with d2 <= radius_sq; none without one
 *   best_a(b)   the a of b's segment with the smallest (d2, index of a) among those with d2 <= radius_sq
 *   a pair      a and b with best_b(a) = b and best_a(b) = a: mutual nearest neighbours, ties to the lowest index
 * An a whose best b prefers another a stays unmatched; it does not fall back to its second-best b. */
#ifndef FSQ_COLOCALIZE_H
#define FSQ_COLOCALIZE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The match of n_a positions A and n_b positions B in n_seg segments.
 *   a_hw          int32 [n_a, 2]      (h, w), |coordinate| < 2^30: the caller's to see to (a larger one makes d2 wrap; nothing
 *                                     is read or written out of bounds for it)
 *   a_seg         int32 [n_a]         the segment of every a
 *   a_off, b_off  int64 [n_seg + 1]   a's a_off[s] .. a_off[s + 1] - 1 and b's b_off[s] .. b_off[s + 1] - 1 are segment s:
 *                                     ascending, off[0] = 0, off[n_seg] = n
 *   b_hw          int32 [n_b, 2]
 *   match_of_a    int32 [n_a]         the b paired with a, or -1
 *   match_of_b    int32 [n_b]         the a paired with b, or -1; filled with -1 by the entry itself
 *   dist_sq_of_a  int64 [n_a]         d2 of a's pair, or -1
 *   d_bad         int32 [1]           set to 0 by the entry, then to 1 where a_seg or the offsets are not well formed
 * One lane per a: it scans its segment's B range for best_b(a), then the segment's A range for best_a(best_b(a)); if that is
 * a itself it stores both directions.  A pair has one writer per element: no atomics, and no lane waits on another.
 * a_seg and the offsets live on the device, so the host cannot refuse them.  A lane is bad when its a_seg is not in 0 ..
 * n_seg - 1, when its segment's offsets do not satisfy 0 <= off[s] <= off[s + 1] <= n in A and in B, or when it does not
 * stand in its segment's A range: it stores -1 twice and sets d_bad (every writer writes the same 1).  So does lane s for a
 * segment s whose offsets are not well formed, or whose first and last ones are not 0 and n.  Every loop runs over a range
 * that passed that test; nothing is read or written out of bounds whatever the three arrays hold.  With d_bad set the other
 * lanes' results are not meaningful (ranges may overlap).
 * 0 <= n_a, n_b < 2^31, 0 <= n_seg < 2^31, 0 <= radius_sq, a_hw and b_hw 8-byte aligned (a position is read as one pair);
 * else FSQ_EINVAL, and nothing is written.  One memset of
 * match_of_b, one of d_bad and one launch on `stream`. */
int fsq_colocalize_match(const int32_t* a_hw, const int32_t* a_seg, const int64_t* a_off, const int64_t* b_off, const int32_t* b_hw,
                         int64_t radius_sq, int64_t n_a, int64_t n_b, int64_t n_seg, int32_t* match_of_a, int32_t* match_of_b,
                         int64_t* dist_sq_of_a, int32_t* d_bad, void* stream);

#ifdef __cplusplus
}
#endif
#endif
