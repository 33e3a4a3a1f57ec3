/* fsq_background_joint.h - C ABI of the device part of the background correction for joint signals of several colour
 * channels (libfsq_hip.so, gfx950): the mean of many neighbour lists in one launch.
 *
 * A joint signal is (decrements, zeros, starts) of peptide_simulator.joint_signal, the letters sorted; a definition of this
 * package, the reference stops at one letter.  The neighbours of a key with d drops are its own tuple with the cycles c_i + e_i
 * in place of c_i, the letters, zeros and starts kept, for e in itertools.product((-1, 0, 1), repeat=d), e != 0, in that
 * order, every 0 < c_i + e_i <= num_cycles, without a repeated cycle when multidrop is excluded.  A kept candidate is looked
 * up as it stands: a perturbed tuple that no longer ascends by (cycle, letter) is no key and counts 0.  With up to
 * FSQ_BACKGROUND_JOINT_MAX_DROPS drops a key has up to 6 560 neighbours, nine times what fsq_background_iterate's one lane
 * adds serially.  The iteration on joint keys runs on the host (background.joint_background_records); its interpolation,
 * MCsimlib.interpolate_signal for many targets at once, is the entry below. */
#ifndef FSQ_BACKGROUND_JOINT_H
#define FSQ_BACKGROUND_JOINT_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_BACKGROUND_JOINT_MAX_DROPS 8            /* 3^8 - 1 = 6 560 neighbours */
#define FSQ_BACKGROUND_JOINT_MAX_NEIGHBOURS 6560    /* and the longest list fsq_background_neighbour_means adds */
#define FSQ_BACKGROUND_JOINT_MAX_CYCLES 63          /* a cycle is 6 bits of the joint key (fsq_signal_sweep.h) */

/* np.mean of n_lists ragged lists of counts in one launch, one wavefront per list: list l is d_nb[d_nb_off[l] ..
 * d_nb_off[l + 1] - 1], indices into d_count[n_counts]; an index outside 0 .. n_counts - 1 counts 0.  d_out[l] is
 * (0.0 + numpy's pairwise sum) / length with numpy's bits, NaN for an empty list, and NaN for a list whose offsets do not
 * ascend or that is longer than FSQ_BACKGROUND_JOINT_MAX_NEIGHBOURS (nothing of it is read).  d_nb_off: int64 [n_lists + 1],
 * ascending from >= 0; d_nb must hold d_nb_off[n_lists] entries, and may be NULL where every list is empty (a non-empty
 * list then gives NaN).  Enqueues on `stream` and does not synchronise. */
int fsq_background_neighbour_means(const int32_t* d_nb, const int64_t* d_nb_off, int64_t n_lists, const double* d_count,
                                   int64_t n_counts, double* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
