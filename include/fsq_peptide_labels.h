/* fsq_peptide_labels.h - C ABI of the peptide Monte-Carlo simulation for several label letters, one colour channel each
 * (libfsq_hip.so, gfx950).
 *
 * fsq_peptide_sim.h's simulation with `labels` a set of up to FSQ_PEPTIDE_MAX_CHANNELS letters: peptide_simulator.py counts
 * the dyes per letter (:128-145) and draws one intensity row per letter (:485-497).  The chemistry needs no new draw rule:
 * the reference draws once per residue whose letter is in `labels`, in position order, whatever the letter, which is the
 * walk of fsq_peptide_sim.h on the union of the channels' masks.
 *
 * Draw contract (the draws themselves are those of fsq_peptide_sim.h: Philox4x32-10 keyed by seed, counter (block, molecule,
 * stream)).  Stream 0: the chemistry on the union mask.  Channel 0's photometry reads stream 1 (superdye draws) and stream 2
 * (the uniforms of the polar normals); channel k >= 1 reads streams 2 + 2k and 3 + 2k (stream 3 stays the proteome
 * Monte-Carlo's).  Every channel of every molecule starts with an empty Gaussian cache.  With n_channels = 1 every table
 * therefore equals fsq_peptide_simulate's bit for bit.
 *
 * Order contract.  The reference iterates a Python-2 dict of letters, an order nobody can pin; callers here pass the channels
 * in the order of the sorted label letters.  A channel's draws do not depend on that order: each has its own streams.
 *
 * Conventions are those of fsq_peptide_sim.h: the entry enqueues on `stream` and does not synchronise, buffers are the
 * caller's, every element of every output is written, return codes are those of include/fsq.h. */
#ifndef FSQ_PEPTIDE_LABELS_H
#define FSQ_PEPTIDE_LABELS_H
#include <stdint.h>

#include "fsq_peptide_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_PEPTIDE_MAX_CHANNELS 4

typedef struct {
    uint64_t channel_mask[FSQ_PEPTIDE_MAX_CHANNELS];    /* bit i: residue i carries channel k's letter; disjoint, no bit at or
                                                           above `length`, at most FSQ_PEPTIDE_MAX_LABELLED bits each */
    uint64_t seed;
    int64_t first_molecule;                             /* molecule ids are first_molecule + i, in 0 .. 2^63 - 1 */
    double p;                                           /* the chemistry of FsqPeptideSimParams, one value for all letters */
    double per_cycle_b;
    double u;
    double s, s2;
    double log_beta[FSQ_PEPTIDE_MAX_CHANNELS];          /* per channel: the host's log(beta) */
    double beta_sigma[FSQ_PEPTIDE_MAX_CHANNELS];
    double superdye_rate[FSQ_PEPTIDE_MAX_CHANNELS];     /* 0 .. 1 */
    double superdye_factor[FSQ_PEPTIDE_MAX_CHANNELS];
    double ddif[FSQ_PEPTIDE_MAX_CHANNELS][FSQ_PEPTIDE_MAX_LABELLED];    /* [k][count - 1] is subtracted from the mean */
    int32_t n_ddif[FSQ_PEPTIDE_MAX_CHANNELS];           /* entries of ddif[k] given: at least the bits of channel_mask[k] */
    int32_t n_channels;                                 /* K: 1 .. FSQ_PEPTIDE_MAX_CHANNELS; entries k >= K are not read */
    int32_t length;                                     /* 1 .. FSQ_PEPTIDE_MAX_LENGTH */
    int32_t num_mocks, num_edmans;                      /* >= 0; num_mocks + num_edmans + 1 <= FSQ_PEPTIDE_MAX_FRAMES */
    int32_t sc;                                         /* cycles count from 1 at the first mock */
    int32_t reserved_;
} FsqPeptideLabelsParams;

/* n_molecules molecules, one lane each.  With K = n_channels, frames = num_mocks + num_edmans + 1 and L = the number of
 * labelled residues of the union of the masks, in position order.  The per-channel tables are channel-major: one channel's
 * table is a contiguous [n][frames] block, which fsq_lognormal_fit takes as it is.
 *   d_counts        uint8  [K][n][frames]   popcount(live & channel_mask[k]) after every cycle
 *   d_loss_cycle    uint8  [n][L]           the cycle a labelled residue lost its dye in (0 with cause none)
 *   d_loss_cause    uint8  [n][L]           FSQ_PEPTIDE_CAUSE_*
 *   d_edman_fail    uint64 [n]              bit c: the Edman of cycle c drew and failed
 *   d_intensity     double [K][n][frames]   0.0 where the channel's count is 0
 *   d_log_intensity double [K][n][frames]   glibc's log(I) for I > 0, else FSQ_PEPTIDE_OFF_LOG
 *   d_category      uint64 [K][n]           bit f: the channel's count > 0 at frame f
 *   d_n_draws       int32  [n][1 + 2K]      draws consumed of stream 0, then (superdye stream, normal stream) per channel
 * (d_loss_cycle and d_loss_cause may be null when L = 0.)  An invalid shape or parameter returns FSQ_EINVAL and writes
 * nothing. */
int fsq_peptide_simulate_labels(const FsqPeptideLabelsParams* prm, int64_t n_molecules, uint8_t* d_counts, uint8_t* d_loss_cycle,
                                uint8_t* d_loss_cause, uint64_t* d_edman_fail, double* d_intensity, double* d_log_intensity,
                                uint64_t* d_category, int32_t* d_n_draws, void* stream);

#ifdef __cplusplus
}
#endif
#endif
