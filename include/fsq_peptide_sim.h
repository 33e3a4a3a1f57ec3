/* fsq_peptide_sim.h - C ABI of the peptide Monte-Carlo simulation (libfsq_hip.so, gfx950).
 *
 * peptide_simulator.py's simulate_dye_counts (:44-169, 251-277) and simulate_photometries (:333-353, 405-434, number = 1) for
 * n molecules of one peptide with one label letter: duds, photobleaching, surface loss and Edman cycles, then one lognormal
 * intensity per frame.  The reference is unseeded; here the draws are explicit and everything computed from them has the
 * reference's bits:
 *   Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (block, molecule & 0xffffffff, molecule >> 32, stream);
 *   draw j of a (molecule, stream) pair uses block j >> 1, even j words (0, 1), odd j words (2, 3), and is CPython's
 *   ((a >> 5) * 67108864 + (b >> 6)) / 2^53.  Stream 0: the chemistry; stream 1: the superdye draws; stream 2: the uniforms
 *   of numpy's legacy polar normals, every molecule starting with an empty cache.
 * Conventions are those of fsq_lognormal.h: every entry enqueues on `stream` and does not synchronise, buffers are the
 * caller's, every element of every output row is written, return codes are those of include/fsq.h. */
#ifndef FSQ_PEPTIDE_SIM_H
#define FSQ_PEPTIDE_SIM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_PEPTIDE_MAX_LENGTH 64           /* residues: one bit each in label_mask */
#define FSQ_PEPTIDE_MAX_LABELLED 15         /* FSQ_LOGNORMAL_MAX_POSSIBLE */
#define FSQ_PEPTIDE_MAX_FRAMES 64           /* num_mocks + num_edmans + 1: FSQ_LOGNORMAL_MAX_FRAMES */

#define FSQ_PEPTIDE_CAUSE_NONE 0            /* the dye is still there after the last cycle */
#define FSQ_PEPTIDE_CAUSE_DUD 1
#define FSQ_PEPTIDE_CAUSE_DESTRUCTION 2
#define FSQ_PEPTIDE_CAUSE_EDMAN 3
#define FSQ_PEPTIDE_CAUSE_STRIP 4

#define FSQ_PEPTIDE_OFF_LOG (-10000.0)      /* log_intensity where the intensity is not > 0 (MCsimlib.py:5423) */

typedef struct {
    uint64_t label_mask;                    /* bit i: residue i (0 = N-terminal) is labelled; no bit at or above `length` */
    uint64_t seed;
    int64_t first_molecule;                 /* molecule ids are first_molecule + i, in 0 .. 2^63 - 1 */
    double p;                               /* Edman efficiency */
    double per_cycle_b;                     /* the host's math.e ** -b: a dye survives an exposure when r <= per_cycle_b */
    double u;                               /* dud rate */
    double s, s2;                           /* surface loss per cycle: s while cycle <= sc, then s2 */
    double log_beta;                        /* the host's log(beta) */
    double beta_sigma;
    double superdye_rate;                   /* 0 .. 1 */
    double superdye_factor;
    double ddif[FSQ_PEPTIDE_MAX_LABELLED];  /* [count - 1] is subtracted from the mean at `count` dyes */
    int32_t n_ddif;                         /* entries of ddif given: at least the number of labelled residues */
    int32_t length;                         /* 1 .. FSQ_PEPTIDE_MAX_LENGTH */
    int32_t num_mocks, num_edmans;          /* >= 0; num_mocks + num_edmans + 1 <= FSQ_PEPTIDE_MAX_FRAMES */
    int32_t sc;                             /* cycles count from 1 at the first mock */
    int32_t reserved_;
} FsqPeptideSimParams;

/* n_molecules molecules, one lane each.  With frames = num_mocks + num_edmans + 1 and L = the number of labelled residues:
 *   d_counts        uint8  [n][frames]   dyes left at every frame
 *   d_loss_cycle    uint8  [n][L]        the cycle a labelled residue lost its dye in (0 with cause none)
 *   d_loss_cause    uint8  [n][L]        FSQ_PEPTIDE_CAUSE_*
 *   d_edman_fail    uint64 [n]           bit c: the Edman of cycle c drew and failed
 *   d_intensity     double [n][frames]   0.0 where the count is 0
 *   d_log_intensity double [n][frames]   what fsq_lognormal_fit reads: glibc's log(I) for I > 0, else FSQ_PEPTIDE_OFF_LOG
 *   d_category      uint64 [n]           bit f: count > 0 at frame f
 *   d_n_draws       int32  [n][3]        draws consumed of streams 0, 1 and 2
 * (d_loss_cycle and d_loss_cause may be null when L = 0.)  An invalid shape or parameter returns FSQ_EINVAL and writes
 * nothing. */
int fsq_peptide_simulate(const FsqPeptideSimParams* prm, int64_t n_molecules, uint8_t* d_counts, uint8_t* d_loss_cycle,
                         uint8_t* d_loss_cause, uint64_t* d_edman_fail, double* d_intensity, double* d_log_intensity,
                         uint64_t* d_category, int32_t* d_n_draws, void* stream);

/* d_out[i][0..3] = Philox4x32-10 of counter d_counters[i][0..3] under key d_keys[i][0..1] (the known answers). */
int fsq_philox_words(const uint32_t* d_counters, const uint32_t* d_keys, int64_t n, uint32_t* d_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
