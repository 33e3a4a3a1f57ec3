/* fsq_signal_sweep.h - C ABI of simulation parameter sweeps scored against observed signals (libfsq_hip.so, gfx950).
 *
 * jupyter_development.py's loop over all_simulations = {(p, b, u): (signals, molecular_signals)} (match_diagnostic, :786-948)
 * as one device path: a simulation batched over many parameter points, a signal tally per point that stays on the device,
 * and signal_correlation (:279-578) for every point at once; then match_diagnostic's incompatibility loop over signal pairs
 * (:833-889) on the same count matrix.  Conventions are those of fsq_peptide_sim.h: every entry
 * enqueues on `stream` and does not synchronise (but for fsq_signal_pair_best's check of its rows, see there), buffers are the caller's, return codes are those of include/fsq.h, an
 * invalid shape or parameter returns FSQ_EINVAL and writes nothing.
 *
 * THE SIGNAL KEY.  A row of dye counts (a molecule's counts, or a fit's best_seq), uint8 [frames], has the reference's signal
 * (decrements, last == 0, first).  Its key is exact and 64 bits wide:
 *   bits 0 .. 3           the starting count, 0 .. 15;
 *   bits 4 + 6i .. 9 + 6i the cycle (1 .. 63) of drop i, i = 0 .. 9, ascending (a drop of d dyes stands d times); 0: no drop i,
 *                         and none after it.
 * `last == 0` is not stored: the last count is zero exactly when the number of drops equals the starting count.  A row with
 * more than FSQ_SIGNAL_MAX_DROPS drops, or that starts above 15, has no key (it is counted in d_unkeyed); a row with an
 * upstep has no signal (d_none).  Bit patterns with a drop after a 0 are no row's key: FSQ_SIGNAL_EMPTY marks a free slot
 * and FSQ_SIGNAL_NEVER is a key no table holds. */
#ifndef FSQ_SIGNAL_SWEEP_H
#define FSQ_SIGNAL_SWEEP_H
#include <stdint.h>

#include "fsq_peptide_labels.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_SIGNAL_MAX_DROPS 10
#define FSQ_SIGNAL_MAX_FRAMES 64
#define FSQ_SIGNAL_EMPTY 0x400ull           /* drop 0 absent, drop 1 at cycle 1 */
#define FSQ_SIGNAL_NEVER 0x800ull           /* drop 0 absent, drop 1 at cycle 2 */
#define FSQ_SIGNAL_MAX_SLOTS (1 << 24)

typedef struct {
    double p;                               /* Edman efficiency */
    double per_cycle_b;                     /* a dye survives an exposure when r <= per_cycle_b */
    double u;                               /* dud rate */
    double s, s2;                           /* surface loss per cycle: s while cycle <= sc, then s2 */
} FsqSweepPoint;

/* fsq_peptide_simulate for n_points parameter points of n_per_point molecules each: rows first_row .. first_row + n_rows - 1
 * of the flattened [n_points][n_per_point] space, one lane per row.  Row g belongs to point k = g / n_per_point and is
 * molecule base->first_molecule + k * molecule_stride + g % n_per_point, simulated with d_points[k] in place of base's p,
 * per_cycle_b, u, s and s2 and everything else from `base`: what fsq_peptide_simulate writes for that molecule under those
 * parameters, bit for bit.  molecule_stride = 0: every point sees the same draws (common random numbers).
 *   d_points    FsqSweepPoint [n_points]  device memory; its values are the caller's to check (they are only compared with draws)
 *   d_counts    uint8  [n_rows][frames]
 *   d_intensity double [n_rows][frames]
 *   d_category  uint64 [n_rows]
 * Needs n_points >= 1, n_per_point >= 1, molecule_stride >= 0, 0 <= first_row, n_rows >= 0, first_row + n_rows <=
 * n_points * n_per_point, and every molecule id within 0 .. 2^63 - 1. */
int fsq_peptide_simulate_points(const FsqPeptideSimParams* base, const FsqSweepPoint* d_points, int64_t n_points,
                                int64_t n_per_point, int64_t molecule_stride, int64_t first_row, int64_t n_rows,
                                uint8_t* d_counts, double* d_intensity, uint64_t* d_category, void* stream);

/* Adds the signals of n_rows rows to the tables of their points.
 *   d_rows      uint8 [n_rows][frames], 1 <= frames <= FSQ_SIGNAL_MAX_FRAMES
 *   d_point     int32 [n_rows]          the row's point; a row whose point is not in 0 .. n_points - 1 is left out
 *   d_valid     uint8 [n_rows] or null  rows with 0 are left out
 *   d_keys      uint64 [n_points][slots], d_counts int64 [n_points][slots]: one open-addressing table per point, `slots` a
 *               power of two up to FSQ_SIGNAL_MAX_SLOTS.  Before the first call the caller fills d_keys with FSQ_SIGNAL_EMPTY and
 *               d_counts, d_none, d_unkeyed and d_overflow with 0; calls accumulate.
 *   d_none      int64 [n_points]        rows with an upstep
 *   d_unkeyed   int64 [n_points]        rows without a key (more than FSQ_SIGNAL_MAX_DROPS drops, a start above 15)
 *   d_overflow  int32 [n_points]        set to 1 when a row of the point found no slot: its table then misses counts
 * A slot is claimed or matched by one 64-bit compare-and-swap and the count added by an integer atomic add; every probe
 * loop is bounded by `slots`; no lane waits for another's store.  Counts are integers: the tables' contents as sets of
 * (key, count) do not depend on arrival order (where a key sits does). */
int fsq_signal_tally(const uint8_t* d_rows, int32_t frames, const int32_t* d_point, const uint8_t* d_valid, int64_t n_rows,
                     int32_t n_points, int32_t slots, uint64_t* d_keys, int64_t* d_counts, int64_t* d_none, int64_t* d_unkeyed,
                     int32_t* d_overflow, void* stream);

/* THE JOINT KEY.  A molecule seen in K colour channels (K = 1 .. FSQ_PEPTIDE_MAX_CHANNELS label letters, in sorted-letter
 * order) has K count rows and the joint signal (decrements, zeros, starts) of peptide_simulator.joint_signal - a definition
 * of this package, the reference stops at one letter.  Its key is again exact and 64 bits wide, so that fsq_signal_lookup,
 * fsq_signal_scores, fsq_signal_pair_best and fsq_signal_pair_extremes serve it as they are.  With B = 6 + ceil(log2 K) bits
 * per drop (6, 7, 8, 8):
 *   bits 0 .. 3                     the starting count of channel 0;
 *   bits 4 + B i .. 3 + B (i + 1)   drop i: the low 6 bits its cycle (1 .. 63), the bits above its channel; 0: no drop i, and
 *                                   none after it.  Drops ascend by (cycle, channel); a drop of d dyes stands d times;
 *   bits 64 - 4 (K - k) .. 67 - 4 (K - k)   the starting count of channel k = 1 .. K - 1: the top nibbles.
 * The drop capacity D(K) = FSQ_SIGNAL_JOINT_MAX_DROPS(K) is 10, 8, 6, 6.  With K = 1 this is the key above, bit for bit.
 * `zeros` is not stored: a channel ends at zero exactly when its drops number its starting count.  FSQ_SIGNAL_EMPTY and
 * FSQ_SIGNAL_NEVER are no molecule's key for any K: bit 10 or 11 alone is a drop field whose cycle is 0 (K >= 2: bit 10 is a
 * channel bit of drop 0; bit 11 is one too for K >= 3) or a drop that follows an absent one (K = 2: bit 11 is cycle 1 of drop
 * 1 with drop 0 absent).  A molecule with more than D(K) drops in all, or a channel that starts above 15, has no key
 * (d_unkeyed); one with an upstep in any channel has no signal (d_none).  A 128-bit key would lift the drop cap and need
 * lookup, score and pair kernels of its own. */
#define FSQ_SIGNAL_JOINT_DROP_BITS(K) ((K) <= 1 ? 6 : (K) == 2 ? 7 : 8)
#define FSQ_SIGNAL_JOINT_MAX_DROPS(K) ((K) <= 1 ? 10 : (K) == 2 ? 8 : 6)

/* fsq_signal_tally for molecules of n_channels colour channels: the joint key of each molecule's n_channels rows.
 *   d_rows      uint8 [n_channels][n_rows][frames], channel-major: what fsq_peptide_simulate_labels and
 *               fsq_peptide_simulate_labels_points write, and what n_channels lognormal fits fill
 * and every other argument as fsq_signal_tally takes it, with the same tables and the same guarantees: bounded probe loops,
 * one 64-bit compare-and-swap per probe, no lane waits for another's store, an overflow sets d_overflow and costs a count.
 * With n_channels = 1 it leaves the (key, count) sets fsq_signal_tally leaves. */
int fsq_signal_tally_joint(const uint8_t* d_rows, int32_t n_channels, int32_t frames, const int32_t* d_point, const uint8_t* d_valid,
                           int64_t n_rows, int32_t n_points, int32_t slots, uint64_t* d_keys, int64_t* d_counts, int64_t* d_none,
                           int64_t* d_unkeyed, int32_t* d_overflow, void* stream);

/* fsq_peptide_simulate_labels over the flattened [n_points][n_per_point] space, as fsq_peptide_simulate_points is
 * fsq_peptide_simulate over it: the same row-to-(point, molecule) rule, the same molecule_stride, first_row and n_rows, and
 * d_points[k] in place of base's p, per_cycle_b, u, s and s2.  Only three tables are written, channel-major over the call's
 * rows, K = base->n_channels:
 *   d_counts    uint8  [K][n_rows][frames]
 *   d_intensity double [K][n_rows][frames]
 *   d_category  uint64 [K][n_rows]
 * each what fsq_peptide_simulate_labels writes for that molecule under that point's parameters, bit for bit; with K = 1 what
 * fsq_peptide_simulate_points writes.  Defined in fsq_peptide_labels.hip.  A shape whose staging would need more LDS than a
 * launch gets without an attribute (64 KiB) returns FSQ_EINVAL; none within the limits of fsq_peptide_labels.h does. */
int fsq_peptide_simulate_labels_points(const FsqPeptideLabelsParams* base, const FsqSweepPoint* d_points, int64_t n_points,
                                       int64_t n_per_point, int64_t molecule_stride, int64_t first_row, int64_t n_rows,
                                       uint8_t* d_counts, double* d_intensity, uint64_t* d_category, void* stream);

/* d_out[w][k] = the count of key d_wanted[w] in point k's table, 0 where it is absent: int64 [n_wanted][n_points]. */
int fsq_signal_lookup(const uint64_t* d_keys, const int64_t* d_counts, int32_t n_points, int32_t slots, const uint64_t* d_wanted,
                      int32_t n_wanted, int64_t* d_out, void* stream);

#define FSQ_SCORE_NAIVE 0
#define FSQ_SCORE_MY_EUCLIDEAN 1
#define FSQ_SCORE_NORMALIZED_EUCLIDEAN 2
#define FSQ_SCORE_MY_STD_NORMALIZED_EUCLIDEAN 3
#define FSQ_SCORE_MY_SIM_STD_NORMALIZED_EUCLIDEAN 4
#define FSQ_SCORE_LOG_RMSD 5
#define FSQ_SCORE_MY_CANBERRA 6
#define FSQ_SCORE_MY_CHEBYSHEV 7
#define FSQ_SCORE_MY_NORMALIZED_CHEBYSHEV 8
#define FSQ_SCORE_MY_STD_NORMALIZED_CHEBYSHEV 9
#define FSQ_SCORE_N_METRICS 10

#define FSQ_SCORE_NORMALIZE_COUNTS 1        /* bits of `normalization`; with both, normalize_counts wins where it applies */
#define FSQ_SCORE_HEATMAP_NORMALIZE_COUNTS 2

#define FSQ_SCORE_OK 0
#define FSQ_SCORE_EMPTY 1                   /* nothing pairs: the reference returns None (the factor is still written) */
#define FSQ_SCORE_DIVZERO 2                 /* the reference raises ZeroDivisionError */
#define FSQ_SCORE_DOMAIN 3                  /* the reference raises ValueError: a maximum of nothing, a root of a negative */

typedef struct {
    int64_t n_observed;                     /* the std metrics' n: the observed counts that pass zero_only and allow_multidrop.
                                             * 0 .. 2^31 - 1, as every count: beyond it fsq_signal_scores returns FSQ_EINVAL. */
    double small_count_cutoff;              /* read when has_cutoff != 0 */
    int32_t has_cutoff;
    int32_t normalization;                  /* FSQ_SCORE_NORMALIZE_COUNTS | FSQ_SCORE_HEATMAP_NORMALIZE_COUNTS */
    int32_t metric;                         /* FSQ_SCORE_* */
    int32_t reserved_;
} FsqScoreParams;

/* signal_correlation (:279-578) of one observed dict against n_points fit dicts over n_keys keys in ascending key order,
 * one lane per point, every sum left to right in that order.
 *   d_observed     int64 [n_keys]            0 .. 2^31 - 1
 *   d_in_observed  uint8 [n_keys]            the key is in the observed dict
 *   d_admitted     uint8 [n_keys]            the key passes select_signals, zero_only, heatmap_only, allow_multidrop, exclude_signals
 *   d_heatmap      uint8 [n_keys]            the key counts for heatmap_normalize_counts (z, one or two distinct drops)
 *   d_fit          int64 [n_keys][n_points]  0 .. 2^31 - 1; a key is in point k's fit dict when its count is positive
 *   d_fit_total    int64 [n_points]          the sum of point k's whole fit dict (my_sim_std_normalized_euclidean's n)
 *   d_score, d_factor double [n_points], d_status int32 [n_points]; d_contrib double [n_keys][n_points] or null: NaN where
 *   the key has no contribution.
 * A key is paired for a point when it is admitted and in the observed dict or the point's fit dict, and passes the cutoff.
 * d_score is written only with FSQ_SCORE_OK (else NaN); d_factor whenever the reference has computed it (else NaN).
 * Choosing among the points is the caller's: signal_sweep.best_point takes the smallest (or largest) score, the first point
 * in grid order among equal ones (the reference: the first in its dict's order), and never a point without a score. */
int fsq_signal_scores(const int64_t* d_observed, const uint8_t* d_in_observed, const uint8_t* d_admitted, const uint8_t* d_heatmap,
                      const int64_t* d_fit, const int64_t* d_fit_total, int32_t n_keys, int32_t n_points,
                      const FsqScoreParams* prm, double* d_score, double* d_factor, int32_t* d_status, double* d_contrib,
                      void* stream);

/* The complete candidate list of 63 cycles (the key's highest cycle) is 63 single and 63 * 62 / 2 double drops: 2 016 signals
 * and 2 031 120 pairs.  The cap lies above it, and keeps every pair and distance index within 32 bits. */
#define FSQ_SIGNAL_PAIR_MAX_SEL 2048

/* match_diagnostic's incompatibility loop (:838-874) for all pairs of n_sel candidate signals at once.  Pair t = (i, j), i < j,
 * in itertools.combinations' order: t = i (2 n_sel - i - 1) / 2 + j - i - 1, K = n_sel (n_sel - 1) / 2 pairs.  For pair t
 * and point k the result is what fsq_signal_scores gives at k when d_admitted is ANDed with the two keys d_rows[i] and
 * d_rows[j] (:845-859, select_signals = {ss1, ss2}): the same pairing, cutoff, factor, terms and statuses.  The best point of
 * the pair (:861-869) is the one with the smallest result, or the largest with reverse_order != 0; among equal results the
 * lowest point, and never a point that is not FSQ_SCORE_OK.
 *   d_observed .. d_fit_total, n_keys, n_points, prm   as fsq_signal_scores takes them
 *   d_rows         int32 [n_sel]      the row of each candidate in the key table, -1: in no dict (never paired); rows >= 0
 *                                     are distinct (the caller's to see to: a row standing twice is counted twice)
 *   d_heat_factor  double [n_points], d_heat_status int32 [n_points]: read when prm->normalization has
 *                  FSQ_SCORE_HEATMAP_NORMALIZE_COUNTS, else may be null.  The point's heat-map factor does not depend on the
 *                  pair: it is d_factor and d_status of one fsq_signal_scores call with an all-zero d_admitted (status
 *                  FSQ_SCORE_EMPTY with the factor, or FSQ_SCORE_DIVZERO).
 *   d_best_point   int32 [K]          -1: no point has a result
 *   d_result, d_factor double [K]     at the best point, NaN without one
 *   d_dist         double [K][2]      the contributions of i and of j at the best point (:871); NaN: none
 *   d_error_point  int32 [K]          the lowest point that ends FSQ_SCORE_DIVZERO or FSQ_SCORE_DOMAIN (the reference raises
 *                                     out of its loop there), -1: none;  d_error_status int32 [K]: its status, 0 without one
 * Every output element is written on every call.  One wavefront per pair, lanes strided over the points; no atomics, no lane
 * reads another's store, every loop is bounded by n_points.  Needs 2 <= n_sel <= FSQ_SIGNAL_PAIR_MAX_SEL, n_points >= 1,
 * n_keys >= 0 and every row within -1 .. n_keys - 1 (d_rows is read back to check it: this entry synchronises `stream`
 * before it launches). */
int fsq_signal_pair_best(const int64_t* d_observed, const uint8_t* d_in_observed, const uint8_t* d_admitted, const int64_t* d_fit,
                         const int64_t* d_fit_total, int32_t n_keys, int32_t n_points, const FsqScoreParams* prm,
                         const int32_t* d_rows, int32_t n_sel, int32_t reverse_order, const double* d_heat_factor,
                         const int32_t* d_heat_status, int32_t* d_best_point, double* d_result, double* d_factor, double* d_dist,
                         int32_t* d_error_point, int32_t* d_error_status, void* stream);

/* The per-signal incompatibility score (:875-889): for each of the n_sel candidates the maximum of its distances over its
 * n_sel - 1 pairs, or the minimum with reverse_order != 0, NaN skipped in both directions.
 *   d_dist         double [K][2]      fsq_signal_pair_best's
 *   d_score        double [n_sel]     NaN: the candidate has no distance (the reference leaves it out of its dict)
 *   d_n_distances  int32  [n_sel]     how many of its n_sel - 1 distances are not NaN
 * One wavefront per candidate, a fixed reduction tree, no atomics: the same bits on every run.  Needs 2 <= n_sel <=
 * FSQ_SIGNAL_PAIR_MAX_SEL. */
int fsq_signal_pair_extremes(const double* d_dist, int32_t n_sel, int32_t reverse_order, double* d_score, int32_t* d_n_distances,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif
