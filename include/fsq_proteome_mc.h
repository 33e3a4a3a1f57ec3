/* fsq_proteome_mc.h - C ABI of the proteome-scale Monte-Carlo (libfsq_hip.so, gfx950).
 *
 * The reference's MCsimlib.py samples every attached peptide of a proteome sample_size times with random_signal (:863-1074),
 * counts the signals per source protein in a SignalTrie (:1224-1281) and asks find_uniques (:1398-1486) which signals point
 * to one protein.  Here that is three entries on the device: the signals as 64-bit keys, the (signal, protein) counts in two
 * open-addressing tables, and the scan of find_uniques over the sorted counts.  A fourth, fsq_proteome_project, folds a
 * tally onto what shorter runs would have shown (truncating_projection, :1697-1759) for many cycle counts at once, and adds one
 * tally into another (merge, :1674-1696).  Conventions are those of
 * fsq_signal_sweep.h: every entry enqueues on `stream` and does not synchronise, buffers are the caller's, return codes are
 * those of include/fsq.h, an invalid shape or parameter returns FSQ_EINVAL and writes nothing.
 *
 * THE KEY.  A signal is a set of (position, acid) pairs.  Per acid a, with windows W_a (bit x: position x, 1 .. 63):
 * exposures E_a = W_a | (W_a >> 1), observable positions O_a = E_a & (E_a << 1); the pair (x, a) is key bit
 * base_a + popcount(O_a & ((1 << x) - 1)), base_a the number of observable positions of the acids before a.  The sum of
 * popcount(O_a) is at most 64.  Key 0 is the empty signal: the reference's trie does not store it (add_descendant returns on
 * length 0, :1268), so 0 marks a free slot of the signal table.
 *
 * THE DRAWS.  Row g of the flattened [peptides][sample_size] space is sample first_sample + g and reads stream 3 of that
 * item under `seed` (fsq_philox.h: counter (draw >> 1, item lo, item hi, 3)), in the order of the reference's
 * random.random() calls: the dud draws of the labels in "for acid: head occurrences by position, then tail occurrences",
 * then one Edman draw per surviving head label by position, then one bleach draw per surviving head label, then one per
 * surviving tail label acid-major. */
#ifndef FSQ_PROTEOME_MC_H
#define FSQ_PROTEOME_MC_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_PMC_STREAM 3
#define FSQ_PMC_MAX_ACIDS 8
#define FSQ_PMC_MAX_LABELS 64               /* labelled residues of a peptide, head and tail together */
#define FSQ_PMC_MAX_HEAD 255
#define FSQ_PMC_MAX_ROW 4096                /* entries of an Edman delay row: a search of at most 12 steps */
#define FSQ_PMC_MAX_EXPOSURES 64
#define FSQ_PMC_MAX_SIGNAL_SLOTS (1 << 27)
#define FSQ_PMC_MAX_PAIR_SLOTS (1 << 28)
#define FSQ_PMC_PAIR_EMPTY 0xffffffffffffffffull

typedef struct {
    uint64_t E[FSQ_PMC_MAX_ACIDS];          /* exposures of an acid, bit x: after Edman cycle x (0: before any) */
    uint64_t O[FSQ_PMC_MAX_ACIDS];          /* observable positions */
    int32_t base[FSQ_PMC_MAX_ACIDS];        /* first key bit of the acid */
    int32_t n_acids;
    int32_t max_d;                          /* rows of the Edman table: d = 1 .. max_d */
    double u;                               /* a label is a dud unless its draw is above u */
    uint64_t seed;
    uint64_t first_sample;
    int64_t sample_size;
} FsqProteomeParams;

/* random_signal (:863-1074) for rows first_row .. first_row + n_rows - 1 of the flattened [n_peptides][sample_size] space,
 * one lane per row.
 *   d_protein      int32  [n_peptides]       the peptide's protein
 *   d_n_head       int32  [n_peptides]       its head labels
 *   d_label_start  int64  [n_peptides + 1]   CSR into d_labels; at most FSQ_PMC_MAX_LABELS labels per peptide
 *   d_labels       uint32 [total]            walk order (head labels by position, then tail labels acid-major); entry k: bits
 *                                            0-7 position (1 .. 255; 0: tail), 8-15 acid, 16-23 the label's dud draw, 24-29 the
 *                                            walk index of the label whose dud draw is k
 *   d_edman_start  int64  [max_d + 2], d_edman double: row d = d_edman[start[d] .. start[d + 1]), the running sums of
 *                  _dp(d, e, p) (:42-53) as the loop of :979-989 forms them, at most FSQ_PMC_MAX_ROW each; the delay of a draw r
 *                  is the first e with row[e] >= r, else the row's length
 *   d_bleach       double [FSQ_PMC_MAX_EXPOSURES]  T[s] = (sum k <= s of e^(-b k)) (1 - e^-b) (:1035-1038)
 *   d_key          uint64 [n_rows]           the signal's key, 0 for the empty signal
 *   d_row_protein  int32  [n_rows] or null   the row's protein
 *   d_n_draws      int32  [n_rows] or null   the draws the row consumed
 * The tables are the caller's to build (the host twin's edman_table / bleach_table): the device calls no exp or pow.  Every
 * head label's position must be within 1 .. max_d and ascending within a peptide, every acid below n_acids. */
int fsq_proteome_signals(const FsqProteomeParams* prm, const int32_t* d_protein, const int32_t* d_n_head,
                         const int64_t* d_label_start, const uint32_t* d_labels, int64_t n_peptides, const int64_t* d_edman_start,
                         const double* d_edman, const double* d_bleach, int64_t first_row, int64_t n_rows, uint64_t* d_key,
                         int32_t* d_row_protein, int32_t* d_n_draws, void* stream);

/* SignalTrie.add_descendant (:1252-1281) for n_rows (key, protein) rows: rows with key 0 or a negative protein are counted
 * nowhere.
 *   d_signals      uint64 [signal_slots]     table A, key -> slot; 0 is free.  signal_slots a power of two
 *   d_pairs        uint64 [pair_slots]       table B, (slot of A << 32 | protein) -> count; FSQ_PMC_PAIR_EMPTY is free
 *   d_counts       int64  [pair_slots]
 *   d_overflow     int32  [2]                [0]: a row found no slot in A, [1]: none in B; the tables then miss counts
 * Before the first call the caller fills d_signals, d_counts and d_overflow with 0 and d_pairs with all ones; calls accumulate.
 * A slot is claimed or matched by one 64-bit compare-and-swap whose old value tells which, the count is an integer atomic
 * add; every probe loop is bounded by the table's size and no lane waits for another's store. */
int fsq_proteome_tally(const uint64_t* d_key, const int32_t* d_row_protein, int64_t n_rows, uint64_t* d_signals,
                       int64_t signal_slots, uint64_t* d_pairs, int64_t* d_counts, int64_t pair_slots, int32_t* d_overflow,
                       void* stream);

#define FSQ_PMC_PROJECT 0                   /* insert key & mask: truncating_projection (:1697-1759) */
#define FSQ_PMC_WITHIN 1                    /* insert key where key & ~mask == 0: merge's cycles= filter (:1694) */
#define FSQ_PMC_MASK_MAJOR 0x100            /* or-ed into the mode: item t is pair t % n under mask t / n, not pair t / n_masks under
                                               mask t % n_masks.  The tables do not depend on it; it is there to be timed */
#define FSQ_PMC_MAX_MASKS 4096

/* The counted pairs (d_key[i], d_protein[i], d_count[i]) under each of n_masks masks, one lane per (pair, mask) item: table m of
 * [n_masks][signal_slots] / [n_masks][pair_slots] receives the pair's key as `mode` and d_mask[m] turn it.  The mask of cycle
 * count c holds the key bits of the pairs (x, a) with x <= c: per acid, bits base_a .. base_a + popcount(O_a & ((1 << (c + 1))
 * - 1)) - 1, so key & mask is the signal a run of c cycles would have shown.
 *   d_key uint64 [n], d_protein int32 [n], d_count int64 [n] or null (every weight 1), d_mask uint64 [n_masks]
 *   d_signals uint64 [n_masks][signal_slots], d_pairs uint64 [n_masks][pair_slots], d_counts int64 [n_masks][pair_slots],
 *   d_overflow int32 [n_masks][2]
 * Table m has the slot format of fsq_proteome_tally and is prepared as there; calls accumulate, and fsq_proteome_tally may go on
 * adding to it.  An item whose turned key is 0, whose protein is negative or whose weight is 0 is counted nowhere.  The count
 * is one 64-bit integer atomic add of the weight; probe loops are bounded by the table's size; a full table sets
 * d_overflow[m][0] (signals) or [m][1] (pairs), loses that item and leaves the other masks exact.  Null pointers (d_count
 * aside), n_masks outside 1 .. FSQ_PMC_MAX_MASKS, slot counts that are no power of two within the limits above or an unknown
 * mode return FSQ_EINVAL and write nothing; n == 0 returns FSQ_OK. */
int fsq_proteome_project(const uint64_t* d_key, const int32_t* d_protein, const int64_t* d_count, int64_t n, const uint64_t* d_mask,
                         int64_t n_masks, int32_t mode, uint64_t* d_signals, int64_t signal_slots, uint64_t* d_pairs,
                         int64_t* d_counts, int64_t pair_slots, int32_t* d_overflow, void* stream);

#define FSQ_PMC_RATIO_NONE 0               /* worst_ratio is None: passes only without a second */
#define FSQ_PMC_RATIO_NUMBER 1
#define FSQ_PMC_RATIO_ABSENT 2              /* find_uniques_absolute: no ratio clause, second_count <= maximum_secondary */

typedef struct {
    double worst_ratio, absolute_min, maximum_secondary;
    int32_t ratio_mode;                     /* FSQ_PMC_RATIO_* */
    int32_t has_maximum_secondary;
    int32_t demote;                         /* 0: the reference's scan; 1: the true top two (an extension) */
    int32_t reserved_;
} FsqUniquesParams;

/* The scan of find_uniques (:1436-1474) and find_uniques_absolute (:1497-1514), one lane per signal over its proteins in
 * ascending protein index.
 *   d_protein int32 [n_pairs], d_count int64 [n_pairs]: the (signal, protein) counts sorted by (signal, protein)
 *   d_segment int64 [n_signals + 1]: signal i owns pairs d_segment[i] .. d_segment[i + 1] - 1 (at least one)
 *   d_best_protein int32, d_best_count int64, d_second_protein int32 (-1: None), d_second_count int64, d_n_ties int32 (further
 *   proteins listed with second), d_tertiary int64, d_passed uint8: [n_signals] each. */
int fsq_proteome_uniques(const int32_t* d_protein, const int64_t* d_count, const int64_t* d_segment, int64_t n_signals,
                         const FsqUniquesParams* prm, int32_t* d_best_protein, int64_t* d_best_count, int32_t* d_second_protein,
                         int64_t* d_second_count, int32_t* d_n_ties, int64_t* d_tertiary, uint8_t* d_passed, void* stream);

/* ---- a grid of (p, b, u) points over the same peptides (csrc/simulate/fsq_proteome_points.hip) ---- */

#define FSQ_PMC_MAX_POINTS 4096

typedef struct {
    double u;                               /* in place of FsqProteomeParams.u */
    int32_t edman_table;                    /* the point's p: a table of d_edman_start, 0 .. n_edman_tables - 1 */
    int32_t bleach_table;                   /* the point's b: a table of d_bleach, 0 .. n_bleach_tables - 1 */
} FsqProteomePoint;

/* fsq_proteome_signals for n_points points at once, one lane per (point, row): rows first_row .. first_row + n_rows - 1 of the
 * [n_peptides][sample_size] space, the same for every point.  Row g of point k is sample base->first_sample + k * sample_stride
 * + g, reads stream 3 of that item under base->seed and uses d_points[k].u, Edman table d_points[k].edman_table and bleach table
 * d_points[k].bleach_table in place of base->u (which is not read) and the single tables.  sample_stride = 0: every point sees
 * the same draws (common random numbers).  d_key[k][t] and d_n_draws[k][t] are what fsq_proteome_signals writes for that sample
 * under that point's parameters, bit for bit: both kernels run the same per-sample body (csrc/simulate/fsq_proteome_lane.h).
 *   d_points       FsqProteomePoint [n_points]
 *   the peptide table (d_protein .. n_peptides) as fsq_proteome_signals takes it
 *   d_edman_start  int64  [n_edman_tables][max_d + 2]  offsets into d_edman: row d of table e is d_edman[start[e][d] ..
 *                  start[e][d + 1]); all tables are built with the same base->max_d
 *   d_bleach       double [n_bleach_tables][FSQ_PMC_MAX_EXPOSURES]
 *   d_key          uint64 [n_points][n_rows]
 *   d_row_protein  int32  [n_rows] or null   the row's protein (the same for every point)
 *   d_n_draws      int32  [n_points][n_rows] or null
 * A point's table indices are device data the entry cannot check: the kernel clamps them into 0 .. n_tables - 1, so a wrong
 * index gives wrong keys and never a read outside the tables.  n_points outside 1 .. FSQ_PMC_MAX_POINTS, a negative
 * sample_stride, sample ids beyond 2^64 - 1, fewer than one table of a kind, n_points * n_rows beyond int64, null pointers
 * (d_row_protein and d_n_draws aside) and what fsq_proteome_signals refuses return FSQ_EINVAL and write nothing; n_rows == 0
 * returns FSQ_OK. */
int fsq_proteome_signals_points(const FsqProteomeParams* base, const FsqProteomePoint* d_points, int64_t n_points,
                                int64_t sample_stride, const int32_t* d_protein, const int32_t* d_n_head,
                                const int64_t* d_label_start, const uint32_t* d_labels, int64_t n_peptides,
                                const int64_t* d_edman_start, const double* d_edman, int32_t n_edman_tables, const double* d_bleach,
                                int32_t n_bleach_tables, int64_t first_row, int64_t n_rows, uint64_t* d_key, int32_t* d_row_protein,
                                int32_t* d_n_draws, void* stream);

/* fsq_proteome_tally for n_points points at once, one lane per (point, row): element t of point k (d_key[k][t], d_row_protein[t])
 * goes into table k of d_signals [n_points][signal_slots], d_pairs / d_counts [n_points][pair_slots], d_overflow [n_points][2].
 * Table k has the slot format of fsq_proteome_tally and is prepared as there; calls accumulate, and fsq_proteome_tally and
 * fsq_proteome_project read and extend a point's tables as they are.  A full table of point k sets d_overflow[k][0] (signals) or
 * [k][1] (pairs), loses that row and leaves every other point exact.  With n_points = 1 the (key, count) sets are
 * fsq_proteome_tally's.  n_points outside 1 .. FSQ_PMC_MAX_POINTS, slot counts that are no power of two within the limits above,
 * n_points * n_rows beyond int64 and null pointers return FSQ_EINVAL and write nothing; n_rows == 0 returns FSQ_OK. */
int fsq_proteome_tally_points(const uint64_t* d_key, const int32_t* d_row_protein, int64_t n_points, int64_t n_rows,
                              uint64_t* d_signals, int64_t signal_slots, uint64_t* d_pairs, int64_t* d_counts, int64_t pair_slots,
                              int32_t* d_overflow, void* stream);

#ifdef __cplusplus
}
#endif
#endif
