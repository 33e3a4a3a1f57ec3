/* fsq_background.h - C ABI of the iterative background correction of signal counts (libfsq_hip.so, gfx950).
 *
 * MCsimlib.iterative_peak_finding_v3 (:5932-6019, what iterative_background_v2.py runs) for P independent problems in one call.
 * A problem is one boc- signals dict against the average and the standard deviation of ac- control experiments.  Conventions
 * are those of fsq_remainder.h: buffers are the caller's, return codes are those of include/fsq.h.  Unlike its siblings
 * fsq_background_iterate synchronises `stream`: it enqueues FSQ_BACKGROUND_BATCH_PASSES passes at a time and reads the
 * problems' done flags after each batch.
 *
 * Order (the contract): dicts are walked in insertion order.  The key universe of a problem is its boc keys
 * in insertion order, then the keys the first pass inserts (ac- keys with std 0 that boc lacks), in ac order.  Every list
 * below is in the order the reference walks it under that contract.
 *
 * A key ((label, pos_0), ..., (label, pos_{d-1})), is_zero = True, starting_intensity) is one 64-bit code:
 *   bits 8 i .. 8 i + 7   pos_i, 0 <= pos_i <= FSQ_BACKGROUND_MAX_POSITION, i < d
 *   bits 48 .. 50         d, 1 <= d <= FSQ_BACKGROUND_MAX_DROPS
 *   bits 51 .. 62         the group of the key: one number per distinct starting_intensity, < FSQ_BACKGROUND_MAX_GROUPS
 * The neighbours of a key are the codes of pos + e for e in itertools.product((-1, 0, 1), repeat=d), e != 0, in that order,
 * every 0 < pos_i + e_i <= num_cycles, without a repeated position when multidrop is excluded (:5722-5768).
 *
 * One pass (:5947-6017), all in float64, every operation rounded on its own:
 *   z_i      = copysign(sqrt(pow(bp - ap, 2.0) / pow(sp, 2.0)), bp - ap) of every defined key (sp != 0), bp its percent
 *              as the previous pass left it (0 for a key that has none), pow glibc's
 *   count_u  = np.mean of the counts of u's neighbours (absent: 0; numpy's pairwise sum / n), for every undefined key in
 *              order, each seeing what the ones before it wrote
 *   total    = the counts of the filtered keys added from 0.0 in order, percent = count / total
 *   stop     FSQ_BACKGROUND_NO_DEFINED without a defined key; FSQ_BACKGROUND_THRESHOLD when the first-in-order largest z
 *              is <= sigma_threshold (Python's max: a NaN in first place stays, a NaN elsewhere never wins)
 *   trial k  for every defined key with not (z_k <= sigma_threshold): its interpolated count in place of its count, the
 *              total re-added value by value, diff_k = z_k - z(interpolated / total_k)
 *   stop     FSQ_BACKGROUND_NO_IMPROVEMENT when the first-in-order largest diff is <= 0
 *   accept   the winner's count becomes its interpolated count
 *   stop     FSQ_BACKGROUND_CONVERGED when no count differs by 0.001 or more from the state after the previous accepted
 *              pass (the percents stay those before the acceptance, as in the reference)
 *   percent  = count / total of the winner's trial
 * FSQ_BACKGROUND_MAX_ITERATIONS ends a problem that has run max_iterations passes; FSQ_BACKGROUND_ZERO_TOTAL one whose
 * filtered counts, or those of one of its trials, add up to 0 (the reference's ZeroDivisionError). */
#ifndef FSQ_BACKGROUND_H
#define FSQ_BACKGROUND_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FSQ_BACKGROUND_MAX_DROPS 6          /* drops per key: 3^6 - 1 = 728 neighbours at most */
#define FSQ_BACKGROUND_MAX_POSITION 250     /* positions 0 .. 250: a neighbour's position fits 8 bits */
#define FSQ_BACKGROUND_MAX_GROUPS 4096      /* distinct starting intensities per problem */
#define FSQ_BACKGROUND_BATCH_PASSES 16      /* passes enqueued between two reads of the done flags */
#define FSQ_BACKGROUND_TRIAL_THREADS 64     /* trials per workgroup of the trial kernel: one wavefront */
#define FSQ_BACKGROUND_TILE 1024            /* counts per LDS tile of the base sum */

#define FSQ_BACKGROUND_RUNNING 0
#define FSQ_BACKGROUND_NO_DEFINED 1
#define FSQ_BACKGROUND_THRESHOLD 2
#define FSQ_BACKGROUND_NO_IMPROVEMENT 3
#define FSQ_BACKGROUND_CONVERGED 4
#define FSQ_BACKGROUND_MAX_ITERATIONS 5
#define FSQ_BACKGROUND_ZERO_TOTAL 6

#define FSQ_BACKGROUND_OVERFLOW_ACCEPTED 1  /* more accepted replacements than accepted_cap */
#define FSQ_BACKGROUND_OVERFLOW_UNDEFINED 2 /* more undefined records than undefined_cap */

/* Every pointer is a device pointer.  N keys, D defined entries, U1 / U2 undefined entries over all P problems. */
typedef struct FsqBackgroundArgs {
    int32_t n_problems;                     /* P >= 0 */
    int32_t max_iterations;                 /* >= 0: passes per problem */
    int32_t max_defined;                    /* the largest def_off[p + 1] - def_off[p]: sizes the trial launch */
    int32_t accepted_cap;                   /* >= 0: entries of accepted_key per problem */
    int32_t undefined_cap;                  /* >= 0: entries of undefined_bp per problem */
    int32_t reserved_;
    int64_t n_keys, n_defined, n_first, n_rest, n_neighbours;      /* N, D, U1, U2, nb_off[N] */
    const int64_t* key_off;                 /* [P + 1] keys key_off[p] .. key_off[p + 1] - 1 are problem p's universe */
    const int64_t* def_off;                 /* [P + 1] into the defined lists */
    const int64_t* first_off;               /* [P + 1] into und_first */
    const int64_t* rest_off;                /* [P + 1] into und_rest */
    const int32_t* num_cycles;              /* [P] */
    const int32_t* include_multidrop;       /* [P] 1 or 0 */
    const double* sigma_threshold;          /* [P] */
    const uint64_t* code;                   /* [N] */
    const uint64_t* sorted_code;            /* [N] each problem's codes ascending */
    const int32_t* sorted_index;            /* [N] the index within its problem of each sorted code */
    const uint8_t* filter;                  /* [N] 1: the key enters total and percent (:5640-5654) */
    const int64_t* nb_off;                  /* [N + 1] room in the neighbour table: 3^d - 1 entries per key, ascending */
    const int32_t* def_key;                 /* [D] the defined keys in ac order: index within the problem, -1 for a key that
                                               the universe lacks (bp = 0; never a trial) */
    const double* def_avg;                  /* [D] ap */
    const double* def_std;                  /* [D] sp != 0 */
    const int32_t* und_first;               /* [U1] the undefined keys of the first pass, in order (index within the problem) */
    const int32_t* und_rest;                /* [U2] those of every later pass */
    double* count;                          /* [N] in: the counts (0 for a key to be inserted); out: the final float counts */
    double* percent;                        /* [N] in: boc_percent (0 where it has no entry); out: the final percents, 0 on
                                               the keys that are not filtered */
    int64_t* rounded;                       /* [N] out: Python 2's int(round(count)); INT64_MIN where that is no int64 */
    int32_t* stop_reason;                   /* [P] out */
    int32_t* n_passes;                      /* [P] out: passes begun */
    int32_t* n_accepted;                    /* [P] out */
    int32_t* overflow;                      /* [P] out: FSQ_BACKGROUND_OVERFLOW_* bits */
    int32_t* accepted_key;                  /* [P, accepted_cap] out: the key accepted by each accepting pass */
    double* undefined_bp;                   /* [P, undefined_cap] out, or NULL: bp of each undefined key, pass after pass */
} FsqBackgroundArgs;

/* Bytes of workspace fsq_background_iterate needs; FSQ_EINVAL for sizes it refuses. */
int64_t fsq_background_workspace_bytes(int32_t n_problems, int64_t n_keys, int64_t n_defined, int64_t n_neighbours);

/* Runs every problem to its stop.  `args` is on the host.  Launches: two memsets, the neighbour table and the first z-scores
 * once, then per pass a head (one workgroup per problem), the trials (one lane per trial) and a tail (one workgroup per
 * problem); kernels of a finished problem return at once.  After every FSQ_BACKGROUND_BATCH_PASSES passes the done flags are copied to the host and
 * `stream` is synchronised.  ws: at least fsq_background_workspace_bytes(...), 8-byte aligned.
 * n_keys, n_defined < 2^31; n_neighbours < 2^31. */
int fsq_background_iterate(const FsqBackgroundArgs* args, void* ws, int64_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
