// fsq_proteome_mc.hip - the proteome-scale Monte-Carlo of MCsimlib.py (C ABI of include/fsq_proteome_mc.h).
//
//   kpm_signals   one lane per sample of the flattened [peptides][sample_size] space: random_signal (:863-1074) as a 64-bit key
//                 (the per-sample body is pmc_sample of fsq_proteome_lane.h, which fsq_proteome_points.hip shares).
//                 Pass 1 compares the dud draws with u and builds the survivor mask; pass 2 walks the survivors.  The Edman
//                 delay is a binary search in the host-built row of running _dp sums, the bleach a binary search in the
//                 host-built survival table: no exp, no pow, no per-lane arrays.  A peptide's labels are read straight from
//                 the CSR table: the lanes of a wavefront mostly share a peptide, so these are broadcast loads.
//   kpm_tally     one lane per (key, protein) row: table A key -> slot, table B (slot, protein) -> count (the insert of
//                 fsq_pmc_insert.h, which fsq_proteome_project.hip shares).
//   kpm_uniques   one lane per signal: the scan of find_uniques (:1436-1474) over its proteins in ascending index.
// Every loop has a bound that does not depend on another lane: labels <= 64, a table search <= 13 steps, a probe sequence <=
// the table's size, a scan = the signal's proteins.  A full table costs counts (and sets d_overflow), never a wait.
#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_proteome_mc.h"
#include "fsq_proteome_lane.h"
#include "fsq_pmc_insert.h"

namespace {

constexpr int PMC_BLOCK = 256;
constexpr int PMC_MAX_BLOCKS = 2048;            // one pass of kpm_signals / kpm_tally covers 524 288 rows

__global__ void __launch_bounds__(PMC_BLOCK)
kpm_signals(const FsqProteomeParams prm, const int32_t* __restrict__ g_protein, const int32_t* __restrict__ g_n_head,
            const long long* __restrict__ g_label_start, const uint32_t* __restrict__ g_labels,
            const long long* __restrict__ g_edman_start, const double* __restrict__ g_edman, const double* __restrict__ g_bleach,
            const long long first_row, const long long n_rows, unsigned long long* __restrict__ g_key,
            int32_t* __restrict__ g_row_protein, int32_t* __restrict__ g_n_draws)
{
    __shared__ unsigned long long s_E[FSQ_PMC_MAX_ACIDS], s_O[FSQ_PMC_MAX_ACIDS];
    __shared__ int s_base[FSQ_PMC_MAX_ACIDS];
    __shared__ double s_T[FSQ_PMC_MAX_EXPOSURES];
    const int tid = threadIdx.x;
    if (tid < FSQ_PMC_MAX_ACIDS) {
        const bool on = tid < prm.n_acids;
        s_E[tid] = on ? prm.E[tid] : 0ull;
        s_O[tid] = on ? prm.O[tid] : 0ull;
        s_base[tid] = on ? prm.base[tid] : 0;
    }
    if (tid < FSQ_PMC_MAX_EXPOSURES) s_T[tid] = g_bleach[tid];
    __syncthreads();

    for (long long t = (long long)blockIdx.x * PMC_BLOCK + tid; t < n_rows; t += (long long)gridDim.x * PMC_BLOCK) {
        const long long g = first_row + t;
        const long long pep = g / prm.sample_size;
        const unsigned long long item = prm.first_sample + (unsigned long long)g;
        int L, H, n_draws;
        const uint32_t* __restrict__ lab = pmc_labels(g_label_start, g_labels, g_n_head, pep, L, H);
        const unsigned long long key = pmc_sample(item, prm.seed, prm.u, prm.max_d, lab, L, H, g_edman_start, g_edman, s_T, s_E, s_O,
                                                  s_base, n_draws);
        g_key[t] = key;
        if (g_row_protein) g_row_protein[t] = g_protein[pep];
        if (g_n_draws) g_n_draws[t] = n_draws;
    }
}

__global__ void __launch_bounds__(PMC_BLOCK)
kpm_tally(const unsigned long long* __restrict__ g_key, const int32_t* __restrict__ g_row_protein, const long long n_rows,
          unsigned long long* __restrict__ g_signals, const long long signal_slots, unsigned long long* __restrict__ g_pairs,
          long long* __restrict__ g_counts, const long long pair_slots, int32_t* __restrict__ g_overflow)
{
    for (long long t = (long long)blockIdx.x * PMC_BLOCK + threadIdx.x; t < n_rows; t += (long long)gridDim.x * PMC_BLOCK) {
        const unsigned long long key = g_key[t];
        const int protein = g_row_protein[t];
        if (key == 0ull || protein < 0) continue;
        const int r = pmc_insert<false>(key, protein, 1ull, g_signals, signal_slots, g_pairs, g_counts, pair_slots);
        if (r == FSQ_PMC_NO_SIGNAL_SLOT) g_overflow[0] = 1;
        else if (r == FSQ_PMC_NO_PAIR_SLOT) g_overflow[1] = 1;
    }
}

__global__ void __launch_bounds__(PMC_BLOCK)
kpm_uniques(const int32_t* __restrict__ g_protein, const long long* __restrict__ g_count, const long long* __restrict__ g_segment,
            const long long n_signals, const FsqUniquesParams prm, int32_t* __restrict__ g_best_protein,
            long long* __restrict__ g_best_count, int32_t* __restrict__ g_second_protein, long long* __restrict__ g_second_count,
            int32_t* __restrict__ g_n_ties, long long* __restrict__ g_tertiary, uint8_t* __restrict__ g_passed)
{
    for (long long i = (long long)blockIdx.x * PMC_BLOCK + threadIdx.x; i < n_signals; i += (long long)gridDim.x * PMC_BLOCK) {
        const long long lo = g_segment[i], hi = g_segment[i + 1];
        int bp = -1, sp = -1;
        long long bc = 0, sc = 0;
        for (long long j = lo; j < hi; ++j) {                                       // (:1440-1444)
            const int p = g_protein[j];
            const long long c = g_count[j];
            if (c > bc) {
                if (prm.demote) { sp = bp; sc = bc; }
                bp = p; bc = c;
            } else if (c > sc) {
                sp = p; sc = c;
            }
        }
        int ties = 0;
        long long tertiary = 0;
        for (long long j = lo; j < hi; ++j) {                                       // (:1470-1474)
            const int p = g_protein[j];
            const long long c = g_count[j];
            if (prm.demote && p == bp) continue;
            if (c == sc && p != sp) ++ties;
            else if (c < sc) tertiary += c;
        }
        bool ratio_ok = true, max_ok;
        if (prm.ratio_mode == FSQ_PMC_RATIO_NONE) ratio_ok = sp < 0;
        else if (prm.ratio_mode == FSQ_PMC_RATIO_NUMBER) ratio_ok = sc == 0 || (double)bc / (double)sc >= prm.worst_ratio;
        if (prm.ratio_mode == FSQ_PMC_RATIO_ABSENT) max_ok = (double)sc <= prm.maximum_secondary;
        else max_ok = !prm.has_maximum_secondary || sp < 0 || (double)sc <= prm.maximum_secondary;
        g_best_protein[i] = bp; g_best_count[i] = bc;
        g_second_protein[i] = sp; g_second_count[i] = sc;
        g_n_ties[i] = ties; g_tertiary[i] = tertiary;
        g_passed[i] = ((double)bc >= prm.absolute_min && ratio_ok && max_ok) ? 1 : 0;
    }
}

bool power_of_two(int64_t n, int64_t most) { return n >= 1 && n <= most && !(n & (n - 1)); }

unsigned blocks_for(int64_t n)
{
    const int64_t chunks = (n + PMC_BLOCK - 1) / PMC_BLOCK;
    return (unsigned)(chunks < PMC_MAX_BLOCKS ? chunks : PMC_MAX_BLOCKS);
}

}  // namespace

extern "C" int fsq_proteome_signals(const FsqProteomeParams* prm, const int32_t* d_protein, const int32_t* d_n_head,
                                    const int64_t* d_label_start, const uint32_t* d_labels, int64_t n_peptides,
                                    const int64_t* d_edman_start, const double* d_edman, const double* d_bleach, int64_t first_row,
                                    int64_t n_rows, uint64_t* d_key, int32_t* d_row_protein, int32_t* d_n_draws, void* stream)
{
    if (!prm || n_peptides < 1 || prm->sample_size < 1 || first_row < 0 || n_rows < 0) return FSQ_EINVAL;
    if (prm->n_acids < 0 || prm->n_acids > FSQ_PMC_MAX_ACIDS || prm->max_d < 0 || prm->max_d > FSQ_PMC_MAX_HEAD) return FSQ_EINVAL;
    if (!(prm->u >= 0.0 && prm->u <= 1.0)) return FSQ_EINVAL;
    const __int128 total = (__int128)n_peptides * prm->sample_size;
    if ((__int128)first_row + n_rows > total) return FSQ_EINVAL;
    if ((__int128)prm->first_sample + total > ((__int128)1 << 64)) return FSQ_EINVAL;
    int bits = 0;
    for (int a = 0; a < prm->n_acids; ++a) {
        if (prm->base[a] != bits || prm->O[a] != (prm->E[a] & (prm->E[a] << 1))) return FSQ_EINVAL;
        bits += __builtin_popcountll(prm->O[a]);
    }
    if (bits > 64) return FSQ_EINVAL;
    if (!d_protein || !d_n_head || !d_label_start || !d_labels || !d_edman_start || !d_edman || !d_bleach) return FSQ_EINVAL;
    if (n_rows == 0) return FSQ_OK;
    if (!d_key) return FSQ_EINVAL;
    hipLaunchKernelGGL(kpm_signals, dim3(blocks_for(n_rows)), dim3(PMC_BLOCK), 0, (hipStream_t)stream, *prm, d_protein, d_n_head,
                       (const long long*)d_label_start, d_labels, (const long long*)d_edman_start, d_edman, d_bleach,
                       (long long)first_row, (long long)n_rows, (unsigned long long*)d_key, d_row_protein, d_n_draws);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_proteome_tally(const uint64_t* d_key, const int32_t* d_row_protein, int64_t n_rows, uint64_t* d_signals,
                                  int64_t signal_slots, uint64_t* d_pairs, int64_t* d_counts, int64_t pair_slots,
                                  int32_t* d_overflow, void* stream)
{
    if (n_rows < 0 || !power_of_two(signal_slots, FSQ_PMC_MAX_SIGNAL_SLOTS) || !power_of_two(pair_slots, FSQ_PMC_MAX_PAIR_SLOTS))
        return FSQ_EINVAL;
    if (!d_signals || !d_pairs || !d_counts || !d_overflow) return FSQ_EINVAL;
    if (n_rows == 0) return FSQ_OK;
    if (!d_key || !d_row_protein) return FSQ_EINVAL;
    hipLaunchKernelGGL(kpm_tally, dim3(blocks_for(n_rows)), dim3(PMC_BLOCK), 0, (hipStream_t)stream, (const unsigned long long*)d_key,
                       d_row_protein, (long long)n_rows, (unsigned long long*)d_signals, (long long)signal_slots,
                       (unsigned long long*)d_pairs, (long long*)d_counts, (long long)pair_slots, d_overflow);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_proteome_uniques(const int32_t* d_protein, const int64_t* d_count, const int64_t* d_segment, int64_t n_signals,
                                    const FsqUniquesParams* prm, int32_t* d_best_protein, int64_t* d_best_count,
                                    int32_t* d_second_protein, int64_t* d_second_count, int32_t* d_n_ties, int64_t* d_tertiary,
                                    uint8_t* d_passed, void* stream)
{
    if (!prm || n_signals < 0 || prm->ratio_mode < FSQ_PMC_RATIO_NONE || prm->ratio_mode > FSQ_PMC_RATIO_ABSENT) return FSQ_EINVAL;
    if (prm->worst_ratio != prm->worst_ratio || prm->absolute_min != prm->absolute_min ||
        prm->maximum_secondary != prm->maximum_secondary) return FSQ_EINVAL;
    if (n_signals == 0) return FSQ_OK;
    if (!d_protein || !d_count || !d_segment || !d_best_protein || !d_best_count || !d_second_protein || !d_second_count ||
        !d_n_ties || !d_tertiary || !d_passed) return FSQ_EINVAL;
    hipLaunchKernelGGL(kpm_uniques, dim3(blocks_for(n_signals)), dim3(PMC_BLOCK), 0, (hipStream_t)stream, d_protein,
                       (const long long*)d_count, (const long long*)d_segment, (long long)n_signals, *prm, d_best_protein,
                       (long long*)d_best_count, d_second_protein, (long long*)d_second_count, d_n_ties, (long long*)d_tertiary,
                       d_passed);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
