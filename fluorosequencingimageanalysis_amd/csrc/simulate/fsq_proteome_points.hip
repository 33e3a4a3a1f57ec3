// fsq_proteome_points.hip - the proteome Monte-Carlo over the points of a (p, b, u) grid in one launch each (C ABI of
// include/fsq_proteome_mc.h).
//
//   kpm_signals_points   one lane per (point, row) item, grid-strided: item i is row i % n_rows of point i / n_rows, so a
//                        wavefront mostly shares its point (its tables are broadcast loads, as the peptide's labels are) and
//                        writes a contiguous piece of d_key[point].  The per-sample body is pmc_sample of fsq_proteome_lane.h,
//                        the one kpm_signals runs: the point supplies u, the rows of its Edman table and its bleach table.  The
//                        point's two table indices come from device memory and are clamped into the tables that were passed.
//                        The bleach table is read from global memory (512 bytes a point, cached), not staged in LDS: a block's
//                        lanes may belong to two points or more.
//   kpm_tally_points     one lane per (point, row) item in the same order: key [point][row], protein [row], into table `point`
//                        of [n_points][slots] with the insert of fsq_pmc_insert.h.  A full table sets that point's flag, loses
//                        that row and the lane goes on to its next item.
// Every loop has a bound that does not depend on another lane, as in fsq_proteome_mc.hip; counts are integer atomic adds, so any
// schedule gives the same tables.
#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_proteome_mc.h"
#include "fsq_proteome_lane.h"
#include "fsq_pmc_insert.h"

namespace {

constexpr int PPT_BLOCK = 256;
constexpr int PPT_MAX_BLOCKS = 2048;            // one pass covers 524 288 items

__global__ void __launch_bounds__(PPT_BLOCK)
kpm_signals_points(const FsqProteomeParams prm, const FsqProteomePoint* __restrict__ g_points, const long long n_points,
                   const unsigned long long sample_stride, const int32_t* __restrict__ g_protein, const int32_t* __restrict__ g_n_head,
                   const long long* __restrict__ g_label_start, const uint32_t* __restrict__ g_labels,
                   const long long* __restrict__ g_edman_start, const double* __restrict__ g_edman, const int n_edman_tables,
                   const double* __restrict__ g_bleach, const int n_bleach_tables, const long long first_row, const long long n_rows,
                   unsigned long long* __restrict__ g_key, int32_t* __restrict__ g_row_protein, int32_t* __restrict__ g_n_draws)
{
    __shared__ unsigned long long s_E[FSQ_PMC_MAX_ACIDS], s_O[FSQ_PMC_MAX_ACIDS];
    __shared__ int s_base[FSQ_PMC_MAX_ACIDS];
    const int tid = threadIdx.x;
    if (tid < FSQ_PMC_MAX_ACIDS) {
        const bool on = tid < prm.n_acids;
        s_E[tid] = on ? prm.E[tid] : 0ull;
        s_O[tid] = on ? prm.O[tid] : 0ull;
        s_base[tid] = on ? prm.base[tid] : 0;
    }
    __syncthreads();

    const long long items = n_points * n_rows;
    for (long long i = (long long)blockIdx.x * PPT_BLOCK + tid; i < items; i += (long long)gridDim.x * PPT_BLOCK) {
        const long long k = i / n_rows, t = i - k * n_rows;
        const FsqProteomePoint pt = g_points[k];
        const int et = pt.edman_table < 0 ? 0 : pt.edman_table >= n_edman_tables ? n_edman_tables - 1 : pt.edman_table;
        const int bt = pt.bleach_table < 0 ? 0 : pt.bleach_table >= n_bleach_tables ? n_bleach_tables - 1 : pt.bleach_table;
        const long long g = first_row + t;
        const long long pep = g / prm.sample_size;
        const unsigned long long item = prm.first_sample + (unsigned long long)k * sample_stride + (unsigned long long)g;
        int L, H, n_draws;
        const uint32_t* __restrict__ lab = pmc_labels(g_label_start, g_labels, g_n_head, pep, L, H);
        const unsigned long long key = pmc_sample(item, prm.seed, pt.u, prm.max_d, lab, L, H,
                                                  g_edman_start + (long long)et * (prm.max_d + 2), g_edman,
                                                  g_bleach + (long long)bt * FSQ_PMC_MAX_EXPOSURES, s_E, s_O, s_base, n_draws);
        g_key[i] = key;
        if (g_row_protein && k == 0) g_row_protein[t] = g_protein[pep];
        if (g_n_draws) g_n_draws[i] = n_draws;
    }
}

__global__ void __launch_bounds__(PPT_BLOCK)
kpm_tally_points(const unsigned long long* __restrict__ g_key, const int32_t* __restrict__ g_row_protein, const long long n_points,
                 const long long n_rows, unsigned long long* __restrict__ g_signals, const long long signal_slots,
                 unsigned long long* __restrict__ g_pairs, long long* __restrict__ g_counts, const long long pair_slots,
                 int32_t* __restrict__ g_overflow)
{
    const long long items = n_points * n_rows;
    for (long long i = (long long)blockIdx.x * PPT_BLOCK + threadIdx.x; i < items; i += (long long)gridDim.x * PPT_BLOCK) {
        const long long k = i / n_rows, t = i - k * n_rows;
        const unsigned long long key = g_key[i];
        const int protein = g_row_protein[t];
        if (key == 0ull || protein < 0) continue;
        const int r = pmc_insert<false>(key, protein, 1ull, g_signals + k * signal_slots, signal_slots, g_pairs + k * pair_slots,
                                        g_counts + k * pair_slots, pair_slots);
        if (r == FSQ_PMC_NO_SIGNAL_SLOT) g_overflow[2 * k] = 1;
        else if (r == FSQ_PMC_NO_PAIR_SLOT) g_overflow[2 * k + 1] = 1;
    }
}

bool power_of_two(int64_t n, int64_t most) { return n >= 1 && n <= most && !(n & (n - 1)); }

unsigned blocks_for(int64_t n)
{
    const int64_t chunks = (n + PPT_BLOCK - 1) / PPT_BLOCK;
    return (unsigned)(chunks < PPT_MAX_BLOCKS ? chunks : PPT_MAX_BLOCKS);
}

}  // namespace

extern "C" int fsq_proteome_signals_points(const FsqProteomeParams* base, const FsqProteomePoint* d_points, int64_t n_points,
                                           int64_t sample_stride, const int32_t* d_protein, const int32_t* d_n_head,
                                           const int64_t* d_label_start, const uint32_t* d_labels, int64_t n_peptides,
                                           const int64_t* d_edman_start, const double* d_edman, int32_t n_edman_tables,
                                           const double* d_bleach, int32_t n_bleach_tables, int64_t first_row, int64_t n_rows,
                                           uint64_t* d_key, int32_t* d_row_protein, int32_t* d_n_draws, void* stream)
{
    const FsqProteomeParams* prm = base;
    if (!prm || n_peptides < 1 || prm->sample_size < 1 || first_row < 0 || n_rows < 0) return FSQ_EINVAL;
    if (n_points < 1 || n_points > FSQ_PMC_MAX_POINTS || sample_stride < 0 || n_edman_tables < 1 || n_bleach_tables < 1) return FSQ_EINVAL;
    if (prm->n_acids < 0 || prm->n_acids > FSQ_PMC_MAX_ACIDS || prm->max_d < 0 || prm->max_d > FSQ_PMC_MAX_HEAD) return FSQ_EINVAL;
    const __int128 total = (__int128)n_peptides * prm->sample_size;
    if ((__int128)first_row + n_rows > total) return FSQ_EINVAL;
    if ((__int128)prm->first_sample + (__int128)(n_points - 1) * sample_stride + total > ((__int128)1 << 64)) return FSQ_EINVAL;
    if (n_rows > INT64_MAX / n_points) return FSQ_EINVAL;
    int bits = 0;
    for (int a = 0; a < prm->n_acids; ++a) {
        if (prm->base[a] != bits || prm->O[a] != (prm->E[a] & (prm->E[a] << 1))) return FSQ_EINVAL;
        bits += __builtin_popcountll(prm->O[a]);
    }
    if (bits > 64) return FSQ_EINVAL;
    if (!d_points || !d_protein || !d_n_head || !d_label_start || !d_labels || !d_edman_start || !d_edman || !d_bleach) return FSQ_EINVAL;
    if (n_rows == 0) return FSQ_OK;
    if (!d_key) return FSQ_EINVAL;
    hipLaunchKernelGGL(kpm_signals_points, dim3(blocks_for(n_points * n_rows)), dim3(PPT_BLOCK), 0, (hipStream_t)stream, *prm, d_points,
                       (long long)n_points, (unsigned long long)sample_stride, d_protein, d_n_head, (const long long*)d_label_start,
                       d_labels, (const long long*)d_edman_start, d_edman, (int)n_edman_tables, d_bleach, (int)n_bleach_tables,
                       (long long)first_row, (long long)n_rows, (unsigned long long*)d_key, d_row_protein, d_n_draws);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_proteome_tally_points(const uint64_t* d_key, const int32_t* d_row_protein, int64_t n_points, int64_t n_rows,
                                         uint64_t* d_signals, int64_t signal_slots, uint64_t* d_pairs, int64_t* d_counts,
                                         int64_t pair_slots, int32_t* d_overflow, void* stream)
{
    if (n_rows < 0 || n_points < 1 || n_points > FSQ_PMC_MAX_POINTS) return FSQ_EINVAL;
    if (!power_of_two(signal_slots, FSQ_PMC_MAX_SIGNAL_SLOTS) || !power_of_two(pair_slots, FSQ_PMC_MAX_PAIR_SLOTS)) return FSQ_EINVAL;
    if (n_rows > INT64_MAX / n_points) return FSQ_EINVAL;
    if (!d_signals || !d_pairs || !d_counts || !d_overflow) return FSQ_EINVAL;
    if (n_rows == 0) return FSQ_OK;
    if (!d_key || !d_row_protein) return FSQ_EINVAL;
    hipLaunchKernelGGL(kpm_tally_points, dim3(blocks_for(n_points * n_rows)), dim3(PPT_BLOCK), 0, (hipStream_t)stream,
                       (const unsigned long long*)d_key, d_row_protein, (long long)n_points, (long long)n_rows,
                       (unsigned long long*)d_signals, (long long)signal_slots, (unsigned long long*)d_pairs, (long long*)d_counts,
                       (long long)pair_slots, d_overflow);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
