// fsq_proteome_project.hip - SignalTrie.truncating_projection (:1697-1759) and merge's cycles= filter (:1694) of MCsimlib.py on
// counted (signal, protein) pairs, for many cycle counts in one launch (C ABI of include/fsq_proteome_mc.h).
//
//   kpm_project   one lane per (pair, mask) item, grid-strided.  Item t is pair t / n_masks under mask t % n_masks (pair-major:
//                 the lanes of a wavefront spread over the masks' tables, so at a short cycle count, where all pairs of a
//                 protein fold onto a handful of slots, a wavefront sends at most 64 / n_masks adds to one slot) or, with
//                 FSQ_PMC_MASK_MAJOR, pair t % n under mask t / n.  The projected key goes through the insert of
//                 fsq_pmc_insert.h into table mask of [n_masks][slots], with a plain load before each compare-and-swap: most
//                 items find their slot already claimed.  The count is one 64-bit integer atomic add of the pair's weight.
// Every schedule of integer adds gives the same tables, so neither order nor the plain load shows in a result.  A full table sets
// that mask's flag and the lane goes on to its next item.
#include "../fsq_common.h"
#include "../../../include/fsq_proteome_mc.h"
#include "fsq_pmc_insert.h"

namespace {

constexpr int PPJ_BLOCK = 256;
constexpr int PPJ_MAX_BLOCKS = 2048;            // one pass covers 524 288 items

__global__ void __launch_bounds__(PPJ_BLOCK)
kpm_project(const unsigned long long* __restrict__ g_key, const int32_t* __restrict__ g_protein, const long long* __restrict__ g_count,
            const long long n, const unsigned long long* __restrict__ g_mask, const long long n_masks, const int within,
            const int mask_major, unsigned long long* __restrict__ g_signals, const long long signal_slots,
            unsigned long long* __restrict__ g_pairs, long long* __restrict__ g_counts, const long long pair_slots,
            int32_t* __restrict__ g_overflow)
{
    const long long items = n * n_masks;
    for (long long t = (long long)blockIdx.x * PPJ_BLOCK + threadIdx.x; t < items; t += (long long)gridDim.x * PPJ_BLOCK) {
        const long long i = mask_major ? t % n : t / n_masks;
        const long long m = mask_major ? t / n : t % n_masks;
        const unsigned long long key = g_key[i], mask = g_mask[m];
        const int protein = g_protein[i];
        const unsigned long long weight = g_count ? (unsigned long long)g_count[i] : 1ull;
        const unsigned long long projected = within ? ((key & ~mask) ? 0ull : key) : (key & mask);
        if (projected == 0ull || protein < 0 || weight == 0ull) continue;
        const int r = pmc_insert<true>(projected, protein, weight, g_signals + m * signal_slots, signal_slots,
                                       g_pairs + m * pair_slots, g_counts + m * pair_slots, pair_slots);
        if (r == FSQ_PMC_NO_SIGNAL_SLOT) g_overflow[2 * m] = 1;
        else if (r == FSQ_PMC_NO_PAIR_SLOT) g_overflow[2 * m + 1] = 1;
    }
}

bool power_of_two(int64_t n, int64_t most) { return n >= 1 && n <= most && !(n & (n - 1)); }

}  // namespace

extern "C" int fsq_proteome_project(const uint64_t* d_key, const int32_t* d_protein, const int64_t* d_count, int64_t n,
                                    const uint64_t* d_mask, int64_t n_masks, int32_t mode, uint64_t* d_signals, int64_t signal_slots,
                                    uint64_t* d_pairs, int64_t* d_counts, int64_t pair_slots, int32_t* d_overflow, void* stream)
{
    const int32_t what = mode & ~FSQ_PMC_MASK_MAJOR;
    if (n < 0 || n_masks < 1 || n_masks > FSQ_PMC_MAX_MASKS || (what != FSQ_PMC_PROJECT && what != FSQ_PMC_WITHIN)) return FSQ_EINVAL;
    if (!power_of_two(signal_slots, FSQ_PMC_MAX_SIGNAL_SLOTS) || !power_of_two(pair_slots, FSQ_PMC_MAX_PAIR_SLOTS)) return FSQ_EINVAL;
    if (n > INT64_MAX / n_masks) return FSQ_EINVAL;
    if (!d_mask || !d_signals || !d_pairs || !d_counts || !d_overflow) return FSQ_EINVAL;
    if (n == 0) return FSQ_OK;
    if (!d_key || !d_protein) return FSQ_EINVAL;
    const int64_t chunks = (n * n_masks + PPJ_BLOCK - 1) / PPJ_BLOCK;
    hipLaunchKernelGGL(kpm_project, dim3((unsigned)(chunks < PPJ_MAX_BLOCKS ? chunks : PPJ_MAX_BLOCKS)), dim3(PPJ_BLOCK), 0,
                       (hipStream_t)stream, (const unsigned long long*)d_key, d_protein, (const long long*)d_count, (long long)n,
                       (const unsigned long long*)d_mask, (long long)n_masks, what == FSQ_PMC_WITHIN ? 1 : 0,
                       (mode & FSQ_PMC_MASK_MAJOR) ? 1 : 0, (unsigned long long*)d_signals, (long long)signal_slots,
                       (unsigned long long*)d_pairs, (long long*)d_counts, (long long)pair_slots, d_overflow);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
