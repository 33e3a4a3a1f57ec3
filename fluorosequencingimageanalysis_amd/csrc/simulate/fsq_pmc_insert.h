// fsq_pmc_insert.h - the claim-or-match insert into the two tables of the proteome tally (include/fsq_proteome_mc.h), shared by
// kpm_tally (fsq_proteome_mc.hip) and kpm_project (fsq_proteome_project.hip).
//
// Table A maps a key to its slot (0: free), table B maps (slot of A << 32 | protein) to a count (all ones: free).  A slot goes
// from free to one value once and never changes again, so one 64-bit compare-and-swap either claims it or tells whose it is,
// and a plain load that shows a value other than free is final.  Both probe loops are bounded by their table's size; no lane
// waits for another lane's store.
#ifndef FSQ_PMC_INSERT_H
#define FSQ_PMC_INSERT_H
#include "../../../include/fsq_proteome_mc.h"

#define FSQ_PMC_INSERTED 0
#define FSQ_PMC_NO_SIGNAL_SLOT 1
#define FSQ_PMC_NO_PAIR_SLOT 2

__device__ __forceinline__ unsigned long long pmc_hash(unsigned long long x)        // splitmix64's finaliser
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// The slot of `value` in a table of `slots` (a power of two) entries whose free entries hold `free`, claimed if it is new; -1
// if the table is full of other values.  PEEK: look with a plain load first and swap only where the slot looks free.
template <bool PEEK>
__device__ __forceinline__ long long pmc_claim(unsigned long long* __restrict__ table, const long long slots,
                                               const unsigned long long value, const unsigned long long free)
{
    const unsigned long long h = pmc_hash(value);
    for (long long i = 0; i < slots; ++i) {
        const long long at = (long long)((h + (unsigned long long)i) & (unsigned long long)(slots - 1));
        if (PEEK) {
            const unsigned long long seen = __hip_atomic_load(&table[at], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (seen == value) return at;
            if (seen != free) continue;
        }
        const unsigned long long was = atomicCAS(&table[at], free, value);
        if (was == free || was == value) return at;
    }
    return -1;
}

// Adds `weight` to the count of (key, protein): FSQ_PMC_INSERTED, or which table had no slot left (nothing is added then).
// key is not 0 and protein is not negative.
template <bool PEEK>
__device__ __forceinline__ int pmc_insert(const unsigned long long key, const int protein, const unsigned long long weight,
                                          unsigned long long* __restrict__ g_signals, const long long signal_slots,
                                          unsigned long long* __restrict__ g_pairs, long long* __restrict__ g_counts,
                                          const long long pair_slots)
{
    const long long slot = pmc_claim<PEEK>(g_signals, signal_slots, key, 0ull);
    if (slot < 0) return FSQ_PMC_NO_SIGNAL_SLOT;
    const unsigned long long pair = ((unsigned long long)slot << 32) | (unsigned long long)(uint32_t)protein;
    const long long at = pmc_claim<PEEK>(g_pairs, pair_slots, pair, (unsigned long long)FSQ_PMC_PAIR_EMPTY);
    if (at < 0) return FSQ_PMC_NO_PAIR_SLOT;
    atomicAdd((unsigned long long*)&g_counts[at], weight);
    return FSQ_PMC_INSERTED;
}

#endif
