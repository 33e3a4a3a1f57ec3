// fsq_proteome_lane.h - one sample of the proteome Monte-Carlo (random_signal, MCsimlib.py :863-1074) as a 64-bit key: the
// per-sample body shared by kpm_signals (fsq_proteome_mc.hip: one chemistry for the launch) and kpm_signals_points
// (fsq_proteome_points.hip: one chemistry per point of a (p, b, u) grid).  What a point varies - the dud threshold u, the rows of
// its Edman table and its bleach table - are arguments; everything else is the sample's.  Both kernels therefore give the same
// key and the same number of draws for the same sample under the same parameters, by construction.
//
// Pass 1 compares the dud draws with u and builds the survivor mask; pass 2 walks the survivors.  The Edman delay is a binary
// search in the host-built row of running _dp sums, the bleach a binary search in the host-built survival table: no exp, no pow,
// no per-lane arrays.  Every loop is bounded: labels <= 64, a table search <= 13 steps.
#ifndef FSQ_PROTEOME_LANE_H
#define FSQ_PROTEOME_LANE_H
#include "../../../include/fsq_proteome_mc.h"
#include "fsq_philox.h"

// the draws of one item's stream 3, random access; the last block is kept
struct ItemDraws {
    uint32_t lo, hi, k0, k1;
    int block;
    Words w;
    __device__ __forceinline__ double get(const int j)
    {
        const int b = j >> 1;
        if (b != block) {
            w = philox4x32_10((uint32_t)b, lo, hi, (uint32_t)FSQ_PMC_STREAM, k0, k1);
            block = b;
        }
        return (j & 1) ? uniform53(w.w2, w.w3) : uniform53(w.w0, w.w1);
    }
};

// the first i < n with row[i] >= r, else n; n <= 4096
__device__ __forceinline__ int first_at_least(const double* __restrict__ row, int n, const double r)
{
    int lo = 0;
    for (int it = 0; it < 13 && n > 0; ++it) {
        const int half = n >> 1;
        if (row[lo + half] < r) { lo += half + 1; n -= half + 1; }
        else n = half;
    }
    return lo;
}

// the position of set bit number s (0-based) of m; m has more than s set bits
__device__ __forceinline__ int nth_set_bit(unsigned long long m, int s)
{
    int pos = 0;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
        const int c = __builtin_popcountll(m & ((1ull << w) - 1ull));
        if (s >= c) { s -= c; m >>= w; pos += w; }
    }
    return pos;
}

// The key of sample `item` under `seed` of the peptide whose L labels (H of them head labels) start at lab; n_draws receives the
// draws it consumed.  edman_start / edman are one Edman table (rows d = 1 .. max_d), T one bleach table of
// FSQ_PMC_MAX_EXPOSURES entries; s_E, s_O and s_base are the layout's per-acid words (FSQ_PMC_MAX_ACIDS each).
__device__ __forceinline__ unsigned long long
pmc_sample(const unsigned long long item, const unsigned long long seed, const double u, const int max_d,
           const uint32_t* __restrict__ lab, const int L, const int H, const long long* __restrict__ edman_start,
           const double* __restrict__ edman, const double* __restrict__ T, const unsigned long long* __restrict__ s_E,
           const unsigned long long* __restrict__ s_O, const int* __restrict__ s_base, int& n_draws)
{
    ItemDraws da = {(uint32_t)item, (uint32_t)(item >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), -1, {0, 0, 0, 0}};
    ItemDraws db = da;

    unsigned long long surv = 0ull;                                             // pass 1: duds (:910-933)
    for (int j = 0; j < L; ++j)
        if (da.get(j) > u) surv |= 1ull << ((lab[j] >> 24) & 63u);
    const int nsh = __builtin_popcountll(surv & (H >= 64 ? ~0ull : (1ull << H) - 1ull));

    unsigned long long key = 0ull;
    long long cum = 0;
    int prev = 0, rank = 0;
    for (int k = 0; k < H; ++k) {                                               // pass 2: surviving head labels by position
        if (!((surv >> k) & 1ull)) continue;
        const uint32_t w = lab[k];
        const int x0 = (int)(w & 0xffu), a = (int)((w >> 8) & 7u);
        const int d = x0 - prev;
        prev = x0;
        const double r = da.get(L + rank);                                      // Edman delay (:960-995)
        if (d >= 1 && d <= max_d) {
            const long long at = edman_start[d];
            long long n = edman_start[d + 1] - at;
            n = n < 0 ? 0 : n > FSQ_PMC_MAX_ROW ? FSQ_PMC_MAX_ROW : n;
            cum += first_at_least(edman + at, (int)n, r);
        }
        const long long gap = x0 + cum;
        const double r2 = db.get(L + nsh + rank);                               // bleach (:1007-1040)
        const unsigned long long Ea = s_E[a], Oa = s_O[a];
        const long long gm = gap - 1;
        const unsigned long long expo = gm >= 64 ? Ea : gm <= 0 ? 0ull : Ea & ((1ull << gm) - 1ull);
        const int s = first_at_least(T, FSQ_PMC_MAX_EXPOSURES, r2);
        long long x = gap;
        if (s < __builtin_popcountll(expo)) x = nth_set_bit(expo, s) + 1;
        if (x < 64 && ((Oa >> x) & 1ull)) key |= 1ull << (s_base[a] + __builtin_popcountll(Oa & ((1ull << x) - 1ull)));
        ++rank;
    }
    int trank = 0;
    for (int k = H; k < L; ++k) {                                               // surviving tail labels (:1044-1056)
        if (!((surv >> k) & 1ull)) continue;
        const int a = (int)((lab[k] >> 8) & 7u);
        const double r = db.get(L + 2 * nsh + trank);
        const unsigned long long Ea = s_E[a], Oa = s_O[a];
        const int s = first_at_least(T, FSQ_PMC_MAX_EXPOSURES, r);
        if (s < __builtin_popcountll(Ea)) {
            const int x = nth_set_bit(Ea, s) + 1;
            if (x < 64 && ((Oa >> x) & 1ull)) key |= 1ull << (s_base[a] + __builtin_popcountll(Oa & ((1ull << x) - 1ull)));
        }
        ++trank;
    }
    n_draws = L + 2 * nsh + trank;
    return key;
}

// the labels of peptide pep in the CSR table, the counts clamped to what a lane walks
__device__ __forceinline__ const uint32_t* pmc_labels(const long long* __restrict__ g_label_start, const uint32_t* __restrict__ g_labels,
                                                      const int32_t* __restrict__ g_n_head, const long long pep, int& L, int& H)
{
    const long long ls = g_label_start[pep];
    L = (int)(g_label_start[pep + 1] - ls);
    L = L < 0 ? 0 : L > FSQ_PMC_MAX_LABELS ? FSQ_PMC_MAX_LABELS : L;
    H = g_n_head[pep];
    H = H < 0 ? 0 : H > L ? L : H;
    return g_labels + ls;
}

#endif
