// fsq_peptide_lane.h - one lane's walk of one molecule through peptide_simulator.py's experimental_sequence (:251-277) and
// simulate_photometries (:333-353, 405-434): the body kps_simulate (fsq_peptide_sim.hip) and kss_simulate_points
// (fsq_signal_sweep.hip) share.  The chemistry parameters a sweep varies are a LaneChem value: uniform over a launch of
// the first kernel, a per-lane value in the second, where a wavefront may straddle parameter points.  Include after
// ../fsq_common.h, ../fsq_devmath.h, ../../../include/fsq_peptide_sim.h, ../libm/fsq_glibc_log.h and fsq_philox.h.
#pragma once

namespace {

// The draws of one (molecule, stream) pair in order: a block gives two, the second waits in w2, w3.
struct Draws {
    uint32_t k0, k1, mlo, mhi, stream, w2, w3;
    int j;
    __device__ __forceinline__ double next()
    {
        double r;
        if ((j & 1) == 0) {
            const Words w = philox4x32_10((uint32_t)(j >> 1), mlo, mhi, stream, k0, k1);
            w2 = w.w2; w3 = w.w3;
            r = uniform53(w.w0, w.w1);
        } else {
            r = uniform53(w2, w3);
        }
        ++j;
        return r;
    }
};

__device__ __forceinline__ Draws draws_of(unsigned long long seed, unsigned long long molecule, uint32_t stream)
{
    Draws d;
    d.k0 = (uint32_t)seed; d.k1 = (uint32_t)(seed >> 32);
    d.mlo = (uint32_t)molecule; d.mhi = (uint32_t)(molecule >> 32);
    d.stream = stream; d.w2 = d.w3 = 0u; d.j = 0;
    return d;
}

// LDS row strides for `frames` frames: doubles (odd) and bytes (a multiple of 4 with an odd number of banks)
__host__ __device__ __forceinline__ int dbl_stride(int frames) { return frames | 1; }
__host__ __device__ __forceinline__ int cnt_stride(int frames)
{
    int s = (frames + 3) / 4;
    return 4 * (s | 1);
}

// what a sweep varies: Edman efficiency, survival of an exposure, dud rate, surface loss before and after cycle sc
struct LaneChem {
    double p, per_cycle_b, u, s, s2;
};

// The chemistry (stream 0): dud and photobleach at cycle 0, then per cycle [Edman,] strip, photobleach.  put(c, live) gets
// the mask of live dyes after every cycle c in 0 .. C; with LOSS, my_lcyc / my_lcau get the loss cycle and cause of every
// labelled residue and *fail the cycles whose Edman drew and failed.  Returns the draws consumed.  `labels` may be the
// union of several letters' masks (fsq_peptide_labels.hip): the reference draws per labelled residue whatever its letter.
template <bool LOSS, class Put>
__device__ __forceinline__ int lane_chemistry_put(const LaneChem& ch, const unsigned long long seed, const unsigned long long molecule,
                                                  const unsigned long long labels, const int L, const int length, const int num_mocks,
                                                  const int C, const int sc, const Put put, uint8_t* const my_lcyc,
                                                  uint8_t* const my_lcau, unsigned long long* const fail)
{
    Draws d0 = draws_of(seed, molecule, 0u);
    unsigned long long live = labels;
    int nterm = 0;
    if (LOSS)
        for (int k = 0; k < L; ++k) { my_lcyc[k] = 0; my_lcau[k] = FSQ_PEPTIDE_CAUSE_NONE; }
    auto lose = [&](int b, int cycle, int cause) {
        if (LOSS) {
            const int k = __builtin_popcountll(labels & ((1ull << b) - 1ull));
            my_lcyc[k] = (uint8_t)cycle;
            my_lcau[k] = (uint8_t)cause;
        }
        live &= ~(1ull << b);
    };
    for (unsigned long long m = labels; m; m &= m - 1ull)                       // dud (:105-120)
        if (d0.next() < ch.u) lose(__builtin_ctzll(m), 0, FSQ_PEPTIDE_CAUSE_DUD);
    for (int c = 0; c <= C; ++c) {
        if (c > num_mocks && nterm < length) {                                  // Edman (:47-75)
            if (d0.next() < ch.p) {
                if ((live >> nterm) & 1ull) lose(nterm, c, FSQ_PEPTIDE_CAUSE_EDMAN);
                ++nterm;
            } else if (LOSS) {
                *fail |= 1ull << c;
            }
        }
        if (c > 0 && d0.next() < (c <= sc ? ch.s : ch.s2))                      // strip (:153-169)
            for (unsigned long long m = live; m; m &= m - 1ull) lose(__builtin_ctzll(m), c, FSQ_PEPTIDE_CAUSE_STRIP);
        for (unsigned long long m = live; m; m &= m - 1ull)                     // photobleach (:84-99)
            if (d0.next() > ch.per_cycle_b) lose(__builtin_ctzll(m), c, FSQ_PEPTIDE_CAUSE_DESTRUCTION);
        put(c, live);
    }
    return d0.j;
}

// one label letter: my_cnt[0 .. C] gets the count of every frame
template <bool LOSS>
__device__ __forceinline__ int lane_chemistry(const LaneChem& ch, const unsigned long long seed, const unsigned long long molecule,
                                              const unsigned long long labels, const int L, const int length, const int num_mocks,
                                              const int C, const int sc, uint8_t* const my_cnt, uint8_t* const my_lcyc,
                                              uint8_t* const my_lcau, unsigned long long* const fail)
{
    return lane_chemistry_put<LOSS>(ch, seed, molecule, labels, L, length, num_mocks, C, sc,
                                    [&](int c, unsigned long long live) { my_cnt[c] = (uint8_t)__builtin_popcountll(live); }, my_lcyc,
                                    my_lcau, fail);
}

// what the photometry of one colour channel needs beside its ddif row
struct LanePhot {
    double log_beta, beta_sigma, superdye_rate, superdye_factor;
};

// The photometry of the count row my_cnt[0 .. F): the superdye draws (stream s1) as a bit mask - the suffix sums of :350-352
// are then popcounts - and per frame with dyes one polar normal (stream s2), the mean summed left to right with glibc's
// log, glibc's exp.  my_dbl[0 .. F) gets the intensities, 0.0 where the count is 0; returns the category word; *n1 and
// *n2 get the draws consumed of the two streams.  The Gaussian cache starts empty.
__device__ __forceinline__ unsigned long long lane_photometry_streams(const LanePhot& ph, const unsigned long long seed,
                                                                      const uint32_t s1, const uint32_t s2, const double* const s_ddif,
                                                                      const unsigned long long molecule, const int F,
                                                                      const uint8_t* const my_cnt, double* const my_dbl, int* const n1,
                                                                      int* const n2)
{
    Draws d1 = draws_of(seed, molecule, s1), d2 = draws_of(seed, molecule, s2);
    const int c0 = my_cnt[0];
    unsigned super = 0u;                                                        // bit q: superdye draw q came out true
    for (int q = 0; q < c0; ++q)
        if (d1.next() < ph.superdye_rate) super |= 1u << q;
    const int total = __builtin_popcount(super);
    unsigned long long category = 0ull;
    bool has_gauss = false;
    double gauss = 0.0;
    int prev = c0;
    for (int f = 0; f < F; ++f) {
        const int c = my_cnt[f];
        double intensity = 0.0;
        if (c > 0) {
            double dyes = (double)c;
            if (ph.superdye_rate != 0.0) {
                // the draws of the drops before frame f are the first c0 - counts[f - 1]: what is left of `total`
                // is the suffix sum of :350-352
                const int before = f == 0 ? 0 : c0 - prev;
                const int inc = total - __builtin_popcount(super & ((1u << before) - 1u));
                dyes = dyes + (double)inc * ph.superdye_factor;
            }
            const double mean = (ph.log_beta + ln_log(dyes)) - s_ddif[c - 1];
            double z;
            if (has_gauss) {
                z = gauss;
                has_gauss = false;
            } else {                                                            // numpy's legacy_gauss
                int block = d2.j >> 1;
                z = polar_pair(&block, d2.mlo, d2.mhi, s2, d2.k0, d2.k1, &gauss);
                d2.j = 2 * block;
                has_gauss = true;
            }
            intensity = fsq_exp(mean + ph.beta_sigma * z);
            category |= 1ull << f;
        }
        prev = c;
        my_dbl[f] = intensity;
    }
    *n1 = d1.j; *n2 = d2.j;
    return category;
}

// one label letter: streams 1 and 2
__device__ __forceinline__ unsigned long long lane_photometry(const FsqPeptideSimParams& prm, const double* const s_ddif,
                                                              const unsigned long long molecule, const int F,
                                                              const uint8_t* const my_cnt, double* const my_dbl, int* const n1,
                                                              int* const n2)
{
    const LanePhot ph = {prm.log_beta, prm.beta_sigma, prm.superdye_rate, prm.superdye_factor};
    return lane_photometry_streams(ph, prm.seed, 1u, 2u, s_ddif, molecule, F, my_cnt, my_dbl, n1, n2);
}

inline bool is_finite(double x) { return x - x == 0.0; }

// the checks fsq_peptide_simulate makes before a launch: n molecules from prm->first_molecule on
inline bool params_ok(const FsqPeptideSimParams* p, int64_t n)
{
    if (!p || n < 0) return false;
    if (p->length < 1 || p->length > FSQ_PEPTIDE_MAX_LENGTH) return false;
    if (p->length < 64 && (p->label_mask >> p->length) != 0) return false;
    const int L = __builtin_popcountll(p->label_mask);
    if (L > FSQ_PEPTIDE_MAX_LABELLED) return false;
    if (p->num_mocks < 0 || p->num_edmans < 0 || p->num_mocks > FSQ_PEPTIDE_MAX_FRAMES || p->num_edmans > FSQ_PEPTIDE_MAX_FRAMES ||
        p->num_mocks + p->num_edmans + 1 > FSQ_PEPTIDE_MAX_FRAMES)
        return false;
    if (p->n_ddif < L || p->n_ddif > FSQ_PEPTIDE_MAX_LABELLED) return false;
    for (int i = 0; i < p->n_ddif; ++i)
        if (!is_finite(p->ddif[i])) return false;
    if (!(is_finite(p->p) && is_finite(p->per_cycle_b) && is_finite(p->u) && is_finite(p->s) && is_finite(p->s2) && is_finite(p->log_beta) &&
          is_finite(p->beta_sigma) && is_finite(p->superdye_factor)))
        return false;
    if (!(p->superdye_rate >= 0.0 && p->superdye_rate <= 1.0)) return false;
    if (p->first_molecule < 0 || n > INT64_MAX - p->first_molecule) return false;
    return true;
}

}  // namespace
