// fsq_peptide_sim.hip - peptide Monte-Carlo simulation (C ABI of include/fsq_peptide_sim.h).
//
// One lane walks one molecule through peptide_simulator.py's experimental_sequence (:251-277): its state is a uint64 mask
// of live dyes, the index of the N-terminal residue and the draw counters, all in registers.  The draws are Philox4x32-10
// blocks keyed by (seed, molecule, stream), so a lane needs nothing from its neighbours and a chunked run repeats a whole
// one.  A block is one wavefront and takes 64 consecutive molecules at a time:
//   1. chemistry (stream 0): dud and photobleach at cycle 0, then per cycle [Edman,] strip, photobleach.  The count of every
//      frame and the loss cycle / cause of every labelled residue go to the lane's row in LDS.
//   2. photometry: the superdye draws (stream 1) as a bit mask - the suffix sums of :350-352 are then popcounts - and per
//      frame with dyes one polar normal (stream 2), the mean summed left to right with glibc's log, glibc's exp.
// The tables a lane fills row by row ([n][frames] counts, intensities, log intensities, [n][labelled] losses) are staged in
// LDS, row stride odd in banks, and leave as the 64 rows' contiguous span of global memory, consecutive lanes storing
// consecutive elements.  The per-molecule words (category, Edman failures, draw counts) are stored by their lane.
#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_peptide_sim.h"
#include "../libm/fsq_glibc_log.h"
#include "fsq_philox.h"

namespace {

constexpr int WAVE = 64;
constexpr int MAX_BLOCKS = 16384;
constexpr int LOSS_STRIDE = 20;              // bytes of a lane's loss row in LDS: 5 banks, odd

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
size_t lds_bytes(int frames)
{
    return (size_t)WAVE * dbl_stride(frames) * 8 + (size_t)WAVE * cnt_stride(frames) + 2 * (size_t)WAVE * LOSS_STRIDE;
}

__global__ void __launch_bounds__(WAVE)
kps_simulate(const FsqPeptideSimParams prm, const long long n, uint8_t* __restrict__ g_counts, uint8_t* __restrict__ g_loss_cycle,
             uint8_t* __restrict__ g_loss_cause, unsigned long long* __restrict__ g_edman_fail, double* __restrict__ g_intensity,
             double* __restrict__ g_log_intensity, unsigned long long* __restrict__ g_category, int32_t* __restrict__ g_n_draws)
{
    extern __shared__ double s_dbl[];
    __shared__ double s_ddif[FSQ_PEPTIDE_MAX_LABELLED + 1];
    const int lane = threadIdx.x;
    const int C = prm.num_mocks + prm.num_edmans, F = C + 1;
    const int L = __builtin_popcountll(prm.label_mask);
    const int DS = dbl_stride(F), CS = cnt_stride(F);
    uint8_t* const s_cnt = (uint8_t*)(s_dbl + WAVE * DS);
    uint8_t* const s_lcyc = s_cnt + WAVE * CS;
    uint8_t* const s_lcau = s_lcyc + WAVE * LOSS_STRIDE;
    if (lane <= FSQ_PEPTIDE_MAX_LABELLED) s_ddif[lane] = lane < prm.n_ddif && lane < FSQ_PEPTIDE_MAX_LABELLED ? prm.ddif[lane] : 0.0;
    uint8_t* const my_cnt = s_cnt + lane * CS;
    uint8_t* const my_lcyc = s_lcyc + lane * LOSS_STRIDE;
    uint8_t* const my_lcau = s_lcau + lane * LOSS_STRIDE;
    double* const my_dbl = s_dbl + lane * DS;
    const unsigned long long labels = prm.label_mask;

    for (long long base = (long long)blockIdx.x * WAVE; base < n; base += (long long)gridDim.x * WAVE) {
        const int rows = (int)(n - base < WAVE ? n - base : WAVE);
        const bool active = lane < rows;
        const unsigned long long molecule = (unsigned long long)prm.first_molecule + (unsigned long long)(base + lane);
        int n_draws0 = 0;
        unsigned long long fail = 0ull;

        // ---- 1. chemistry --------------------------------------------------------------------------------------------
        if (active) {
            Draws d0 = draws_of(prm.seed, molecule, 0u);
            unsigned long long live = labels;
            int nterm = 0;
            for (int k = 0; k < L; ++k) { my_lcyc[k] = 0; my_lcau[k] = FSQ_PEPTIDE_CAUSE_NONE; }
            auto lose = [&](int b, int cycle, int cause) {
                const int k = __builtin_popcountll(labels & ((1ull << b) - 1ull));
                my_lcyc[k] = (uint8_t)cycle;
                my_lcau[k] = (uint8_t)cause;
                live &= ~(1ull << b);
            };
            for (unsigned long long m = labels; m; m &= m - 1ull)                       // dud (:105-120)
                if (d0.next() < prm.u) lose(__builtin_ctzll(m), 0, FSQ_PEPTIDE_CAUSE_DUD);
            for (int c = 0; c <= C; ++c) {
                if (c > prm.num_mocks && nterm < prm.length) {                          // Edman (:47-75)
                    if (d0.next() < prm.p) {
                        if ((live >> nterm) & 1ull) lose(nterm, c, FSQ_PEPTIDE_CAUSE_EDMAN);
                        ++nterm;
                    } else {
                        fail |= 1ull << c;
                    }
                }
                if (c > 0 && d0.next() < (c <= prm.sc ? prm.s : prm.s2))                // strip (:153-169)
                    for (unsigned long long m = live; m; m &= m - 1ull) lose(__builtin_ctzll(m), c, FSQ_PEPTIDE_CAUSE_STRIP);
                for (unsigned long long m = live; m; m &= m - 1ull)                     // photobleach (:84-99)
                    if (d0.next() > prm.per_cycle_b) lose(__builtin_ctzll(m), c, FSQ_PEPTIDE_CAUSE_DESTRUCTION);
                my_cnt[c] = (uint8_t)__builtin_popcountll(live);
            }
            n_draws0 = d0.j;
        }
        __syncthreads();
        for (int t = lane; t < rows * F; t += WAVE) g_counts[base * F + t] = s_cnt[(t / F) * CS + t % F];
        for (int t = lane; t < rows * L; t += WAVE) {
            g_loss_cycle[base * L + t] = s_lcyc[(t / L) * LOSS_STRIDE + t % L];
            g_loss_cause[base * L + t] = s_lcau[(t / L) * LOSS_STRIDE + t % L];
        }

        // ---- 2. photometry -------------------------------------------------------------------------------------------
        if (active) {
            Draws d1 = draws_of(prm.seed, molecule, 1u), d2 = draws_of(prm.seed, molecule, 2u);
            const int c0 = my_cnt[0];
            unsigned super = 0u;                                                        // bit q: superdye draw q came out true
            for (int q = 0; q < c0; ++q)
                if (d1.next() < prm.superdye_rate) super |= 1u << q;
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
                    if (prm.superdye_rate != 0.0) {
                        // the draws of the drops before frame f are the first c0 - counts[f - 1]: what is left of `total`
                        // is the suffix sum of :350-352
                        const int before = f == 0 ? 0 : c0 - prev;
                        const int inc = total - __builtin_popcount(super & ((1u << before) - 1u));
                        dyes = dyes + (double)inc * prm.superdye_factor;
                    }
                    const double mean = (prm.log_beta + ln_log(dyes)) - s_ddif[c - 1];
                    double z;
                    if (has_gauss) {
                        z = gauss;
                        has_gauss = false;
                    } else {                                                            // numpy's legacy_gauss
                        int block = d2.j >> 1;
                        z = polar_pair(&block, d2.mlo, d2.mhi, 2u, d2.k0, d2.k1, &gauss);
                        d2.j = 2 * block;
                        has_gauss = true;
                    }
                    intensity = fsq_exp(mean + prm.beta_sigma * z);
                    category |= 1ull << f;
                }
                prev = c;
                my_dbl[f] = intensity;
            }
            g_category[base + lane] = category;
            g_edman_fail[base + lane] = fail;
            int32_t* const nd = g_n_draws + (base + lane) * 3;
            nd[0] = n_draws0; nd[1] = d1.j; nd[2] = d2.j;
        }
        __syncthreads();
        for (int t = lane; t < rows * F; t += WAVE) g_intensity[base * F + t] = s_dbl[(t / F) * DS + t % F];
        __syncthreads();
        if (active)
            for (int f = 0; f < F; ++f) {
                const double v = my_dbl[f];
                my_dbl[f] = v > 0.0 ? ln_log(v) : FSQ_PEPTIDE_OFF_LOG;
            }
        __syncthreads();
        for (int t = lane; t < rows * F; t += WAVE) g_log_intensity[base * F + t] = s_dbl[(t / F) * DS + t % F];
        __syncthreads();
    }
}

__global__ void kps_philox_words(const uint32_t* __restrict__ counters, const uint32_t* __restrict__ keys, long long n,
                                 uint32_t* __restrict__ out)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const Words w = philox4x32_10(counters[4 * i], counters[4 * i + 1], counters[4 * i + 2], counters[4 * i + 3], keys[2 * i],
                                      keys[2 * i + 1]);
        out[4 * i] = w.w0; out[4 * i + 1] = w.w1; out[4 * i + 2] = w.w2; out[4 * i + 3] = w.w3;
    }
}

bool is_finite(double x) { return x - x == 0.0; }

bool params_ok(const FsqPeptideSimParams* p, int64_t n)
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

extern "C" int fsq_peptide_simulate(const FsqPeptideSimParams* prm, int64_t n_molecules, uint8_t* d_counts, uint8_t* d_loss_cycle,
                                    uint8_t* d_loss_cause, uint64_t* d_edman_fail, double* d_intensity, double* d_log_intensity,
                                    uint64_t* d_category, int32_t* d_n_draws, void* stream)
{
    if (!params_ok(prm, n_molecules)) return FSQ_EINVAL;
    if (n_molecules == 0) return FSQ_OK;
    const int L = __builtin_popcountll(prm->label_mask);
    if (!d_counts || !d_edman_fail || !d_intensity || !d_log_intensity || !d_category || !d_n_draws) return FSQ_EINVAL;
    if (L > 0 && (!d_loss_cycle || !d_loss_cause)) return FSQ_EINVAL;
    const int frames = prm->num_mocks + prm->num_edmans + 1;
    const int64_t chunks = (n_molecules + WAVE - 1) / WAVE;
    const int64_t blocks = chunks < MAX_BLOCKS ? chunks : MAX_BLOCKS;
    hipLaunchKernelGGL(kps_simulate, dim3((unsigned)blocks), dim3(WAVE), lds_bytes(frames), (hipStream_t)stream, *prm,
                       (long long)n_molecules, d_counts, d_loss_cycle, d_loss_cause, (unsigned long long*)d_edman_fail, d_intensity,
                       d_log_intensity, (unsigned long long*)d_category, d_n_draws);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_philox_words(const uint32_t* d_counters, const uint32_t* d_keys, int64_t n, uint32_t* d_out, void* stream)
{
    if (n < 0) return FSQ_EINVAL;
    if (n == 0) return FSQ_OK;
    if (!d_counters || !d_keys || !d_out) return FSQ_EINVAL;
    const int64_t blocks = (n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096;
    hipLaunchKernelGGL(kps_philox_words, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_counters, d_keys, (long long)n,
                       d_out);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
