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
// The lane's two steps are in fsq_peptide_lane.h, which the parameter sweep (fsq_signal_sweep.hip) shares.
#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_peptide_sim.h"
#include "../libm/fsq_glibc_log.h"
#include "fsq_philox.h"
#include "fsq_peptide_lane.h"

namespace {

constexpr int WAVE = 64;
constexpr int MAX_BLOCKS = 16384;
constexpr int LOSS_STRIDE = 20;              // bytes of a lane's loss row in LDS: 5 banks, odd

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
    const LaneChem chem = {prm.p, prm.per_cycle_b, prm.u, prm.s, prm.s2};

    for (long long base = (long long)blockIdx.x * WAVE; base < n; base += (long long)gridDim.x * WAVE) {
        const int rows = (int)(n - base < WAVE ? n - base : WAVE);
        const bool active = lane < rows;
        const unsigned long long molecule = (unsigned long long)prm.first_molecule + (unsigned long long)(base + lane);
        int n_draws0 = 0;
        unsigned long long fail = 0ull;

        // ---- 1. chemistry --------------------------------------------------------------------------------------------
        if (active) {
            n_draws0 = lane_chemistry<true>(chem, prm.seed, molecule, labels, L, prm.length, prm.num_mocks, C, prm.sc, my_cnt, my_lcyc,
                                            my_lcau, &fail);
        }
        __syncthreads();
        for (int t = lane; t < rows * F; t += WAVE) g_counts[base * F + t] = s_cnt[(t / F) * CS + t % F];
        for (int t = lane; t < rows * L; t += WAVE) {
            g_loss_cycle[base * L + t] = s_lcyc[(t / L) * LOSS_STRIDE + t % L];
            g_loss_cause[base * L + t] = s_lcau[(t / L) * LOSS_STRIDE + t % L];
        }

        // ---- 2. photometry -------------------------------------------------------------------------------------------
        if (active) {
            int n_draws1, n_draws2;
            const unsigned long long category = lane_photometry(prm, s_ddif, molecule, F, my_cnt, my_dbl, &n_draws1, &n_draws2);
            g_category[base + lane] = category;
            g_edman_fail[base + lane] = fail;
            int32_t* const nd = g_n_draws + (base + lane) * 3;
            nd[0] = n_draws0; nd[1] = n_draws1; nd[2] = n_draws2;
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
