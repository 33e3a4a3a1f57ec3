// fsq_peptide_labels.hip - peptide Monte-Carlo simulation for several label letters, one colour channel each (C ABI of
// include/fsq_peptide_labels.h).
//
// kps_simulate (fsq_peptide_sim.hip) with a channel axis.  One lane walks one molecule; a block is one wavefront and takes 64
// consecutive molecules at a time:
//   1. chemistry (stream 0) on the union of the channels' masks - the reference draws per labelled residue whatever its
//      letter - with the count of every channel after every cycle, popcount(live & channel_mask[k]), to the lane's K count
//      rows in LDS and the loss cycle / cause of every labelled residue of the union to its loss rows;
//   2. per channel k, the photometry of its count row on its own two streams (1, 2 for k = 0, else 2 + 2k, 3 + 2k) into the
//      lane's one double row, which leaves as the intensities, is turned into logs in place and leaves again.
// The lane's steps are those of fsq_peptide_lane.h.  Tables are staged in LDS, row stride odd in banks, and leave as the
// 64 rows' contiguous span of a channel's [n][frames] block, consecutive lanes storing consecutive elements.
// LDS per block: 64 * (8 * dbl_stride(F) + K * cnt_stride(F) + 2 * loss_stride(L)) bytes, 59 392 at K = 4, F = 64, L = 60:
// below the 64 KiB a launch gets without an attribute.
#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_peptide_labels.h"
#include "../../../include/fsq_signal_sweep.h"
#include "../libm/fsq_glibc_log.h"
#include "fsq_philox.h"
#include "fsq_peptide_lane.h"

namespace {

constexpr int WAVE = 64;
constexpr int MAX_BLOCKS = 16384;
constexpr int MAX_K = FSQ_PEPTIDE_MAX_CHANNELS;
constexpr int DDIF_ROW = FSQ_PEPTIDE_MAX_LABELLED + 1;

// bytes of a lane's loss row in LDS for L labelled residues (up to 60): a multiple of 4 with an odd number of banks
__host__ __device__ __forceinline__ int loss_stride(int L) { return cnt_stride(L); }

size_t lds_bytes(int K, int frames, int L)
{
    return (size_t)WAVE * dbl_stride(frames) * 8 + (size_t)K * WAVE * cnt_stride(frames) + 2 * (size_t)WAVE * loss_stride(L);
}

__host__ __device__ __forceinline__ uint32_t superdye_stream(int k) { return k == 0 ? 1u : (uint32_t)(2 + 2 * k); }
__host__ __device__ __forceinline__ uint32_t normal_stream(int k) { return k == 0 ? 2u : (uint32_t)(3 + 2 * k); }

__global__ void __launch_bounds__(WAVE)
kpl_simulate(const FsqPeptideLabelsParams prm, const long long n, uint8_t* __restrict__ g_counts, uint8_t* __restrict__ g_loss_cycle,
             uint8_t* __restrict__ g_loss_cause, unsigned long long* __restrict__ g_edman_fail, double* __restrict__ g_intensity,
             double* __restrict__ g_log_intensity, unsigned long long* __restrict__ g_category, int32_t* __restrict__ g_n_draws)
{
    extern __shared__ double s_dbl[];
    __shared__ double s_ddif[MAX_K * DDIF_ROW];
    __shared__ LanePhot s_phot[MAX_K];
    const int lane = threadIdx.x;
    const int K = prm.n_channels;
    const int C = prm.num_mocks + prm.num_edmans, F = C + 1;
    unsigned long long mask[MAX_K], labels = 0ull;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k) {
        mask[k] = k < K ? prm.channel_mask[k] : 0ull;
        labels |= mask[k];
    }
    const int L = __builtin_popcountll(labels);
    const int DS = dbl_stride(F), CS = cnt_stride(F), LS = loss_stride(L);
    uint8_t* const s_cnt = (uint8_t*)(s_dbl + WAVE * DS);                       // [K][WAVE][CS]
    uint8_t* const s_lcyc = s_cnt + K * WAVE * CS;
    uint8_t* const s_lcau = s_lcyc + WAVE * LS;
    {
        const int k = lane / DDIF_ROW, i = lane % DDIF_ROW;                     // 64 lanes: 4 rows of 16
        s_ddif[lane] = k < K && i < prm.n_ddif[k] && i < FSQ_PEPTIDE_MAX_LABELLED ? prm.ddif[k][i] : 0.0;
        if (lane < MAX_K) {
            const bool on = lane < K;
            const LanePhot ph = {on ? prm.log_beta[lane] : 0.0, on ? prm.beta_sigma[lane] : 0.0, on ? prm.superdye_rate[lane] : 0.0,
                                 on ? prm.superdye_factor[lane] : 0.0};
            s_phot[lane] = ph;
        }
    }
    uint8_t* const my_cnt = s_cnt + lane * CS;                                  // channel k's row: + k * WAVE * CS
    uint8_t* const my_lcyc = s_lcyc + lane * LS;
    uint8_t* const my_lcau = s_lcau + lane * LS;
    double* const my_dbl = s_dbl + lane * DS;
    const LaneChem chem = {prm.p, prm.per_cycle_b, prm.u, prm.s, prm.s2};
    const int ND = 1 + 2 * K;
    __syncthreads();

    for (long long base = (long long)blockIdx.x * WAVE; base < n; base += (long long)gridDim.x * WAVE) {
        const int rows = (int)(n - base < WAVE ? n - base : WAVE);
        const bool active = lane < rows;
        const unsigned long long molecule = (unsigned long long)prm.first_molecule + (unsigned long long)(base + lane);

        // ---- 1. chemistry on the union --------------------------------------------------------------------------------
        if (active) {
            unsigned long long fail = 0ull;
            const int n_draws0 = lane_chemistry_put<true>(
                chem, prm.seed, molecule, labels, L, prm.length, prm.num_mocks, C, prm.sc,
                [&](int c, unsigned long long live) {
#pragma unroll
                    for (int k = 0; k < MAX_K; ++k)
                        if (k < K) my_cnt[k * WAVE * CS + c] = (uint8_t)__builtin_popcountll(live & mask[k]);
                },
                my_lcyc, my_lcau, &fail);
            g_edman_fail[base + lane] = fail;
            g_n_draws[(base + lane) * ND] = n_draws0;
        }
        __syncthreads();
        for (int k = 0; k < K; ++k) {
            uint8_t* const g = g_counts + ((long long)k * n + base) * F;
            const uint8_t* const s = s_cnt + k * WAVE * CS;
            for (int t = lane; t < rows * F; t += WAVE) g[t] = s[(t / F) * CS + t % F];
        }
        for (int t = lane; t < rows * L; t += WAVE) {
            g_loss_cycle[base * L + t] = s_lcyc[(t / L) * LS + t % L];
            g_loss_cause[base * L + t] = s_lcau[(t / L) * LS + t % L];
        }

        // ---- 2. photometry, channel by channel through the one double row ---------------------------------------------
        for (int k = 0; k < K; ++k) {
            double* const g_int = g_intensity + ((long long)k * n + base) * F;
            double* const g_log = g_log_intensity + ((long long)k * n + base) * F;
            if (active) {
                int n1, n2;
                const LanePhot ph = s_phot[k];
                const unsigned long long category = lane_photometry_streams(ph, prm.seed, superdye_stream(k), normal_stream(k),
                                                                            s_ddif + k * DDIF_ROW, molecule, F, my_cnt + k * WAVE * CS,
                                                                            my_dbl, &n1, &n2);
                g_category[(long long)k * n + base + lane] = category;
                int32_t* const nd = g_n_draws + (base + lane) * ND + 1 + 2 * k;
                nd[0] = n1; nd[1] = n2;
            }
            __syncthreads();
            for (int t = lane; t < rows * F; t += WAVE) g_int[t] = s_dbl[(t / F) * DS + t % F];
            __syncthreads();
            if (active)
                for (int f = 0; f < F; ++f) {
                    const double v = my_dbl[f];
                    my_dbl[f] = v > 0.0 ? ln_log(v) : FSQ_PEPTIDE_OFF_LOG;
                }
            __syncthreads();
            for (int t = lane; t < rows * F; t += WAVE) g_log[t] = s_dbl[(t / F) * DS + t % F];
            __syncthreads();
        }
    }
}

// ---- the sweep's batched form (fsq_peptide_simulate_labels_points of include/fsq_signal_sweep.h) ----
// kpl_simulate's lane over the flattened [points][molecules] space, as kss_simulate_points (fsq_signal_sweep.hip) is
// kps_simulate's: each lane with its own point's chemistry parameters, only counts, intensities and categories written.  No
// loss rows are staged: the dynamic LDS is 64 * (8 * dbl_stride(F) + K * cnt_stride(F)) bytes, 50 688 at K = 4, F = 64, and
// the channel values (s_ddif, s_phot) are 640 static bytes more.
constexpr size_t POINTS_STATIC_LDS = MAX_K * DDIF_ROW * 8 + MAX_K * 32;
constexpr size_t LAUNCH_LDS_LIMIT = 64 * 1024;

size_t points_lds_bytes(int K, int frames) { return (size_t)WAVE * dbl_stride(frames) * 8 + (size_t)K * WAVE * cnt_stride(frames); }

__global__ void __launch_bounds__(WAVE)
kpl_simulate_points(const FsqPeptideLabelsParams prm, const FsqSweepPoint* __restrict__ g_points, const long long n_per_point,
                    const long long molecule_stride, const long long first_row, const long long n, uint8_t* __restrict__ g_counts,
                    double* __restrict__ g_intensity, unsigned long long* __restrict__ g_category)
{
    extern __shared__ double s_dbl[];
    __shared__ double s_ddif[MAX_K * DDIF_ROW];
    __shared__ LanePhot s_phot[MAX_K];
    static_assert(sizeof(s_ddif) + sizeof(s_phot) == POINTS_STATIC_LDS, "POINTS_STATIC_LDS");
    const int lane = threadIdx.x;
    const int K = prm.n_channels;
    const int C = prm.num_mocks + prm.num_edmans, F = C + 1;
    unsigned long long mask[MAX_K], labels = 0ull;
#pragma unroll
    for (int k = 0; k < MAX_K; ++k) {
        mask[k] = k < K ? prm.channel_mask[k] : 0ull;
        labels |= mask[k];
    }
    const int L = __builtin_popcountll(labels);
    const int DS = dbl_stride(F), CS = cnt_stride(F);
    uint8_t* const s_cnt = (uint8_t*)(s_dbl + WAVE * DS);                       // [K][WAVE][CS]
    {
        const int k = lane / DDIF_ROW, i = lane % DDIF_ROW;                     // 64 lanes: 4 rows of 16
        s_ddif[lane] = k < K && i < prm.n_ddif[k] && i < FSQ_PEPTIDE_MAX_LABELLED ? prm.ddif[k][i] : 0.0;
        if (lane < MAX_K) {
            const bool on = lane < K;
            const LanePhot ph = {on ? prm.log_beta[lane] : 0.0, on ? prm.beta_sigma[lane] : 0.0, on ? prm.superdye_rate[lane] : 0.0,
                                 on ? prm.superdye_factor[lane] : 0.0};
            s_phot[lane] = ph;
        }
    }
    uint8_t* const my_cnt = s_cnt + lane * CS;                                  // channel k's row: + k * WAVE * CS
    double* const my_dbl = s_dbl + lane * DS;
    __syncthreads();

    for (long long base = (long long)blockIdx.x * WAVE; base < n; base += (long long)gridDim.x * WAVE) {
        const int rows = (int)(n - base < WAVE ? n - base : WAVE);
        const bool active = lane < rows;
        unsigned long long molecule = 0ull;
        if (active) {
            const long long g = first_row + base + lane;
            const long long pk = g / n_per_point;                                   // the row's point: a per-lane value
            const FsqSweepPoint pt = g_points[pk];
            const LaneChem chem = {pt.p, pt.per_cycle_b, pt.u, pt.s, pt.s2};
            molecule = (unsigned long long)prm.first_molecule + (unsigned long long)(pk * molecule_stride) +
                       (unsigned long long)(g - pk * n_per_point);
            lane_chemistry_put<false>(
                chem, prm.seed, molecule, labels, L, prm.length, prm.num_mocks, C, prm.sc,
                [&](int c, unsigned long long live) {
#pragma unroll
                    for (int k = 0; k < MAX_K; ++k)
                        if (k < K) my_cnt[k * WAVE * CS + c] = (uint8_t)__builtin_popcountll(live & mask[k]);
                },
                nullptr, nullptr, nullptr);
        }
        __syncthreads();
        for (int k = 0; k < K; ++k) {
            uint8_t* const g = g_counts + ((long long)k * n + base) * F;
            const uint8_t* const s = s_cnt + k * WAVE * CS;
            for (int t = lane; t < rows * F; t += WAVE) g[t] = s[(t / F) * CS + t % F];
        }
        for (int k = 0; k < K; ++k) {
            double* const g_int = g_intensity + ((long long)k * n + base) * F;
            if (active) {
                int n1, n2;
                const LanePhot ph = s_phot[k];
                g_category[(long long)k * n + base + lane] =
                    lane_photometry_streams(ph, prm.seed, superdye_stream(k), normal_stream(k), s_ddif + k * DDIF_ROW, molecule, F,
                                            my_cnt + k * WAVE * CS, my_dbl, &n1, &n2);
            }
            __syncthreads();
            for (int t = lane; t < rows * F; t += WAVE) g_int[t] = s_dbl[(t / F) * DS + t % F];
            __syncthreads();
        }
    }
}

// the checks fsq_peptide_simulate_labels makes before a launch
bool labels_params_ok(const FsqPeptideLabelsParams* p, int64_t n)
{
    if (!p || n < 0) return false;
    if (p->n_channels < 1 || p->n_channels > MAX_K) return false;
    if (p->length < 1 || p->length > FSQ_PEPTIDE_MAX_LENGTH) return false;
    if (p->num_mocks < 0 || p->num_edmans < 0 || p->num_mocks > FSQ_PEPTIDE_MAX_FRAMES || p->num_edmans > FSQ_PEPTIDE_MAX_FRAMES ||
        p->num_mocks + p->num_edmans + 1 > FSQ_PEPTIDE_MAX_FRAMES)
        return false;
    unsigned long long seen = 0ull;
    for (int k = 0; k < p->n_channels; ++k) {
        const unsigned long long m = p->channel_mask[k];
        if (p->length < 64 && (m >> p->length) != 0) return false;
        if (m & seen) return false;
        seen |= m;
        const int L = __builtin_popcountll(m);
        if (L > FSQ_PEPTIDE_MAX_LABELLED) return false;
        if (p->n_ddif[k] < L || p->n_ddif[k] > FSQ_PEPTIDE_MAX_LABELLED) return false;
        for (int i = 0; i < p->n_ddif[k]; ++i)
            if (!is_finite(p->ddif[k][i])) return false;
        if (!(is_finite(p->log_beta[k]) && is_finite(p->beta_sigma[k]) && is_finite(p->superdye_factor[k]))) return false;
        if (!(p->superdye_rate[k] >= 0.0 && p->superdye_rate[k] <= 1.0)) return false;
    }
    if (!(is_finite(p->p) && is_finite(p->per_cycle_b) && is_finite(p->u) && is_finite(p->s) && is_finite(p->s2))) return false;
    if (p->first_molecule < 0 || n > INT64_MAX - p->first_molecule) return false;
    return true;
}

}  // namespace

extern "C" int fsq_peptide_simulate_labels(const FsqPeptideLabelsParams* prm, int64_t n_molecules, uint8_t* d_counts,
                                           uint8_t* d_loss_cycle, uint8_t* d_loss_cause, uint64_t* d_edman_fail, double* d_intensity,
                                           double* d_log_intensity, uint64_t* d_category, int32_t* d_n_draws, void* stream)
{
    if (!labels_params_ok(prm, n_molecules)) return FSQ_EINVAL;
    if (n_molecules == 0) return FSQ_OK;
    const int K = prm->n_channels;
    unsigned long long labels = 0ull;
    for (int k = 0; k < K; ++k) labels |= prm->channel_mask[k];
    const int L = __builtin_popcountll(labels);
    if (!d_counts || !d_edman_fail || !d_intensity || !d_log_intensity || !d_category || !d_n_draws) return FSQ_EINVAL;
    if (L > 0 && (!d_loss_cycle || !d_loss_cause)) return FSQ_EINVAL;
    const int frames = prm->num_mocks + prm->num_edmans + 1;
    const int64_t chunks = (n_molecules + WAVE - 1) / WAVE;
    const int64_t blocks = chunks < MAX_BLOCKS ? chunks : MAX_BLOCKS;
    hipLaunchKernelGGL(kpl_simulate, dim3((unsigned)blocks), dim3(WAVE), lds_bytes(K, frames, L), (hipStream_t)stream, *prm,
                       (long long)n_molecules, d_counts, d_loss_cycle, d_loss_cause, (unsigned long long*)d_edman_fail, d_intensity,
                       d_log_intensity, (unsigned long long*)d_category, d_n_draws);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_peptide_simulate_labels_points(const FsqPeptideLabelsParams* base, const FsqSweepPoint* d_points, int64_t n_points,
                                                  int64_t n_per_point, int64_t molecule_stride, int64_t first_row, int64_t n_rows,
                                                  uint8_t* d_counts, double* d_intensity, uint64_t* d_category, void* stream)
{
    if (!labels_params_ok(base, 0)) return FSQ_EINVAL;
    if (n_points < 1 || n_per_point < 1 || molecule_stride < 0 || first_row < 0 || n_rows < 0) return FSQ_EINVAL;
    const __int128 total = (__int128)n_points * n_per_point;
    if ((__int128)first_row + n_rows > total) return FSQ_EINVAL;
    if ((__int128)base->first_molecule + (__int128)(n_points - 1) * molecule_stride + n_per_point - 1 > (__int128)INT64_MAX) return FSQ_EINVAL;
    if (!d_points) return FSQ_EINVAL;
    const int K = base->n_channels, frames = base->num_mocks + base->num_edmans + 1;
    const size_t lds = points_lds_bytes(K, frames);
    if (lds + POINTS_STATIC_LDS > LAUNCH_LDS_LIMIT) return FSQ_EINVAL;
    if ((__int128)n_rows * frames * K * 8 > (__int128)INT64_MAX) return FSQ_EINVAL;
    if (n_rows == 0) return FSQ_OK;
    if (!d_counts || !d_intensity || !d_category) return FSQ_EINVAL;
    const int64_t chunks = (n_rows + WAVE - 1) / WAVE;
    const int64_t blocks = chunks < MAX_BLOCKS ? chunks : MAX_BLOCKS;
    hipLaunchKernelGGL(kpl_simulate_points, dim3((unsigned)blocks), dim3(WAVE), lds, (hipStream_t)stream, *base, d_points,
                       (long long)n_per_point, (long long)molecule_stride, (long long)first_row, (long long)n_rows, d_counts,
                       d_intensity, (unsigned long long*)d_category);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
