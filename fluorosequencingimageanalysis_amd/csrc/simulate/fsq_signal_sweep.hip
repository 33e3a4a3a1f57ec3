// fsq_signal_sweep.hip - simulation parameter sweeps scored against observed signals (C ABI of include/fsq_signal_sweep.h).
//
//   kss_simulate_points  the lane of kps_simulate (fsq_peptide_lane.h) over the flattened [points][molecules] space: a block is
//                        one wavefront and takes 64 consecutive rows, each lane with its own point's chemistry parameters.
//                        Only counts, intensities and categories are written, staged in LDS as in fsq_peptide_sim.hip.
//   kss_tally            one lane per row: the row's 64-bit signal key, added to a per-block LDS table (one sub-table for
//                        each of the first TALLY_POINTS points of the block), which is then flushed to the points' global
//                        open-addressing tables with one atomic add per distinct (point, key) of the block.
//   kss_tally_joint      kss_tally for molecules of K colour channels, rows [K][n_rows][frames]: only the row-to-key step
//                        differs (joint_row_key, the joint key of include/fsq_signal_sweep.h); the tables are the same.
//   kss_lookup           one lane per (wanted key, point): the dense count matrix.
//   kss_scores           one lane per point: signal_correlation (jupyter_development.py:279-578), sums left to right.
// Every probe loop has a fixed bound and no lane reads what another lane stores without an atomic: a full or wrong table costs
// a count (and sets d_overflow), never a wait.
#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_signal_sweep.h"
#include "../libm/fsq_glibc_log.h"
#include "../libm/fsq_glibc_pow.h"
#include "fsq_philox.h"
#include "fsq_peptide_lane.h"
#include "fsq_score_term.h"

namespace {

constexpr int WAVE = 64;
constexpr int MAX_BLOCKS = 16384;

size_t points_lds_bytes(int frames) { return (size_t)WAVE * dbl_stride(frames) * 8 + (size_t)WAVE * cnt_stride(frames); }

__global__ void __launch_bounds__(WAVE)
kss_simulate_points(const FsqPeptideSimParams prm, const FsqSweepPoint* __restrict__ g_points, const long long n_per_point,
                    const long long molecule_stride, const long long first_row, const long long n, uint8_t* __restrict__ g_counts,
                    double* __restrict__ g_intensity, unsigned long long* __restrict__ g_category)
{
    extern __shared__ double s_dbl[];
    __shared__ double s_ddif[FSQ_PEPTIDE_MAX_LABELLED + 1];
    const int lane = threadIdx.x;
    const int C = prm.num_mocks + prm.num_edmans, F = C + 1;
    const int L = __builtin_popcountll(prm.label_mask);
    const int DS = dbl_stride(F), CS = cnt_stride(F);
    uint8_t* const s_cnt = (uint8_t*)(s_dbl + WAVE * DS);
    if (lane <= FSQ_PEPTIDE_MAX_LABELLED) s_ddif[lane] = lane < prm.n_ddif && lane < FSQ_PEPTIDE_MAX_LABELLED ? prm.ddif[lane] : 0.0;
    uint8_t* const my_cnt = s_cnt + lane * CS;
    double* const my_dbl = s_dbl + lane * DS;
    __syncthreads();

    for (long long base = (long long)blockIdx.x * WAVE; base < n; base += (long long)gridDim.x * WAVE) {
        const int rows = (int)(n - base < WAVE ? n - base : WAVE);
        if (lane < rows) {
            const long long g = first_row + base + lane;
            const long long k = g / n_per_point;                                    // the row's point: a per-lane value
            const FsqSweepPoint pt = g_points[k];
            const LaneChem chem = {pt.p, pt.per_cycle_b, pt.u, pt.s, pt.s2};
            const unsigned long long molecule = (unsigned long long)prm.first_molecule + (unsigned long long)(k * molecule_stride) +
                                                (unsigned long long)(g - k * n_per_point);
            lane_chemistry<false>(chem, prm.seed, molecule, prm.label_mask, L, prm.length, prm.num_mocks, C, prm.sc, my_cnt, nullptr,
                                  nullptr, nullptr);
            int n1, n2;
            g_category[base + lane] = lane_photometry(prm, s_ddif, molecule, F, my_cnt, my_dbl, &n1, &n2);
        }
        __syncthreads();
        for (int t = lane; t < rows * F; t += WAVE) {
            g_counts[base * F + t] = s_cnt[(t / F) * CS + t % F];
            g_intensity[base * F + t] = s_dbl[(t / F) * DS + t % F];
        }
        __syncthreads();
    }
}

// ---- the tally ----

constexpr int TALLY_BLOCK = 256;
constexpr int TALLY_POINTS = 4;                 // points of a block that get an LDS sub-table (rows arrive in point order)
constexpr int TALLY_SUB = 128;                  // slots of a sub-table
constexpr int TALLY_LDS_SLOTS = TALLY_POINTS * TALLY_SUB;
constexpr int TALLY_LDS_PROBES = 16;            // then the row goes to the global table itself
constexpr int ROW_SIGNAL = 0, ROW_NONE = 1, ROW_UNKEYED = 2;

__device__ __forceinline__ unsigned long long key_hash(unsigned long long x)        // splitmix64's finaliser
{
    x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27; x *= 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

// (decrements, last == 0, first) of a count row as the key of include/fsq_signal_sweep.h
__device__ __forceinline__ int row_key(const uint8_t* __restrict__ row, const int frames, unsigned long long* key)
{
    int prev = row[0], drops = 0;
    unsigned long long k = (unsigned long long)(prev & 15);
    bool up = false, unkeyed = prev > 15;
    for (int f = 1; f < frames; ++f) {
        const int c = row[f];
        if (c > prev) up = true;
        for (int j = c; j < prev; ++j) {
            if (drops < FSQ_SIGNAL_MAX_DROPS) k |= (unsigned long long)f << (4 + 6 * drops);
            ++drops;
        }
        prev = c;
    }
    *key = k;
    return up ? ROW_NONE : (unkeyed || drops > FSQ_SIGNAL_MAX_DROPS) ? ROW_UNKEYED : ROW_SIGNAL;
}

// n more of `key` in point's table: at most `slots` probes, one compare-and-swap each
__device__ __forceinline__ void table_add(unsigned long long* __restrict__ g_keys, long long* __restrict__ g_counts,
                                          int32_t* __restrict__ g_overflow, const int point, const int slots,
                                          const unsigned long long key, const long long n)
{
    const long long base = (long long)point * slots;
    const unsigned h = (unsigned)key_hash(key);
    for (int i = 0; i < slots; ++i) {
        const long long at = base + (long long)((h + (unsigned)i) & (unsigned)(slots - 1));
        const unsigned long long was = atomicCAS(&g_keys[at], (unsigned long long)FSQ_SIGNAL_EMPTY, key);
        if (was == FSQ_SIGNAL_EMPTY || was == key) {
            atomicAdd((unsigned long long*)&g_counts[at], (unsigned long long)n);
            return;
        }
    }
    g_overflow[point] = 1;
}

// The joint key of include/fsq_signal_sweep.h of a molecule's K count rows, channel k's at row0 + k * channel_stride: the
// frames once, the channels inside, a field per lost dye.  K = 1: row_key's key and answer.
__device__ __forceinline__ int joint_row_key(const uint8_t* __restrict__ row0, const long long channel_stride, const int K,
                                             const int frames, unsigned long long* key)
{
    const int B = FSQ_SIGNAL_JOINT_DROP_BITS(K), D = FSQ_SIGNAL_JOINT_MAX_DROPS(K);
    int prev[FSQ_PEPTIDE_MAX_CHANNELS], drops = 0;
    unsigned long long k = 0ull;
    bool up = false, unkeyed = false;
#pragma unroll
    for (int ch = 0; ch < FSQ_PEPTIDE_MAX_CHANNELS; ++ch) {
        prev[ch] = 0;
        if (ch < K) {
            prev[ch] = row0[ch * channel_stride];
            unkeyed |= prev[ch] > 15;
            k |= (unsigned long long)(prev[ch] & 15) << (ch == 0 ? 0 : 64 - 4 * (K - ch));
        }
    }
    for (int f = 1; f < frames; ++f) {
#pragma unroll
        for (int ch = 0; ch < FSQ_PEPTIDE_MAX_CHANNELS; ++ch) {
            if (ch < K) {
                const int c = row0[ch * channel_stride + f];
                if (c > prev[ch]) up = true;
                for (int j = c; j < prev[ch]; ++j) {
                    if (drops < D) k |= (unsigned long long)(f | (ch << 6)) << (4 + B * drops);
                    ++drops;
                }
                prev[ch] = c;
            }
        }
    }
    *key = k;
    return up ? ROW_NONE : (unkeyed || drops > D) ? ROW_UNKEYED : ROW_SIGNAL;
}

// The tally of kss_tally and kss_tally_joint: row_key_of(g, &key) classifies row g and gives its key.
template <class RowKey>
__device__ __forceinline__ void tally_rows(const RowKey row_key_of, const int32_t* __restrict__ g_point,
                                           const uint8_t* __restrict__ g_valid, const long long n_rows, const int n_points,
                                           const int slots, unsigned long long* __restrict__ g_keys, long long* __restrict__ g_counts,
                                           long long* __restrict__ g_none, long long* __restrict__ g_unkeyed,
                                           int32_t* __restrict__ g_overflow)
{
    __shared__ unsigned long long l_key[TALLY_LDS_SLOTS];
    __shared__ int l_cnt[TALLY_LDS_SLOTS];
    __shared__ int l_first;                                                         // the lowest point among the block's signals
    const int tid = threadIdx.x;
    for (long long base = (long long)blockIdx.x * TALLY_BLOCK; base < n_rows; base += (long long)gridDim.x * TALLY_BLOCK) {
        for (int t = tid; t < TALLY_LDS_SLOTS; t += TALLY_BLOCK) { l_key[t] = FSQ_SIGNAL_EMPTY; l_cnt[t] = 0; }
        if (tid == 0) l_first = 0x7fffffff;
        __syncthreads();
        const long long g = base + tid;
        bool has = false;
        int point = 0;
        unsigned long long key = 0ull;
        if (g < n_rows && (!g_valid || g_valid[g])) {
            point = g_point[g];
            if (point >= 0 && point < n_points) {
                const int what = row_key_of(g, &key);
                if (what == ROW_SIGNAL) {
                    has = true;
                    atomicMin(&l_first, point);
                } else {
                    atomicAdd((unsigned long long*)(what == ROW_NONE ? &g_none[point] : &g_unkeyed[point]), 1ull);
                }
            }
        }
        __syncthreads();
        const int first = l_first;
        if (has) {
            const int lp = point - first;
            bool done = false;
            if (lp < TALLY_POINTS) {
                const unsigned h = (unsigned)key_hash(key);
                for (int i = 0; i < TALLY_LDS_PROBES && !done; ++i) {
                    const int at = lp * TALLY_SUB + (int)((h + (unsigned)i) & (unsigned)(TALLY_SUB - 1));
                    const unsigned long long was = atomicCAS(&l_key[at], (unsigned long long)FSQ_SIGNAL_EMPTY, key);
                    if (was == FSQ_SIGNAL_EMPTY || was == key) {
                        atomicAdd(&l_cnt[at], 1);
                        done = true;
                    }
                }
            }
            if (!done) table_add(g_keys, g_counts, g_overflow, point, slots, key, 1);
        }
        __syncthreads();
        for (int t = tid; t < TALLY_LDS_SLOTS; t += TALLY_BLOCK) {
            const unsigned long long k = l_key[t];
            if (k != FSQ_SIGNAL_EMPTY) table_add(g_keys, g_counts, g_overflow, first + t / TALLY_SUB, slots, k, l_cnt[t]);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(TALLY_BLOCK)
kss_tally(const uint8_t* __restrict__ g_rows, const int frames, const int32_t* __restrict__ g_point, const uint8_t* __restrict__ g_valid,
          const long long n_rows, const int n_points, const int slots, unsigned long long* __restrict__ g_keys,
          long long* __restrict__ g_counts, long long* __restrict__ g_none, long long* __restrict__ g_unkeyed,
          int32_t* __restrict__ g_overflow)
{
    tally_rows([&](long long g, unsigned long long* key) { return row_key(g_rows + g * frames, frames, key); }, g_point, g_valid, n_rows,
               n_points, slots, g_keys, g_counts, g_none, g_unkeyed, g_overflow);
}

// g_rows is [K][n_rows][frames]: molecule g's channel k row at (k * n_rows + g) * frames
__global__ void __launch_bounds__(TALLY_BLOCK)
kss_tally_joint(const uint8_t* __restrict__ g_rows, const int K, const int frames, const int32_t* __restrict__ g_point,
                const uint8_t* __restrict__ g_valid, const long long n_rows, const int n_points, const int slots,
                unsigned long long* __restrict__ g_keys, long long* __restrict__ g_counts, long long* __restrict__ g_none,
                long long* __restrict__ g_unkeyed, int32_t* __restrict__ g_overflow)
{
    const long long channel_stride = n_rows * frames;
    tally_rows([&](long long g, unsigned long long* key) { return joint_row_key(g_rows + g * frames, channel_stride, K, frames, key); },
               g_point, g_valid, n_rows, n_points, slots, g_keys, g_counts, g_none, g_unkeyed, g_overflow);
}

__global__ void __launch_bounds__(256)
kss_lookup(const unsigned long long* __restrict__ g_keys, const long long* __restrict__ g_counts, const int n_points, const int slots,
           const unsigned long long* __restrict__ g_wanted, const long long n_out, long long* __restrict__ g_out)
{
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n_out; t += (long long)gridDim.x * blockDim.x) {
        const int point = (int)(t % n_points);
        const unsigned long long key = g_wanted[t / n_points];
        const long long base = (long long)point * slots;
        const unsigned h = (unsigned)key_hash(key);
        long long count = 0;
        for (int i = 0; i < slots; ++i) {
            const long long at = base + (long long)((h + (unsigned)i) & (unsigned)(slots - 1));
            const unsigned long long k = g_keys[at];
            if (k == key) count = g_counts[at];
            if (k == key || k == FSQ_SIGNAL_EMPTY) break;
        }
        g_out[t] = count;
    }
}

// ---- the scores ----

__global__ void __launch_bounds__(WAVE)
kss_scores(const long long* __restrict__ g_obs, const uint8_t* __restrict__ g_in_obs, const uint8_t* __restrict__ g_admitted,
           const uint8_t* __restrict__ g_heatmap, const long long* __restrict__ g_fit, const long long* __restrict__ g_fit_total,
           const int S, const int P, const FsqScoreParams prm, double* __restrict__ g_score, double* __restrict__ g_factor,
           int32_t* __restrict__ g_status, double* __restrict__ g_contrib)
{
    const int k = blockIdx.x * WAVE + threadIdx.x;
    if (k >= P) return;
    const double nan = __builtin_nan("");
    const int metric = prm.metric;
    auto paired = [&](int i, long long o, long long f) { return score_paired(prm, g_admitted[i], g_in_obs[i], o, f); };
    if (g_contrib)
        for (int i = 0; i < S; ++i) g_contrib[(long long)i * P + k] = nan;
    g_score[k] = nan;
    // the pairs and the factor (:288-358)
    long long sum_o = 0, sum_f = 0;
    int n_paired = 0;
    for (int i = 0; i < S; ++i) {
        const long long o = g_obs[i], f = g_fit[(long long)i * P + k];
        if (paired(i, o, f)) { sum_o += o; sum_f += f; ++n_paired; }
    }
    double factor = 1.0;
    if ((prm.normalization & FSQ_SCORE_NORMALIZE_COUNTS) && n_paired > 0 && sum_f > 0) {
        factor = (double)sum_o / (double)sum_f;
    } else if (prm.normalization & FSQ_SCORE_HEATMAP_NORMALIZE_COUNTS) {
        long long heat_o = 0, heat_f = 0;
        for (int i = 0; i < S; ++i) {
            const long long f = g_fit[(long long)i * P + k];
            if (g_heatmap[i] && (g_in_obs[i] || f > 0)) { heat_o += g_in_obs[i] ? g_obs[i] : 0; heat_f += f; }
        }
        if (heat_f == 0) {
            g_factor[k] = nan;
            g_status[k] = FSQ_SCORE_DIVZERO;
            return;
        }
        factor = (double)heat_o / (double)heat_f;
    }
    g_factor[k] = factor;
    if (n_paired == 0) {
        g_status[k] = FSQ_SCORE_EMPTY;
        return;
    }
    // the contributions (:364-503), in key order: the terms are fsq_score_term.h's
    const long long n_obs = prm.n_observed, n_fit = g_fit_total[k];
    double acc = 0.0;
    int n_contrib = 0;
    bool divzero = false, domain = false;
    for (int i = 0; i < S; ++i) {
        const long long oi = g_obs[i], fi = g_fit[(long long)i * P + k];
        if (!paired(i, oi, fi)) continue;
        const ScoreTerm t = score_term(metric, oi, fi, factor, n_obs, n_fit);
        divzero |= t.divzero;
        domain |= t.domain;
        if (!t.have) continue;
        ++n_contrib;
        if (g_contrib) g_contrib[(long long)i * P + k] = t.c;
        acc = score_accumulate(acc, t);
    }
    if (domain || divzero) {
        g_status[k] = domain ? FSQ_SCORE_DOMAIN : FSQ_SCORE_DIVZERO;
        return;
    }
    double result;
    if (!score_result(metric, acc, n_contrib, &result)) {
        g_status[k] = FSQ_SCORE_DOMAIN;
        return;
    }
    g_score[k] = result;
    g_status[k] = FSQ_SCORE_OK;
}

bool pow2(int64_t x) { return x > 0 && (x & (x - 1)) == 0; }

bool tables_ok(int32_t n_points, int32_t slots)
{
    return n_points >= 1 && slots >= 1 && slots <= FSQ_SIGNAL_MAX_SLOTS && pow2(slots) && (int64_t)n_points * slots <= (int64_t)1 << 40;
}

}  // namespace

extern "C" int fsq_peptide_simulate_points(const FsqPeptideSimParams* base, const FsqSweepPoint* d_points, int64_t n_points,
                                           int64_t n_per_point, int64_t molecule_stride, int64_t first_row, int64_t n_rows,
                                           uint8_t* d_counts, double* d_intensity, uint64_t* d_category, void* stream)
{
    if (!params_ok(base, 0)) return FSQ_EINVAL;
    if (n_points < 1 || n_per_point < 1 || molecule_stride < 0 || first_row < 0 || n_rows < 0) return FSQ_EINVAL;
    const __int128 total = (__int128)n_points * n_per_point;
    if ((__int128)first_row + n_rows > total) return FSQ_EINVAL;
    if ((__int128)base->first_molecule + (__int128)(n_points - 1) * molecule_stride + n_per_point - 1 > (__int128)INT64_MAX) return FSQ_EINVAL;
    if (!d_points) return FSQ_EINVAL;
    if (n_rows == 0) return FSQ_OK;
    if (!d_counts || !d_intensity || !d_category) return FSQ_EINVAL;
    const int frames = base->num_mocks + base->num_edmans + 1;
    const int64_t chunks = (n_rows + WAVE - 1) / WAVE;
    const int64_t blocks = chunks < MAX_BLOCKS ? chunks : MAX_BLOCKS;
    hipLaunchKernelGGL(kss_simulate_points, dim3((unsigned)blocks), dim3(WAVE), points_lds_bytes(frames), (hipStream_t)stream, *base,
                       d_points, (long long)n_per_point, (long long)molecule_stride, (long long)first_row, (long long)n_rows, d_counts,
                       d_intensity, (unsigned long long*)d_category);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_signal_tally(const uint8_t* d_rows, int32_t frames, const int32_t* d_point, const uint8_t* d_valid, int64_t n_rows,
                                int32_t n_points, int32_t slots, uint64_t* d_keys, int64_t* d_counts, int64_t* d_none,
                                int64_t* d_unkeyed, int32_t* d_overflow, void* stream)
{
    if (frames < 1 || frames > FSQ_SIGNAL_MAX_FRAMES || n_rows < 0 || !tables_ok(n_points, slots)) return FSQ_EINVAL;
    if (!d_keys || !d_counts || !d_none || !d_unkeyed || !d_overflow) return FSQ_EINVAL;
    if (n_rows == 0) return FSQ_OK;
    if (!d_rows || !d_point) return FSQ_EINVAL;
    const int64_t chunks = (n_rows + TALLY_BLOCK - 1) / TALLY_BLOCK;
    const int64_t blocks = chunks < MAX_BLOCKS ? chunks : MAX_BLOCKS;
    hipLaunchKernelGGL(kss_tally, dim3((unsigned)blocks), dim3(TALLY_BLOCK), 0, (hipStream_t)stream, d_rows, (int)frames, d_point, d_valid,
                       (long long)n_rows, (int)n_points, (int)slots, (unsigned long long*)d_keys, (long long*)d_counts,
                       (long long*)d_none, (long long*)d_unkeyed, d_overflow);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_signal_tally_joint(const uint8_t* d_rows, int32_t n_channels, int32_t frames, const int32_t* d_point,
                                      const uint8_t* d_valid, int64_t n_rows, int32_t n_points, int32_t slots, uint64_t* d_keys,
                                      int64_t* d_counts, int64_t* d_none, int64_t* d_unkeyed, int32_t* d_overflow, void* stream)
{
    if (n_channels < 1 || n_channels > FSQ_PEPTIDE_MAX_CHANNELS) return FSQ_EINVAL;
    if (frames < 1 || frames > FSQ_SIGNAL_MAX_FRAMES || n_rows < 0 || !tables_ok(n_points, slots)) return FSQ_EINVAL;
    if ((__int128)n_rows * frames * n_channels > (__int128)INT64_MAX) return FSQ_EINVAL;
    if (!d_keys || !d_counts || !d_none || !d_unkeyed || !d_overflow) return FSQ_EINVAL;
    if (n_rows == 0) return FSQ_OK;
    if (!d_rows || !d_point) return FSQ_EINVAL;
    const int64_t chunks = (n_rows + TALLY_BLOCK - 1) / TALLY_BLOCK;
    const int64_t blocks = chunks < MAX_BLOCKS ? chunks : MAX_BLOCKS;
    hipLaunchKernelGGL(kss_tally_joint, dim3((unsigned)blocks), dim3(TALLY_BLOCK), 0, (hipStream_t)stream, d_rows, (int)n_channels,
                       (int)frames, d_point, d_valid, (long long)n_rows, (int)n_points, (int)slots, (unsigned long long*)d_keys,
                       (long long*)d_counts, (long long*)d_none, (long long*)d_unkeyed, d_overflow);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_signal_lookup(const uint64_t* d_keys, const int64_t* d_counts, int32_t n_points, int32_t slots,
                                 const uint64_t* d_wanted, int32_t n_wanted, int64_t* d_out, void* stream)
{
    if (!tables_ok(n_points, slots) || n_wanted < 0) return FSQ_EINVAL;
    if (!d_keys || !d_counts) return FSQ_EINVAL;
    if (n_wanted == 0) return FSQ_OK;
    if (!d_wanted || !d_out) return FSQ_EINVAL;
    const int64_t n_out = (int64_t)n_wanted * n_points;
    const int64_t chunks = (n_out + 255) / 256;
    const int64_t blocks = chunks < MAX_BLOCKS ? chunks : MAX_BLOCKS;
    hipLaunchKernelGGL(kss_lookup, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)d_keys,
                       (const long long*)d_counts, (int)n_points, (int)slots, (const unsigned long long*)d_wanted, (long long)n_out,
                       (long long*)d_out);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_signal_scores(const int64_t* d_observed, const uint8_t* d_in_observed, const uint8_t* d_admitted,
                                 const uint8_t* d_heatmap, const int64_t* d_fit, const int64_t* d_fit_total, int32_t n_keys,
                                 int32_t n_points, const FsqScoreParams* prm, double* d_score, double* d_factor, int32_t* d_status,
                                 double* d_contrib, void* stream)
{
    if (!prm || n_keys < 0 || n_points < 1) return FSQ_EINVAL;
    if (prm->metric < 0 || prm->metric >= FSQ_SCORE_N_METRICS || (prm->normalization & ~3)) return FSQ_EINVAL;
    if (prm->n_observed < 0 || prm->n_observed > 2147483647ll) return FSQ_EINVAL;       // (oi * (n_observed - oi) stays within 64 bits)
    if (prm->has_cutoff && prm->small_count_cutoff != prm->small_count_cutoff) return FSQ_EINVAL;
    if (!d_fit_total || !d_score || !d_factor || !d_status) return FSQ_EINVAL;
    if (n_keys > 0 && (!d_observed || !d_in_observed || !d_admitted || !d_heatmap || !d_fit)) return FSQ_EINVAL;
    hipLaunchKernelGGL(kss_scores, dim3((unsigned)((n_points + WAVE - 1) / WAVE)), dim3(WAVE), 0, (hipStream_t)stream,
                       (const long long*)d_observed, d_in_observed, d_admitted, d_heatmap, (const long long*)d_fit,
                       (const long long*)d_fit_total, (int)n_keys, (int)n_points, *prm, d_score, d_factor, d_status, d_contrib);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
