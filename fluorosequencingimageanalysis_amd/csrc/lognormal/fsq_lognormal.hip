// fsq_lognormal.hip - lognormal fluor-count fit of track photometries (C ABI of include/fsq_lognormal.h).
//
// MCsimlib._intensities_to_signal_lognormal_v8 (:5413-5466) scores every non-increasing count sequence; here one wavefront
// takes one track and touches only the sequences that pass the reference's three rules:
//   1. pre-pass: L[f] = log(I[f]); per (frame, count) the density S[f][v] and whether the count is admissible there
//      (category rule, deviation rule); backwards over the frames W[f][v] = the number of admissible completions of frames
//      f .. T-1 that hold v at f (multi-drop rule applied between f and f + 1), saturating.  sum_v W[0][v] is the exact
//      number of surviving sequences; above `budget` the track is reported and left alone.
//   2. the survivors, numbered in the reference's enumeration order, are cut into 64 contiguous rank ranges.  A lane
//      unranks the start of its range from W and steps from one survivor to the next: the deepest frame whose count can
//      still go down, then the largest admissible counts after it.  The prefix products (left to right from 1.0, as
//      reduce(mul, scores, 1.0)) of the current sequence sit in LDS, one column per lane, so a step costs one multiply
//      per changed frame.  A lane keeps its first strictly greatest total.
//   3. the wave takes the greatest total and among equals the smallest rank: the reference's `total_score > best_score`
//      in enumeration order.
// No recursion; every loop is bounded by T, by max_possible + 1 or by the lane's share of the counted survivors.
#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_lognormal.h"
#include "../libm/fsq_glibc_exp.h"
#include "../libm/fsq_glibc_log.h"

namespace {

constexpr int WAVE = 64;
constexpr int MAX_BLOCKS = 16384;
constexpr unsigned long long SAT = (unsigned long long)FSQ_LOGNORMAL_MAX_BUDGET;
constexpr double NORM_PDF_C = 0x1.40d931ff62705p+1;          // np.sqrt(2 * np.pi), scipy's _norm_pdf_C

// The counts of one sequence, 4 bits per frame, in one register vector (an indexed array or struct would live in scratch).
typedef unsigned long long Seq __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned seq_get(Seq s, int f)
{
    return (unsigned)(s[f >> 4] >> ((f & 15) * 4)) & 15u;
}

__device__ __forceinline__ Seq seq_put(Seq s, int f, unsigned v)
{
    const int sh = (f & 15) * 4;
    s[f >> 4] = (s[f >> 4] & ~(15ull << sh)) | ((unsigned long long)v << sh);
    return s;
}

// Counts admissible at a frame after count p: at most p, and without multi-drop at least p - 1.
__device__ __forceinline__ unsigned after_mask(unsigned p, bool multidrop)
{
    unsigned m = (2u << p) - 1u;
    if (!multidrop && p > 0) m &= ~((1u << (p - 1)) - 1u);
    return m;
}

// LDS of one block: W and S [T][V], the prefix products [T + 1][WAVE], the log intensities and the admissibility masks [T],
// the means [16]
size_t lds_bytes(int Tcap, int V)
{
    return (size_t)Tcap * V * 16 + (size_t)(Tcap + 1) * WAVE * 8 + (size_t)Tcap * 8 + 16 * 8 + (size_t)Tcap * 4;
}

__global__ void __launch_bounds__(WAVE) kln_fit(const double* __restrict__ intensity, const unsigned long long* __restrict__ category,
                                                const int32_t* __restrict__ n_frames, long long n_tracks, int max_frames,
                                                FsqLognormalParams prm, int32_t* __restrict__ status,
                                                uint8_t* __restrict__ best_seq, double* __restrict__ best_score,
                                                double* __restrict__ frame_score, long long* __restrict__ n_surviving)
{
    extern __shared__ unsigned long long lds[];
    const int lane = threadIdx.x;
    const int m = prm.max_possible, V = m + 1, Tcap = max_frames;
    const bool multidrop = prm.allow_multidrop != 0;
    unsigned long long* W = lds;                                   // [Tcap][V] completions holding v at f
    double* S = (double*)(W + (size_t)Tcap * V);                   // [Tcap][V] densities
    double* P = S + (size_t)Tcap * V;                              // [Tcap + 1][WAVE] prefix products, one column per lane
    double* Lf = P + (size_t)(Tcap + 1) * WAVE;                    // [Tcap] log intensities
    double* Mn = Lf + Tcap;                                        // [16] log_fluor_means (indexed per lane: not from the kernel arguments)
    unsigned* ok = (unsigned*)(Mn + 16);                           // [Tcap] bit v: W[f][v] > 0
    double* red_best = P;                                          // the reduction reuses P's first two rows
    long long* red_rank = (long long*)(P + WAVE);

#pragma unroll
    for (int i = 0; i < FSQ_LOGNORMAL_MAX_POSSIBLE + 1; ++i)
        if (lane == i) Mn[i] = prm.log_fluor_means[i];
    __syncthreads();
    for (long long t = blockIdx.x; t < n_tracks; t += gridDim.x) {
        const int T = n_frames[t];
        const size_t row = (size_t)t * max_frames;
        int st = FSQ_LOGNORMAL_INVALID;
        unsigned long long total = 0;
        double best = -1.0;
        long long best_rank = -1;
        Seq bs = {0, 0, 0, 0};
        int win_lane = -1;
        if (T >= 1 && T <= Tcap) {                                 // (uniform over the wave)
            const unsigned long long cat = category[t];
            for (int f = lane; f < T; f += WAVE) {
                const double I = intensity[row + f];
                Lf[f] = I > 0 ? ln_log(I) : -10000.0;
            }
            __syncthreads();
            for (int idx = lane; idx < T * V; idx += WAVE) {
                const int f = idx / V, v = idx - f * V;
                const bool on = (cat >> f) & 1ull;
                double s = 1.0;
                bool adm = !on;
                if (v > 0) {
                    const double d = Lf[f] - Mn[v - 1];
                    const double z = d / prm.beta_sigma;
                    adm = on && !(__builtin_fabs(d) / prm.beta_sigma > prm.max_deviation);
                    s = sf_exp<false>(-(z * z) / 2.0, 0.0) / NORM_PDF_C / prm.beta_sigma;
                }
                S[idx] = s;
                W[idx] = adm ? 1ull : 0ull;
            }
            __syncthreads();
            for (int f = T - 2; f >= 0; --f) {
                if (lane < V && W[f * V + lane] != 0) {
                    const int lo = (!multidrop && lane > 0) ? lane - 1 : 0;
                    unsigned long long sum = 0;
                    for (int u = lane; u >= lo; --u) {
                        sum += W[(f + 1) * V + u];
                        sum = sum < SAT ? sum : SAT;
                    }
                    W[f * V + lane] = sum;
                }
                __syncthreads();
            }
            for (int f = lane; f < T; f += WAVE) {
                unsigned mask = 0;
                for (int v = 0; v < V; ++v) mask |= (W[f * V + v] != 0 ? 1u : 0u) << v;
                ok[f] = mask;
            }
            for (int v = 0; v < V; ++v) {
                total += W[v];
                total = total < SAT ? total : SAT;
            }
            __syncthreads();
            st = total == 0 ? FSQ_LOGNORMAL_NONE : (total >= SAT || total > (unsigned long long)prm.budget) ?   // (a saturated count is not exact: never enumerated)
                 FSQ_LOGNORMAL_OVER_BUDGET : FSQ_LOGNORMAL_FOUND;
        }
        if (st == FSQ_LOGNORMAL_FOUND) {                           // (uniform)
            const unsigned long long chunk = total / WAVE, rem = total % WAVE;
            const unsigned long long mine = chunk + ((unsigned)lane < rem ? 1 : 0);
            const unsigned long long first = (unsigned long long)lane * chunk + ((unsigned)lane < rem ? (unsigned)lane : rem);
            if (mine > 0) {
                Seq cur = {0, 0, 0, 0};
                // unrank `first`: at each frame skip whole blocks of completions, largest count first
                unsigned long long r = first;
                unsigned p = (unsigned)m;
                double prod = 1.0;
                P[lane] = prod;
                bool good = true;
                for (int f = 0; f < T && good; ++f) {
                    const int lo = (f > 0 && !multidrop && p > 0) ? (int)p - 1 : 0;
                    int v = (int)p;
                    for (; v >= lo; --v) {
                        const unsigned long long c = W[f * V + v];
                        if (r < c) break;
                        r -= c;
                    }
                    good = v >= lo;
                    if (good) {
                        cur = seq_put(cur, f, (unsigned)v);
                        prod = prod * S[f * V + v];
                        P[(f + 1) * WAVE + lane] = prod;
                        p = (unsigned)v;
                    }
                }
                for (unsigned long long it = 0; good;) {
                    const double tot = P[T * WAVE + lane];
                    if (tot > best) {
                        best = tot;
                        best_rank = (long long)(first + it);
                        bs = cur;
                    }
                    if (++it >= mine) break;
                    // the next survivor: the deepest frame whose count can go down ...
                    int f = T - 1;
                    unsigned mask = 0;
                    for (; f >= 0; --f) {
                        const unsigned cv = seq_get(cur, f);
                        mask = ok[f] & ((1u << cv) - 1u);
                        if (f > 0) mask &= after_mask(seq_get(cur, f - 1), multidrop);
                        if (mask) break;
                    }
                    if (f < 0) break;
                    unsigned v = 31u - (unsigned)__builtin_clz(mask);
                    cur = seq_put(cur, f, v);
                    prod = P[f * WAVE + lane] * S[f * V + v];
                    P[(f + 1) * WAVE + lane] = prod;
                    // ... then the largest admissible counts after it
                    for (int g = f + 1; g < T; ++g) {
                        mask = ok[g] & after_mask(v, multidrop);
                        if (!mask) { good = false; break; }
                        v = 31u - (unsigned)__builtin_clz(mask);
                        cur = seq_put(cur, g, v);
                        prod = prod * S[g * V + v];
                        P[(g + 1) * WAVE + lane] = prod;
                    }
                }
            }
            __syncthreads();
            red_best[lane] = best;
            red_rank[lane] = best_rank;
            __syncthreads();
            double wb = -1.0;
            long long wr = -1;
            for (int l = 0; l < WAVE; ++l) {
                const double b = red_best[l];
                const long long rk = red_rank[l];
                if (rk >= 0 && (win_lane < 0 || b > wb || (b == wb && rk < wr))) {
                    wb = b;
                    wr = rk;
                    win_lane = l;
                }
            }
            if (win_lane < 0) st = FSQ_LOGNORMAL_NONE;                // (every total was NaN)
            best = wb;
        }
        // outputs: every element of the track's rows
        if (st == FSQ_LOGNORMAL_FOUND) {
            if (lane == win_lane) {
                for (int f = 0; f < T; ++f) {
                    const unsigned v = seq_get(bs, f);
                    best_seq[row + f] = (uint8_t)v;
                    frame_score[row + f] = S[f * V + v];
                }
            }
            for (int f = T + lane; f < max_frames; f += WAVE) {
                best_seq[row + f] = 0;
                frame_score[row + f] = 0.0;
            }
        } else {
            for (int f = lane; f < max_frames; f += WAVE) {
                best_seq[row + f] = 0;
                frame_score[row + f] = 0.0;
            }
        }
        if (lane == 0) {
            status[t] = st;
            best_score[t] = st == FSQ_LOGNORMAL_FOUND ? best : -1.0;
            n_surviving[t] = (long long)total;
        }
        __syncthreads();                                           // the next track reuses the tables
    }
}

__global__ void __launch_bounds__(256) kln_log(const double* __restrict__ x, double* __restrict__ out, long long n)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = ln_log(x[i]);
}

bool shape_ok(int64_t n_tracks, int32_t max_frames) { return n_tracks >= 0 && max_frames >= 1 && max_frames <= FSQ_LOGNORMAL_MAX_FRAMES; }

bool params_ok(const FsqLognormalParams* p)
{
    if (!p || p->max_possible < 1 || p->max_possible > FSQ_LOGNORMAL_MAX_POSSIBLE) return false;
    if (!(p->beta_sigma > 0) || p->beta_sigma > 0x1.fffffffffffffp+1023) return false;
    if (p->max_deviation != p->max_deviation) return false;
    for (int i = 0; i < p->max_possible; ++i)
        if (!(__builtin_fabs(p->log_fluor_means[i]) <= 0x1.fffffffffffffp+1023)) return false;
    return p->budget >= 1 && p->budget <= FSQ_LOGNORMAL_MAX_BUDGET;
}

}  // namespace

extern "C" int64_t fsq_lognormal_workspace_bytes(int64_t n_tracks, int32_t max_frames)
{
    return shape_ok(n_tracks, max_frames) ? 0 : -1;                // the tables of a track live in LDS
}

extern "C" int fsq_lognormal_fit(const double* d_intensity, const uint64_t* d_category, const int32_t* d_n_frames, int64_t n_tracks,
                                 int32_t max_frames, const FsqLognormalParams* prm, int32_t* d_status, uint8_t* d_best_seq,
                                 double* d_best_score, double* d_frame_score, int64_t* d_n_surviving, void* d_ws,
                                 int64_t ws_bytes, void* stream)
{
    (void)d_ws;
    if (!shape_ok(n_tracks, max_frames) || !params_ok(prm) || ws_bytes < 0) return FSQ_EINVAL;
    if (n_tracks == 0) return FSQ_OK;
    if (!d_intensity || !d_category || !d_n_frames || !d_status || !d_best_seq || !d_best_score || !d_frame_score || !d_n_surviving)
        return FSQ_EINVAL;
    const size_t lds = lds_bytes(max_frames, prm->max_possible + 1);
    const int64_t blocks = n_tracks < MAX_BLOCKS ? n_tracks : MAX_BLOCKS;
    hipLaunchKernelGGL(kln_fit, dim3((unsigned)blocks), dim3(WAVE), lds, (hipStream_t)stream, d_intensity,
                       (const unsigned long long*)d_category, d_n_frames, (long long)n_tracks, (int)max_frames, *prm, d_status,
                       d_best_seq, d_best_score, d_frame_score, (long long*)d_n_surviving);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_lognormal_log(const double* d_x, double* d_out, int64_t n, void* stream)
{
    if (n < 0) return FSQ_EINVAL;
    if (n == 0) return FSQ_OK;
    if (!d_x || !d_out) return FSQ_EINVAL;
    const int64_t blocks = (n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096;
    hipLaunchKernelGGL(kln_log, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, d_x, d_out, (long long)n);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
