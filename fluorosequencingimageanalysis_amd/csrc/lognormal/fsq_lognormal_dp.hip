// fsq_lognormal_dp.hip - the lognormal fluor-count fit by exact dynamic programme (C ABI of include/fsq_lognormal_dp.h).
//
// fsq_lognormal.hip's winner without its enumeration: one wavefront takes one track, a lane takes one count.
//   1. pre-pass, as kln_fit's: L[f] = log(I[f]); per (frame, count) the density S[f][v] and whether the count is admissible
//      there; backwards over the frames W[f][v] = the number of admissible completions of frames f .. T-1 that hold v at f
//      under the mode's transition rule, saturating.  sum_v W[0][v] is the exact number of surviving sequences and W != 0 the
//      completability mask.  (The pre-pass is restated here, not shared: kln_fit's compiled resources stay what they were.)
//   2. forward: P[f][v] = fl(max_u P[f-1][u] * S[f][v]) over the completable predecessors u of v, two rows in LDS;
//      B = max_v P[T-1][v].
//   3. backward: N[T-1][v] = B, N[f][u] = min over allowed v of Q[f+1][v]; Q[f][v] = min_prefix(S[f][v], N[f][v]), the
//      least double p >= 0 with fl(p * S) >= N.  N is +inf where W == 0.
//   4. the winner: from p = 1, at each frame the largest allowed count v with fl(p * S[f][v]) >= N[f][v] (one ballot).
// The argument that this is the reference's winner, bit for bit and with its tie rule, is in the header.
// No recursion; every loop is bounded by T, by max_possible + 1 or by 63.
#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_lognormal_dp.h"
#include "../libm/fsq_glibc_exp.h"
#include "../libm/fsq_glibc_log.h"

namespace {

constexpr int WAVE = 64;
constexpr int MAX_BLOCKS = 16384;
constexpr unsigned long long SAT = (unsigned long long)FSQ_LOGNORMAL_MAX_BUDGET;
constexpr double NORM_PDF_C = 0x1.40d931ff62705p+1;          // np.sqrt(2 * np.pi), scipy's _norm_pdf_C
constexpr int VMAX = FSQ_LOGNORMAL_MAX_POSSIBLE + 1;
constexpr unsigned long long BITS_DBL_MAX = 0x7fefffffffffffffull;
constexpr unsigned long long BITS_INF = 0x7ff0000000000000ull;

__device__ __forceinline__ double from_bits(unsigned long long b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ unsigned long long to_bits(double x) { return (unsigned long long)__double_as_longlong(x); }

// The least double p >= 0 with fl(p * s) >= n (s >= 0 finite, n not NaN): 0 where n <= 0, +inf where no finite p does it.
// Non-negative doubles are ordered like their bit patterns and p -> fl(p * s) is non-decreasing, so the answer is the
// least bit pattern that passes.  n / s and its two neighbours usually bracket it; the search over the bit pattern is
// the fallback (subnormal n or s, a quotient that over- or underflows).
__device__ double min_prefix(double s, double n)
{
    if (n <= 0.0) return 0.0;
    if (!(from_bits(BITS_DBL_MAX) * s >= n)) return from_bits(BITS_INF);
    const unsigned long long q = to_bits(n / s);               // (s > 0 here: DBL_MAX * 0 >= n > 0 fails)
    if (q >= 1 && q <= BITS_DBL_MAX) {
        const bool at = from_bits(q) * s >= n, below = from_bits(q - 1) * s >= n;
        if (at && !below) return from_bits(q);
        if (!at && q < BITS_DBL_MAX && from_bits(q + 1) * s >= n) return from_bits(q + 1);
        if (below && q >= 2 && !(from_bits(q - 2) * s >= n)) return from_bits(q - 1);
    }
    unsigned long long lo = 0, hi = BITS_DBL_MAX;              // fails at lo (0 * s = 0 < n), passes at hi
    for (int it = 0; it < 63 && hi - lo > 1; ++it) {
        const unsigned long long mid = lo + ((hi - lo) >> 1);
        if (from_bits(mid) * s >= n) hi = mid; else lo = mid;
    }
    return from_bits(hi);
}

// LDS of one block: W, S and N [T][V], P and Q [2][16], the log intensities [T], the means [16], the winner's counts [T]
size_t lds_bytes(int Tcap, int V)
{
    return (size_t)Tcap * V * 24 + (size_t)(3 * VMAX) * 8 + (size_t)Tcap * 8 + 16 * 8 + (size_t)((Tcap + 7) & ~7);
}

__global__ void __launch_bounds__(WAVE) kln_fit_dp(const double* __restrict__ intensity, const unsigned long long* __restrict__ category,
                                                   const int32_t* __restrict__ n_frames, long long n_tracks, int max_frames,
                                                   FsqLognormalParams prm, int upsteps, int32_t* __restrict__ status,
                                                   uint8_t* __restrict__ best_seq, double* __restrict__ best_score,
                                                   double* __restrict__ frame_score, long long* __restrict__ n_surviving)
{
    extern __shared__ unsigned long long lds[];
    const int lane = threadIdx.x;
    const int m = prm.max_possible, V = m + 1, Tcap = max_frames;
    const bool multidrop = prm.allow_multidrop != 0;
    unsigned long long* W = lds;                                   // [Tcap][V] completions holding v at f
    double* S = (double*)(W + (size_t)Tcap * V);                   // [Tcap][V] densities
    double* N = S + (size_t)Tcap * V;                              // [Tcap][V] thresholds
    double* P = N + (size_t)Tcap * V;                              // [2][VMAX] forward rows
    double* Q = P + 2 * VMAX;                                      // [VMAX] least prefixes of the frame after
    double* Lf = Q + VMAX;                                         // [Tcap] log intensities
    double* Mn = Lf + Tcap;                                        // [16] log_fluor_means (indexed per lane: not from the kernel arguments)
    uint8_t* win = (uint8_t*)(Mn + 16);                            // [Tcap] the winner's counts
    // the counts that may follow count `lane`, and the counts that `lane` may follow
    const int succ_lo = (!multidrop && lane > 0) ? lane - 1 : 0, succ_hi = upsteps ? m : (lane < m ? lane : m);
    const int pred_lo = upsteps ? 0 : lane, pred_hi = (multidrop || lane + 1 > m) ? m : lane + 1;

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
                    unsigned long long sum = 0;
                    for (int u = succ_hi; u >= succ_lo; --u) {
                        sum += W[(f + 1) * V + u];
                        sum = sum < SAT ? sum : SAT;
                    }
                    W[f * V + lane] = sum;
                }
                __syncthreads();
            }
            for (int v = 0; v < V; ++v) {
                total += W[v];
                total = total < SAT ? total : SAT;
            }
            st = total == 0 ? FSQ_LOGNORMAL_NONE : FSQ_LOGNORMAL_FOUND;
        }
        if (st == FSQ_LOGNORMAL_FOUND) {                           // (uniform)
            // forward: the greatest prefix product per count, -1 where no completable prefix ends there
            if (lane < V) P[lane] = W[lane] != 0 ? 1.0 * S[lane] : -1.0;
            __syncthreads();
            for (int f = 1; f < T; ++f) {
                const double* prev = P + ((f - 1) & 1) * VMAX;
                if (lane < V) {
                    double p = -1.0;
                    if (W[f * V + lane] != 0) {
                        for (int u = pred_lo; u <= pred_hi; ++u) {
                            const double x = prev[u];
                            p = x > p ? x : p;
                        }
                        if (p >= 0.0) p = p * S[f * V + lane];
                    }
                    P[(f & 1) * VMAX + lane] = p;
                }
                __syncthreads();
            }
            {
                const double* last = P + ((T - 1) & 1) * VMAX;
                for (int v = 0; v < V; ++v) best = last[v] > best ? last[v] : best;
            }
            // backward: the thresholds
            for (int f = T - 1; f >= 0; --f) {
                double n = from_bits(BITS_INF);
                if (lane < V && W[f * V + lane] != 0) {
                    if (f == T - 1) n = best;
                    else
                        for (int v = succ_lo; v <= succ_hi; ++v) {
                            const double q = Q[v];
                            n = q < n ? q : n;
                        }
                }
                __syncthreads();                                   // (every lane has read the Q of frame f + 1)
                if (lane < V) {
                    N[f * V + lane] = n;
                    Q[lane] = W[f * V + lane] != 0 ? min_prefix(S[f * V + lane], n) : from_bits(BITS_INF);
                }
                __syncthreads();
            }
            // the winner: at each frame the largest allowed count that can still reach `best`
            double p = 1.0;
            int lo = 0, hi = m;
            bool good = true;
            for (int f = 0; f < T; ++f) {
                bool pass = false;
                if (good && lane >= lo && lane <= hi) pass = p * S[f * V + lane] >= N[f * V + lane];
                const unsigned long long mask = __ballot(pass);
                if (mask == 0) { good = false; break; }            // (uniform; cannot happen: the thresholds admit the sequence that gave `best`)
                const int v = 63 - __builtin_clzll(mask);
                p = p * S[f * V + v];
                if (lane == 0) win[f] = (uint8_t)v;
                lo = (!multidrop && v > 0) ? v - 1 : 0;
                hi = upsteps ? m : v;
            }
            if (!good) { st = FSQ_LOGNORMAL_NONE; best = -1.0; }
            __syncthreads();
        }
        // outputs: every element of the track's rows
        if (st == FSQ_LOGNORMAL_FOUND) {
            for (int f = lane; f < T; f += WAVE) {
                const unsigned v = win[f];
                best_seq[row + f] = (uint8_t)v;
                frame_score[row + f] = S[f * V + v];
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

bool shape_ok(int64_t n_tracks, int32_t max_frames) { return n_tracks >= 0 && max_frames >= 1 && max_frames <= FSQ_LOGNORMAL_MAX_FRAMES; }

bool params_ok(const FsqLognormalParams* p)                       // fsq_lognormal_fit's, without the budget
{
    if (!p || p->max_possible < 1 || p->max_possible > FSQ_LOGNORMAL_MAX_POSSIBLE) return false;
    if (!(p->beta_sigma > 0) || p->beta_sigma > 0x1.fffffffffffffp+1023) return false;
    if (p->max_deviation != p->max_deviation) return false;
    for (int i = 0; i < p->max_possible; ++i)
        if (!(__builtin_fabs(p->log_fluor_means[i]) <= 0x1.fffffffffffffp+1023)) return false;
    return true;
}

// The header's refusal: a density above 1 whose product over max_frames frames could overflow.
bool may_overflow(double beta_sigma, int32_t max_frames)
{
    const double peak = 1.0 / (NORM_PDF_C * beta_sigma);
    return peak > 1.0 && (double)max_frames * log(peak) >= 700.0;
}

}  // namespace

extern "C" int64_t fsq_lognormal_dp_workspace_bytes(int64_t n_tracks, int32_t max_frames)
{
    return shape_ok(n_tracks, max_frames) ? 0 : -1;                // the tables of a track live in LDS
}

extern "C" int fsq_lognormal_fit_dp(const double* d_intensity, const uint64_t* d_category, const int32_t* d_n_frames, int64_t n_tracks,
                                    int32_t max_frames, const FsqLognormalParams* prm, int32_t* d_status, uint8_t* d_best_seq,
                                    double* d_best_score, double* d_frame_score, int64_t* d_n_surviving, int32_t allow_upsteps,
                                    void* d_ws, int64_t ws_bytes, void* stream)
{
    (void)d_ws;
    if (!shape_ok(n_tracks, max_frames) || !params_ok(prm) || ws_bytes < 0) return FSQ_EINVAL;
    if (may_overflow(prm->beta_sigma, max_frames)) return FSQ_EINVAL;
    if (n_tracks == 0) return FSQ_OK;
    if (!d_intensity || !d_category || !d_n_frames || !d_status || !d_best_seq || !d_best_score || !d_frame_score || !d_n_surviving)
        return FSQ_EINVAL;
    const size_t lds = lds_bytes(max_frames, prm->max_possible + 1);
    const int64_t blocks = n_tracks < MAX_BLOCKS ? n_tracks : MAX_BLOCKS;
    hipLaunchKernelGGL(kln_fit_dp, dim3((unsigned)blocks), dim3(WAVE), lds, (hipStream_t)stream, d_intensity,
                       (const unsigned long long*)d_category, d_n_frames, (long long)n_tracks, (int)max_frames, *prm,
                       allow_upsteps != 0 ? 1 : 0, d_status, d_best_seq, d_best_score, d_frame_score, (long long*)d_n_surviving);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
