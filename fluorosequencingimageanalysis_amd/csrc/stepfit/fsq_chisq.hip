// fsq_chisq.hip - chi-squared step fitting and plateau merge filters (include/fsq_chisq.h), gfx950.
//
//   kcs_split_scan   one wavefront per trace (blocks stride over the traces): chi_squared_step_fitter
//                    (stepfitting_library.py:342-505).  The trace lives in LDS, lanes run over the candidate splits of a
//                    plateau (_split_plateau, :161-176), a wave reduction restates the loop's tie rules, the plateau lists
//                    of the best fit and the counter-fit are linked lists (links in LDS, heights in the block's workspace).
//   kcs_merge_filter one lane per trace: filter_upsteps / filter_small_steps (:732-926)
//   kcs_r_squared    one lane per trace: stepfit_r_squared (:1483-1503)
// Heights are np.mean (numpy's pairwise sum / n), residuals Python's left-to-right sum of pow(lum - height, 2.0) as glibc
// computes it (cs_pow2).  A candidate's value depends on (start, stop, split) only, so values are cached (the whole-trace
// candidates for every counter-fit, each plateau's best split while the plateau lives); nothing is re-associated.
// Table writes are wave-uniform: every lane stores the same value and later reads back its own store.
#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_chisq.h"
#include "fsq_pairwise.h"
#include "fsq_plateau_common.h"

namespace {

constexpr int WAVE = 64;
constexpr int CS_UNKNOWN = -2, CS_NONE = -1;
constexpr int MAX_BLOCKS = 8192;
constexpr int LDS_BYTES_PER_FRAME = 4 * 8 + 7 * 2 + 1, WS_BYTES_PER_FRAME = 5 * 8 + 4;

struct ChiCfg {
    int max_frames, Fp, num_steps, L, ignore_cf, fit_cap;
    double mult, min_mag;
};

// plateau list: node i starts at S[i], has height H[i] and residual sum R[i]; nxt[i] links the nodes in frame order.
// cs / ct cache the node's best split under the list's constraints (CS_UNKNOWN: not scanned, CS_NONE: no split).
// The list walk reads S / nxt / cs / ct of every node: those rows live in LDS (int16: frames < 1024), H and R in the workspace.
struct Table {
    int16_t* S;
    int16_t* nxt;
    int16_t* cs;
    double* ct;
    double* H;
    double* R;
    int cnt;
};

struct Trace {
    const double* lum;      // LDS
    double* sq;             // LDS: squared residuals of one plateau
    uint16_t* bstart;       // LDS: first frame of the best-fit plateau that holds frame f
    uint8_t* chas;          // LDS: indexed by a best-fit plateau's first frame: it holds a counter-fit start
    double* top;            // workspace: value of every split of the whole trace (-1: rejected by min_step_magnitude)
    int n, L;
    double min_mag, B;      // B = len * (max - min) ** 2
};

// value of splitting [a, b] after frame u (:164-172), -1 when the step is below min_step_magnitude
__device__ __forceinline__ double split_value(const Trace& T, int a, int b, int u)
{
    const double* l = T.lum;
    const int nl = u - a + 1, nr = b - u;
    const double hl = np_mean_flat<4>(l + a, nl), hr = np_mean_flat<4>(l + u + 1, nr);
    if (__builtin_fabs(hl - hr) < T.min_mag) return -1.0;
    double rl = 0.0, rr = 0.0;                                         // Python sum from the int 0, left to right
    for (int i = 0; i < nl; i++) rl += cs_pow2(l[a + i] - hl);
    for (int i = 0; i < nr; i++) rr += cs_pow2(l[u + 1 + i] - hr);
    return rl + rr;
}

template <bool COUNTER>
__device__ __forceinline__ bool split_allowed(const Trace& T, int a, int b, int u)
{
    if (COUNTER) {
        // not on a best-fit boundary, and not inside a best-fit plateau that already holds a counter-fit start (:212-228)
        const unsigned bs = T.bstart[u];
        return T.bstart[u + 1] == bs && !T.chas[bs];
    }
    return u - a >= T.L && b - u >= T.L;                               // (:231-239)
}

// _split_plateau on [a, b]: the allowed split of the smallest value not above 2 B, the later one on a tie (`<=`, :173).
// Returns the split frame or CS_NONE; *tot its value.  Wave-uniform result.
template <bool COUNTER>
__device__ __forceinline__ int scan_plateau(const Trace& T, int a, int b, double* tot)
{
    const int lane = threadIdx.x;
    const bool whole = a == 0 && b == T.n - 1;
    double best = 2.0 * T.B;
    int bs = CS_NONE;
    for (int u = a + lane; u < b; u += WAVE) {
        if (!split_allowed<COUNTER>(T, a, b, u)) continue;
        const double v = whole ? T.top[u] : split_value(T, a, b, u);
        if (v >= 0.0 && v <= best) { best = v; bs = u; }
    }
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) {
        const double ov = __shfl_xor(best, m, WAVE);
        const int os = __shfl_xor(bs, m, WAVE);
        if (os >= 0 && (bs < 0 || ov < best || (ov == best && os > bs))) { best = ov; bs = os; }
    }
    *tot = best;
    return bs;
}

// sum of pow(lum - h, 2.0) over [a, b], left to right: the powers in parallel, the additions in order
__device__ __forceinline__ double plateau_residual(const Trace& T, int a, int b, double h)
{
    __syncthreads();
    for (int f = a + threadIdx.x; f <= b; f += WAVE) T.sq[f] = cs_pow2(T.lum[f] - h);
    __syncthreads();
    double r = 0.0;
    for (int f = a; f <= b; f++) r += T.sq[f];
    return r;
}

__device__ __forceinline__ int node_stop(const Table& t, int i, int n) { return (t.nxt[i] >= 0 ? t.S[t.nxt[i]] : n) - 1; }

// _best_split (:182-271): scans the nodes not scanned yet, takes the first node with the smallest value below B (`<`, :255)
// and splits it.  Returns the split frame, or CS_NONE when nothing can be split.
template <bool COUNTER>
__device__ __forceinline__ int best_split(const Trace& T, Table& t)
{
    int pick = -1;
    double pick_v = T.B;
    for (int i = 0; i >= 0; i = t.nxt[i]) {
        if (t.cs[i] == CS_UNKNOWN) {
            const int a = t.S[i], b = node_stop(t, i, T.n);
            double v = 0.0;
            int s = CS_NONE;
            if (b > a && (COUNTER || b - a >= T.L)) s = scan_plateau<COUNTER>(T, a, b, &v);
            t.cs[i] = (int16_t)s;
            t.ct[i] = v;
        }
        if (t.cs[i] >= 0 && t.ct[i] < pick_v) { pick = i; pick_v = t.ct[i]; }
    }
    if (pick < 0) return CS_NONE;
    const int a = t.S[pick], b = node_stop(t, pick, T.n), s = t.cs[pick];
    const double hl = np_mean_flat<4>(T.lum + a, s - a + 1), hr = np_mean_flat<4>(T.lum + s + 1, b - s);
    const double rl = plateau_residual(T, a, s, hl), rr = plateau_residual(T, s + 1, b, hr);
    const int j = t.cnt++;
    t.S[j] = (int16_t)(s + 1); t.H[j] = hr; t.R[j] = rr; t.cs[j] = CS_UNKNOWN; t.nxt[j] = t.nxt[pick];
    t.H[pick] = hl; t.R[pick] = rl; t.cs[pick] = CS_UNKNOWN; t.nxt[pick] = (int16_t)j;
    return s;
}

// _plateaus_squared_residuals: the plateaus' sums added in frame order
__device__ __forceinline__ double residual_sum(const Table& t)
{
    double r = 0.0;
    for (int i = 0; i >= 0; i = t.nxt[i]) r += t.R[i];
    return r;
}

__global__ void __launch_bounds__(WAVE) kcs_split_scan(const double* __restrict__ lum_all, const int32_t* __restrict__ len,
                                                       long long n_traces, ChiCfg c, int32_t* fit_start, int32_t* fit_stop,
                                                       double* fit_h, int32_t* __restrict__ fit_n, int32_t* __restrict__ n_fits,
                                                       double* __restrict__ o_best, double* __restrict__ o_counter,
                                                       int32_t* __restrict__ o_cn, double* __restrict__ o_S,
                                                       int32_t* __restrict__ status, char* ws)
{
    // LDS, LDS_BYTES_PER_FRAME x Fp: 4 double rows (lum, sq, the two ct), 7 int16 rows (bstart, S / nxt / cs twice), chas
    extern __shared__ double smem[];
    double* s_lum = smem;
    double* s_sq = smem + c.Fp;
    int16_t* s_i16 = (int16_t*)(smem + 4 * c.Fp);
    uint16_t* s_bstart = (uint16_t*)s_i16;
    uint8_t* s_chas = (uint8_t*)(s_i16 + 7 * c.Fp);
    const int lane = threadIdx.x;
    // the block's workspace, WS_BYTES_PER_FRAME x Fp: 5 double rows (H and R twice, top) and one int32 row (split_at)
    double* wd = (double*)(ws + (size_t)blockIdx.x * (size_t)c.Fp * WS_BYTES_PER_FRAME);
    Table bt{s_i16 + c.Fp, s_i16 + 2 * c.Fp, s_i16 + 3 * c.Fp, smem + 2 * c.Fp, wd, wd + c.Fp, 0};
    Table ct{s_i16 + 4 * c.Fp, s_i16 + 5 * c.Fp, s_i16 + 6 * c.Fp, smem + 3 * c.Fp, wd + 2 * c.Fp, wd + 3 * c.Fp, 0};
    int32_t* split_at = (int32_t*)(wd + 5 * (size_t)c.Fp);

    for (long long t = blockIdx.x; t < n_traces; t += gridDim.x) {
        const int n = len[t];
        int num_steps = c.num_steps;
        bool ok = n >= 1 && n <= c.max_frames && n <= FSQ_CHISQ_MAX_FRAMES;
        if (ok) {
            if (num_steps == 0) {
                const double want = __builtin_ceil(c.mult * (double)n);
                num_steps = want < (double)(n - 2) ? (int)want : n - 2;
                ok = num_steps >= 0;
            } else {
                ok = num_steps > 0 && num_steps < n;
            }
        }
        if (!ok) {
            if (lane == 0) status[t] = FSQ_STEPFIT_INVALID;
            continue;
        }
        __syncthreads();
        const double* row = lum_all + t * (long long)c.max_frames;
        double mx = row[0], mn = row[0];
        for (int f = lane; f < n; f += WAVE) {
            const double v = row[f];
            s_lum[f] = v;
            s_bstart[f] = 0;
            mx = v > mx ? v : mx;
            mn = v < mn ? v : mn;
        }
#pragma unroll
        for (int m = 1; m < WAVE; m <<= 1) {
            const double a = __shfl_xor(mx, m, WAVE), b = __shfl_xor(mn, m, WAVE);
            mx = a > mx ? a : mx;
            mn = b < mn ? b : mn;
        }
        __syncthreads();
        Trace T{s_lum, s_sq, s_bstart, s_chas, wd + 4 * (size_t)c.Fp, n, c.L, c.min_mag, (double)n * cs_pow2(mx - mn)};
        for (int u = lane; u < n - 1; u += WAVE) T.top[u] = split_value(T, 0, n - 1, u);

        const int num_plateaus = num_steps + 1;
        const double h_all = np_mean_flat<4>(s_lum, n);
        const double r_all = plateau_residual(T, 0, n - 1, h_all);
        const long long ob = t * (long long)c.fit_cap;
        int nf = 0, arg = -1, st = FSQ_STEPFIT_OK;
        double max_S = 0.0;
        for (int p = 1; p <= num_plateaus; p++) {
            if (p == 1) {
                bt.cnt = 1;
                bt.S[0] = 0; bt.H[0] = h_all; bt.R[0] = r_all; bt.cs[0] = CS_UNKNOWN; bt.nxt[0] = -1;
            } else {
                const int s = best_split<false>(T, bt);
                if (s < 0) break;                                      // the best fit cannot grow (:475-477)
                split_at[p - 2] = s;
                // frames of the new right plateau take its first frame as their plateau's name
                const unsigned old = s_bstart[s];
                __syncthreads();
                for (int f = s + 1 + lane; f < n; f += WAVE)
                    if (s_bstart[f] == old) s_bstart[f] = (uint16_t)(s + 1);
                __syncthreads();
            }
            if (p + 1 > n) { st = FSQ_STEPFIT_UNSUPPORTED; break; }   // the reference's counter-fit raises (:306)
            const double best_res = residual_sum(bt);
            // counter-fit (:481-487): from one plateau, min_step_length 0, until p + 1 plateaus or no split is left
            __syncthreads();
            for (int f = lane; f < n; f += WAVE) s_chas[f] = 0;
            __syncthreads();
            if (lane == 0) s_chas[0] = 1;
            __syncthreads();
            ct.cnt = 1;
            ct.S[0] = 0; ct.H[0] = h_all; ct.R[0] = r_all; ct.cs[0] = CS_UNKNOWN; ct.nxt[0] = -1;
            while (ct.cnt < p + 1) {
                const int s = best_split<true>(T, ct);
                if (s < 0) break;
                __syncthreads();
                if (lane == 0) s_chas[s_bstart[s + 1]] = 1;
                __syncthreads();
            }
            const double counter_res = residual_sum(ct);
            const double S = best_res != 0.0 ? x86_nan(counter_res / best_res) : 1e10;
            if (o_S && nf < c.fit_cap && lane == 0) {
                o_best[ob + nf] = best_res; o_counter[ob + nf] = counter_res; o_cn[ob + nf] = ct.cnt; o_S[ob + nf] = S;
            }
            if (arg < 0 || S > max_S) { arg = nf; max_S = S; }        // the first entry with the largest S
            nf++;
        }
        if (st != FSQ_STEPFIT_OK) {
            if (lane == 0) status[t] = st;
            continue;
        }
        // the chosen fit: the first `chosen` splits, boundaries in frame order, heights np.mean of their frames
        const int chosen = c.ignore_cf ? nf : arg + 1;
        __syncthreads();
        for (int f = lane; f < n; f += WAVE) s_chas[f] = 0;
        __syncthreads();
        if (lane == 0) {
            s_chas[0] = 1;
            for (int k = 2; k <= chosen; k++) s_chas[split_at[k - 2] + 1] = 1;
        }
        __syncthreads();
        const long long fb = t * (long long)c.max_frames;
        int w = 0;
        for (int f = 0; f < n; f++) {
            if (!s_chas[f]) continue;
            fit_start[fb + w] = f;
            if (w > 0) fit_stop[fb + w - 1] = f - 1;
            w++;
        }
        fit_stop[fb + w - 1] = n - 1;
        for (int i = lane; i < w; i += WAVE) {
            const int a = fit_start[fb + i], b = fit_stop[fb + i];
            fit_h[fb + i] = np_mean_flat<4>(s_lum + a, b - a + 1);
        }
        if (lane == 0) { fit_n[t] = w; n_fits[t] = nf; status[t] = FSQ_STEPFIT_OK; }
    }
}

// ---- merge filters and R^2: one lane per trace (plateaus_valid, seq_residual: fsq_plateau_common.h) ---------------
__global__ void __launch_bounds__(WAVE) kcs_merge_filter(const double* __restrict__ lum_all, const int32_t* __restrict__ len,
                                                         long long n_traces, int max_frames, const int32_t* __restrict__ in_start,
                                                         const int32_t* __restrict__ in_stop, const double* __restrict__ in_h,
                                                         const int32_t* __restrict__ in_n, int mode, int has_mag, double min_mag,
                                                         int has_ratio, double min_ratio, int32_t* o_start, int32_t* o_stop,
                                                         double* o_h, int32_t* __restrict__ o_n, int32_t* __restrict__ status)
{
    const long long t = (long long)blockIdx.x * WAVE + threadIdx.x;
    if (t >= n_traces) return;
    const long long ob = t * (long long)max_frames;
    const int n = len[t];
    int cnt = in_n[t];
    if (!plateaus_valid(n, max_frames, cnt, in_start + ob, in_stop + ob)) {
        status[t] = FSQ_STEPFIT_INVALID; o_n[t] = 0;
        return;
    }
    const double* lum = lum_all + ob;
    int32_t* S = o_start + ob;
    double* H = o_h + ob;
    for (int i = 0; i < cnt; i++) { S[i] = in_start[ob + i]; H[i] = in_h[ob + i]; }
    const int end = in_stop[ob + cnt - 1] + 1;
    auto stop_of = [&](int i) { return (i + 1 < cnt ? S[i + 1] : end) - 1; };
    const int passes = cnt - 1;
    for (int pass = 0; pass < passes && cnt >= 2; pass++) {
        bool merged_any = false;
        int w = 0, r = 0;
        while (r < cnt) {                                              // in place: w <= r
            bool merge = false;
            if (r + 1 < cnt) {
                const double ha = H[r], hb = H[r + 1];
                if (mode == FSQ_MERGE_UPSTEPS) {
                    merge = hb > ha;                                   // (:760)
                } else {
                    const double step = __builtin_fabs(ha - hb);
                    if (has_ratio) {                                   // (:856-861) Python's max keeps the first unless the second is greater
                        const double na = sqrt(seq_residual(lum, S[r], stop_of(r), ha));
                        const double nb = sqrt(seq_residual(lum, S[r + 1], stop_of(r + 1), hb));
                        const double mxn = nb > na ? nb : na;
                        merge = step < mxn * min_ratio;
                    }
                    if (has_mag && step < min_mag) merge = true;
                }
            }
            if (merge) {
                const int a = S[r], o = stop_of(r + 1);                // (read before S[w] is written: w <= r)
                S[w] = a; H[w] = np_mean_flat<7>(lum + a, o - a + 1);
                merged_any = true;
                r += 2;
            } else {
                S[w] = S[r]; H[w] = H[r];
                r += 1;
            }
            w++;
        }
        cnt = w;
        if (!merged_any) break;
    }
    for (int i = 0; i < cnt; i++) o_stop[ob + i] = stop_of(i);
    o_n[t] = cnt;
    status[t] = FSQ_STEPFIT_OK;
}

__global__ void __launch_bounds__(WAVE) kcs_r_squared(const double* __restrict__ lum_all, const int32_t* __restrict__ len,
                                                      long long n_traces, int max_frames, const int32_t* __restrict__ in_start,
                                                      const int32_t* __restrict__ in_stop, const double* __restrict__ in_h,
                                                      const int32_t* __restrict__ in_n, double* __restrict__ r2,
                                                      int32_t* __restrict__ status)
{
    const long long t = (long long)blockIdx.x * WAVE + threadIdx.x;
    if (t >= n_traces) return;
    const long long ob = t * (long long)max_frames;
    const int n = len[t], cnt = in_n[t];
    if (!plateaus_valid(n, max_frames, cnt, in_start + ob, in_stop + ob)) {
        status[t] = FSQ_STEPFIT_INVALID;
        return;
    }
    const double* lum = lum_all + ob;
    const int a = in_start[ob], b = in_stop[ob + cnt - 1];
    const double hm = np_mean_flat<7>(lum + a, b - a + 1);
    double ss_res = 0.0;
    for (int i = 0; i < cnt; i++) ss_res += seq_residual(lum, in_start[ob + i], in_stop[ob + i], in_h[ob + i]);
    const double ss_tot = seq_residual(lum, a, b, hm);
    r2[t] = x86_nan(1.0 - ss_res / ss_tot);
    status[t] = FSQ_STEPFIT_OK;
}

bool chisq_cfg(int64_t n_traces, int32_t max_frames, const FsqChisqParams* prm, int32_t fit_cap, ChiCfg* c)
{
    if (n_traces < 0 || max_frames < 1) return false;
    c->max_frames = max_frames;                                        // the row stride; a trace itself is limited to the cap
    c->Fp = ((max_frames < FSQ_CHISQ_MAX_FRAMES ? max_frames : FSQ_CHISQ_MAX_FRAMES) + 7) & ~7;
    if (!prm) return true;                                             // (workspace size only)
    if (prm->num_steps < 0 || !(prm->num_steps_multiplier > 0.0 && prm->num_steps_multiplier <= 1.0)) return false;
    if (prm->min_step_magnitude != prm->min_step_magnitude || fit_cap < 0) return false;
    c->num_steps = prm->num_steps;
    c->L = prm->min_step_length > 0 ? prm->min_step_length : 0;        // (a negative length forbids what 0 forbids)
    c->ignore_cf = prm->ignore_counterfits != 0;
    c->fit_cap = fit_cap;
    c->mult = prm->num_steps_multiplier;
    c->min_mag = prm->min_step_magnitude;
    return true;
}

int64_t chisq_blocks(int64_t n_traces) { return n_traces < MAX_BLOCKS ? n_traces : MAX_BLOCKS; }

bool filter_args_ok(int64_t n_traces, int32_t max_frames) { return n_traces >= 0 && max_frames >= 1 && max_frames <= FSQ_STEPFIT_MAX_MIRRORED; }

}  // namespace

extern "C" int64_t fsq_chisq_workspace_bytes(int64_t n_traces, int32_t max_frames)
{
    ChiCfg c;
    if (!chisq_cfg(n_traces, max_frames, nullptr, 0, &c)) return -1;
    return chisq_blocks(n_traces) * (int64_t)c.Fp * WS_BYTES_PER_FRAME;
}

extern "C" int fsq_chisq_step_fit(const double* d_lum, const int32_t* d_len, int64_t n_traces, int32_t max_frames,
                                  const FsqChisqParams* prm, int32_t* d_fit_start, int32_t* d_fit_stop, double* d_fit_h,
                                  int32_t* d_fit_n, int32_t* d_n_fits, double* d_best_res, double* d_counter_res,
                                  int32_t* d_counter_n, double* d_S, int32_t fit_cap, int32_t* d_status, void* d_ws,
                                  int64_t ws_bytes, void* stream)
{
    ChiCfg c;
    if (!prm || !chisq_cfg(n_traces, max_frames, prm, fit_cap, &c)) return FSQ_EINVAL;
    if (n_traces == 0) return FSQ_OK;
    if (!d_lum || !d_len || !d_fit_start || !d_fit_stop || !d_fit_h || !d_fit_n || !d_n_fits || !d_status || !d_ws) return FSQ_EINVAL;
    const int n_opt = (d_best_res != nullptr) + (d_counter_res != nullptr) + (d_counter_n != nullptr) + (d_S != nullptr);
    if (n_opt != 0 && n_opt != 4) return FSQ_EINVAL;
    const int64_t blocks = chisq_blocks(n_traces);
    if (ws_bytes < blocks * (int64_t)c.Fp * WS_BYTES_PER_FRAME) return FSQ_EINVAL;
    const size_t lds = (size_t)c.Fp * LDS_BYTES_PER_FRAME;
    hipLaunchKernelGGL(kcs_split_scan, dim3((unsigned)blocks), dim3(WAVE), lds, (hipStream_t)stream, d_lum, d_len,
                       (long long)n_traces, c, d_fit_start, d_fit_stop, d_fit_h, d_fit_n, d_n_fits, d_best_res, d_counter_res,
                       d_counter_n, d_S, d_status, (char*)d_ws);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int64_t fsq_stepfit_merge_filter_workspace_bytes(int64_t n_traces, int32_t max_frames)
{
    return filter_args_ok(n_traces, max_frames) ? 0 : -1;              // the filter works in its output rows
}

extern "C" int fsq_stepfit_merge_filter(const double* d_lum, const int32_t* d_len, int64_t n_traces, int32_t max_frames,
                                        const int32_t* d_in_start, const int32_t* d_in_stop, const double* d_in_h,
                                        const int32_t* d_in_n, int32_t mode, int32_t has_min_magnitude, double min_magnitude,
                                        int32_t has_min_noise_ratio, double min_noise_ratio, int32_t* d_out_start,
                                        int32_t* d_out_stop, double* d_out_h, int32_t* d_out_n, int32_t* d_status, void* d_ws,
                                        int64_t ws_bytes, void* stream)
{
    (void)d_ws; (void)ws_bytes;
    if (!filter_args_ok(n_traces, max_frames) || (mode != FSQ_MERGE_UPSTEPS && mode != FSQ_MERGE_SMALL_STEPS)) return FSQ_EINVAL;
    if (mode == FSQ_MERGE_SMALL_STEPS && ((has_min_magnitude && !(min_magnitude >= 0.0)) || (has_min_noise_ratio && !(min_noise_ratio >= 0.0))))
        return FSQ_EINVAL;
    if (n_traces == 0) return FSQ_OK;
    if (!d_lum || !d_len || !d_in_start || !d_in_stop || !d_in_h || !d_in_n || !d_out_start || !d_out_stop || !d_out_h || !d_out_n ||
        !d_status)
        return FSQ_EINVAL;
    hipLaunchKernelGGL(kcs_merge_filter, dim3((unsigned)((n_traces + WAVE - 1) / WAVE)), dim3(WAVE), 0, (hipStream_t)stream, d_lum,
                       d_len, (long long)n_traces, (int)max_frames, d_in_start, d_in_stop, d_in_h, d_in_n, (int)mode,
                       (int)(has_min_magnitude != 0), min_magnitude, (int)(has_min_noise_ratio != 0), min_noise_ratio, d_out_start,
                       d_out_stop, d_out_h, d_out_n, d_status);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int64_t fsq_stepfit_r_squared_workspace_bytes(int64_t n_traces, int32_t max_frames)
{
    return filter_args_ok(n_traces, max_frames) ? 0 : -1;
}

extern "C" int fsq_stepfit_r_squared(const double* d_lum, const int32_t* d_len, int64_t n_traces, int32_t max_frames,
                                     const int32_t* d_in_start, const int32_t* d_in_stop, const double* d_in_h,
                                     const int32_t* d_in_n, double* d_r2, int32_t* d_status, void* d_ws, int64_t ws_bytes,
                                     void* stream)
{
    (void)d_ws; (void)ws_bytes;
    if (!filter_args_ok(n_traces, max_frames)) return FSQ_EINVAL;
    if (n_traces == 0) return FSQ_OK;
    if (!d_lum || !d_len || !d_in_start || !d_in_stop || !d_in_h || !d_in_n || !d_r2 || !d_status) return FSQ_EINVAL;
    hipLaunchKernelGGL(kcs_r_squared, dim3((unsigned)((n_traces + WAVE - 1) / WAVE)), dim3(WAVE), 0, (hipStream_t)stream, d_lum,
                       d_len, (long long)n_traces, (int)max_frames, d_in_start, d_in_stop, d_in_h, d_in_n, d_r2, d_status);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
