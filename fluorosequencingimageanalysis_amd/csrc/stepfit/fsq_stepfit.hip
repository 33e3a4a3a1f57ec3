// fsq_stepfit.hip - step fitting of spot photometry traces (include/fsq_stepfit.h), gfx950.
//
// Trace.stepfit_photometries (flexlibrary.py:1380-1462) for a batch of traces:
//   ksf_prepare        one lane per (trace, mirrored frame): clamp (photometry_min) + mirror (stepfitting_library.py:1703-1719)
//   ksf_ck_predictors  one lane per (trace, frame): the CK front / back predictors, np.mean of each window (:1117-1137)
//   ksf_ck_filter      one lane per (trace, frame): CK weights (pow(x, -2) as glibc), normalisation, filtered value (:1138-1274)
//   ksf_welch_steps    one lane per (trace, frame): Welch t-test of every radius (sliding_t_fitter, :996-1005), p from an
//                      fp64 regularised incomplete beta, step mask word per 64 frames (wave ballot)
//   ksf_plateaus_ttest one lane per trace: step grouping, plateaus, refit (:1007-1032, :1322), t_test_filter passes
//                      (:1328-1480: early exit, CPython's list.sort, merge rule), unmirror (:1721-1746)
// Means are numpy's pairwise sum (loops_utils.h.src, PW_BLOCKSIZE 128) divided by n; Welch statistics follow
// scipy.stats.ttest_ind(equal_var=False) (_var -> _moment, _unequal_var_ttest_denom).  Stores are plain vector stores.
#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_stepfit.h"
#include "../libm/fsq_glibc_pow.h"
#include "fsq_pairwise.h"

namespace {

constexpr int BLOCK = 256;

struct Cfg {
    int max_frames, Lmax, mirror, ck, nw, M, n_radii, drop_sort, has_min, W64;
    int wl[FSQ_STEPFIT_MAX_WINDOWS];
    double thr, pmin;
};

__device__ __forceinline__ int mirrored_len(const Cfg& c, int n) { return n + min(c.mirror, n); }
__device__ __forceinline__ bool trace_valid(const Cfg& c, int n)
{
    if (n < 1 || n > c.max_frames) return false;
    const int Lm = mirrored_len(c, n);
    return Lm <= FSQ_STEPFIT_MAX_MIRRORED && !(c.ck && Lm <= 2);
}

// pow(x, -2.0) as glibc (the CK b_diff / f_diff); force-inlined, which is what the compiler made of the plain function before
__device__ __forceinline__ double sf_pow_m2(double x) { return sf_pow<-2, false>(x); }

// ---- two-sided Student t p-value: I_x(df/2, 1/2), x = df / (df + t^2) ---------------------------------------------
// Continued fraction (modified Lentz) of the regularised incomplete beta function; 1 - x is formed as t^2 / (df + t^2).
__device__ double betacf(double a, double b, double x)
{
    const double tiny = 1e-300, eps = 1e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 4000; m++) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < eps) break;
    }
    return h;
}

__device__ double student_p2(double t, double df)
{
    if (__builtin_isnan(t) || __builtin_isnan(df)) return __builtin_nan("");
    const double t2 = t * t;
    if (__builtin_isinf(t2)) return 0.0;
    if (t2 == 0.0) return 1.0;
    const double a = 0.5 * df, b = 0.5;
    const double s = df + t2;
    const double x = df / s, y = t2 / s;                               // y = 1 - x without the subtraction
    const double lx = -log1p(t2 / df), ly = log(y);
    // ln B(a, 1/2) = ln sqrt(pi) - (ln G(a + 1/2) - ln G(a)); for a >= 20 the difference comes from its asymptotic series
    // (relative error < 3e-15 there) instead of two lgamma values of ~a ln a whose rounding would dominate at large df
    double lbeta;
    if (a >= 20.0) {
        const double ia = 1.0 / a, ia2 = ia * ia;
        const double d = 0.5 * log(a) - ia * (0.125 - ia2 * (1.0 / 192.0 - ia2 * (1.0 / 640.0 - ia2 * (17.0 / 14336.0))));
        lbeta = 0.57236494292470008707 - d;
    } else {
        lbeta = lgamma(a) + lgamma(b) - lgamma(a + b);
    }
    const double front = exp(a * lx + b * ly - lbeta);
    if (x < (a + 1.0) / (a + b + 2.0)) return front * betacf(a, b, x) / a;
    return 1.0 - front * betacf(b, a, y) / b;
}

// scipy.stats.ttest_ind(a, b, equal_var=False).pvalue for a = seq[a0, a0 + n1), b = seq[b0, b0 + n2)
template <bool SHORT>
__device__ double welch_p(const double* seq, int a0, int n1, int b0, int n2)
{
    if (n1 <= 0 || n2 <= 0) return __builtin_nan("");
    const double* A = seq + a0;
    const double* B = seq + b0;
    const double m1 = SHORT ? np_mean_short(A, n1) : np_mean(A, n1);
    const double m2 = SHORT ? np_mean_short(B, n2) : np_mean(B, n2);
    auto sq1 = [A, m1](int i) { const double d = A[i] - m1; return d * d; };
    auto sq2 = [B, m2](int i) { const double d = B[i] - m2; return d * d; };
    const double s1 = SHORT ? pw_leaf(sq1, 0, n1) : pw_sum<8>(sq1, 0, n1);
    const double s2 = SHORT ? pw_leaf(sq2, 0, n2) : pw_sum<8>(sq2, 0, n2);
    const double N1 = (double)n1, N2 = (double)n2;
    const double v1 = (s1 / N1) * (N1 / (N1 - 1.0)), v2 = (s2 / N2) * (N2 / (N2 - 1.0));
    const double vn1 = v1 / N1, vn2 = v2 / N2;
    const double sv = vn1 + vn2;
    double df = (sv * sv) / ((vn1 * vn1) / (N1 - 1.0) + (vn2 * vn2) / (N2 - 1.0));
    if (__builtin_isnan(df)) df = 1.0;
    const double t = (m1 - m2) / sqrt(sv);
    return student_p2(t, df);
}

// ---- kernels ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) ksf_prepare(const double* __restrict__ phot, const int32_t* __restrict__ len,
                                                     long long n_traces, Cfg c, double* __restrict__ seqm,
                                                     double* __restrict__ ck_out, int32_t* __restrict__ status)
{
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long t = g / c.Lmax;
    const int f = (int)(g - t * c.Lmax);
    if (t >= n_traces) return;
    const int n = len[t];
    const bool ok = trace_valid(c, n);
    if (f == 0) status[t] = ok ? FSQ_STEPFIT_OK : FSQ_STEPFIT_INVALID;
    if (!ok) return;
    const int m = min(c.mirror, n), Lm = n + m;
    if (f >= Lm) return;
    const int src = f < m ? m - 1 - f : f - m;
    double v = phot[t * c.max_frames + src];
    if (c.has_min) v = (v > c.pmin) ? v : c.pmin;                      // Python max(photometry_min, v)
    seqm[t * c.Lmax + f] = v;
    if (!c.ck && f >= c.mirror) ck_out[t * c.max_frames + (f - c.mirror)] = v;
}

__global__ void __launch_bounds__(BLOCK) ksf_ck_predictors(const int32_t* __restrict__ len, long long n_traces, Cfg c,
                                                           const double* __restrict__ seqm, double* __restrict__ pred)
{
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long t = g / c.Lmax;
    const int L = (int)(g - t * c.Lmax);
    if (t >= n_traces) return;
    const int n = len[t];
    if (!trace_valid(c, n)) return;
    const int Lm = mirrored_len(c, n);
    if (L >= Lm) return;
    const double* s = seqm + t * c.Lmax;
    double* P = pred + t * (2LL * c.nw * c.Lmax);
    for (int k = 0; k < c.nw; k++) {
        const int w = c.wl[k];
        const int r0 = max(L - w - 1, 0);                              // rear window luminosities[max(L - w - 1, 0):L]
        P[(2 * k) * (long long)c.Lmax + L] = L > 0 ? np_mean_short(s + r0, L - r0) : 0.0;
        const int f1 = min(L + w + 1, Lm);                             // front window luminosities[L + 1:L + w + 1]
        P[(2 * k + 1) * (long long)c.Lmax + L] = L < Lm - 1 ? np_mean_short(s + L + 1, f1 - (L + 1)) : 0.0;
    }
}

__global__ void __launch_bounds__(BLOCK) ksf_ck_filter(const int32_t* __restrict__ len, long long n_traces, Cfg c,
                                                       const double* __restrict__ seqm, const double* __restrict__ pred,
                                                       double* __restrict__ ckm, double* __restrict__ ck_out)
{
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long t = g / c.Lmax;
    const int L = (int)(g - t * c.Lmax);
    if (t >= n_traces) return;
    const int n = len[t];
    if (!trace_valid(c, n)) return;
    const int Lm = mirrored_len(c, n);
    if (L >= Lm) return;
    const double* s = seqm + t * c.Lmax;
    const double* P = pred + t * (2LL * c.nw * c.Lmax);
    double fw[FSQ_STEPFIT_MAX_WINDOWS], bw[FSQ_STEPFIT_MAX_WINDOWS];
    // comparison windows (:1163-1197): rear frames max(L - M + 1, 1) .. L, front frames L .. end - 1 with
    // end = min(L + M, Lm), one frame less when L + M >= Lm - 1
    const int r0 = max(L - c.M + 1, 1);
    int fe = min(L + c.M, Lm);
    if (L + c.M >= Lm - 1) fe -= 1;
#pragma unroll
    for (int k = 0; k < FSQ_STEPFIT_MAX_WINDOWS; k++) {
        if (k >= c.nw) break;
        if (L == 0) { fw[k] = 0.0; bw[k] = 1.0; continue; }
        if (L == Lm - 1) { fw[k] = 1.0; bw[k] = 0.0; continue; }
        const double* FP = P + (2 * k) * (long long)c.Lmax;
        const double* BP = P + (2 * k + 1) * (long long)c.Lmax;
        double bd = 0.0, fd = 0.0;                                     // Python sum from int 0, left to right
        for (int j = r0; j <= L; j++) { const double d = s[j] - FP[j]; bd = bd + d * d; }
        for (int j = L; j < fe; j++) { const double d = s[j] - BP[j]; fd = fd + d * d; }
        if (bd != 0.0 && fd != 0.0) { fw[k] = sf_pow_m2(bd); bw[k] = sf_pow_m2(fd); }
        else if (bd == 0.0 && fd != 0.0) { fw[k] = 1.0; bw[k] = 0.0; }
        else if (bd != 0.0 && fd == 0.0) { fw[k] = 0.0; bw[k] = 1.0; }
        else { fw[k] = 1.0; bw[k] = 0.0; }
    }
    // total weight: front weights summed in window order, then back weights (dict order 2, 4, 8, 16 under Python 3)
    double ft = 0.0, bt = 0.0;
    for (int k = 0; k < c.nw; k++) ft += fw[k];
    for (int k = 0; k < c.nw; k++) bt += bw[k];
    const double tot = ft + bt;
    double out = 0.0;
    for (int k = 0; k < c.nw; k++) {
        const double fpv = P[(2 * k) * (long long)c.Lmax + L], bpv = P[(2 * k + 1) * (long long)c.Lmax + L];
        if (L == 0) out += (bw[k] / tot) * bpv;
        else if (L == Lm - 1) out += (fw[k] / tot) * fpv;
        else out += (fw[k] / tot) * fpv + (bw[k] / tot) * bpv;
    }
    ckm[t * c.Lmax + L] = out;
    if (L >= c.mirror) ck_out[t * c.max_frames + (L - c.mirror)] = out;
}

// one lane per (trace, frame), frames padded to W64 * 64 so that a wave covers one mask word of one trace
__global__ void __launch_bounds__(BLOCK) ksf_welch_steps(const int32_t* __restrict__ len, long long n_traces, Cfg c,
                                                         const double* __restrict__ seq_all, unsigned long long* __restrict__ words,
                                                         double* __restrict__ p_out)
{
    const long long g = (long long)blockIdx.x * BLOCK + threadIdx.x;
    const long long per = 64LL * c.W64;
    const long long t = g / per;
    const int f = (int)(g - t * per);
    if (t >= n_traces) return;                                         // whole waves leave together (per is a multiple of 64)
    const int n = len[t];
    const bool ok = trace_valid(c, n);
    const int Lm = ok ? mirrored_len(c, n) : 0;
    bool step = false;
    if (f < Lm) {
        const double* s = seq_all + t * c.Lmax;
        step = c.n_radii > 0;
        for (int k = 0; k < c.n_radii; k++) {
            const int r = 5 + k;
            int a0 = f - r;                                            // Python slice [f - r:f]
            if (a0 < 0) a0 += Lm;
            if (a0 < 0) a0 = 0;
            const int n1 = max(f - a0, 0);
            const int n2 = min(f + r, Lm) - f;                         // [f:f + r]
            const double p = welch_p<true>(s, a0, n1, f, n2);
            step = step && (p < c.thr);
            if (p_out) p_out[(t * c.n_radii + k) * c.Lmax + f] = p;
        }
    }
    const unsigned long long m = __ballot(step);
    if ((threadIdx.x & 63) == 0) words[t * c.W64 + (f >> 6)] = m;
}

// CPython list.sort(key=p, reverse=True) (listobject.c, 3.x) of idx[0..n) for n < 64 (one run, no merges): reverse,
// count_run, binary insertion sort with `<`, reverse.
__device__ void cpython_sort_desc(const double* key, int32_t* idx, int n)
{
    for (int i = 0; i < n; i++) idx[i] = n - 1 - i;
    if (n < 2) return;
    int run = 2;
    if (key[idx[1]] < key[idx[0]]) {
        while (run < n && key[idx[run]] < key[idx[run - 1]]) run++;
        for (int i = 0, j = run - 1; i < j; i++, j--) { const int32_t tmp = idx[i]; idx[i] = idx[j]; idx[j] = tmp; }
    } else {
        while (run < n && !(key[idx[run]] < key[idx[run - 1]])) run++;
    }
    for (int st = run; st < n; st++) {
        const int32_t pv = idx[st];
        const double pk = key[pv];
        int l = 0, r = st;
        do {
            const int p = l + ((r - l) >> 1);
            if (pk < key[idx[p]]) r = p; else l = p + 1;
        } while (l < r);
        for (int j = st; j > l; j--) idx[j] = idx[j - 1];
        idx[l] = pv;
    }
    for (int i = 0, j = n - 1; i < j; i++, j--) { const int32_t tmp = idx[i]; idx[i] = idx[j]; idx[j] = tmp; }
}

// Stable descending sort of idx[0..n) by key without NaN keys (what CPython's sort gives at any length then):
// bottom-up merge sort, O(n log n), tmp holds n entries.
__device__ void stable_sort_desc(const double* key, int32_t* idx, int32_t* tmp, int n)
{
    for (int i = 0; i < n; i++) idx[i] = i;
    int32_t* src = idx;
    int32_t* dst = tmp;
    for (int w = 1; w < n; w *= 2) {
        for (int lo = 0; lo < n; lo += 2 * w) {
            const int mid = min(lo + w, n), hi = min(lo + 2 * w, n);
            int a = lo, b = mid, o = lo;
            while (a < mid && b < hi) dst[o++] = (key[src[b]] > key[src[a]]) ? src[b++] : src[a++];
            while (a < mid) dst[o++] = src[a++];
            while (b < hi) dst[o++] = src[b++];
        }
        int32_t* x = src; src = dst; dst = x;
    }
    if (src != idx)
        for (int i = 0; i < n; i++) idx[i] = src[i];
}

__device__ void write_unmirrored(const int32_t* st, const double* h, int cnt, int end, int mirror, int32_t* o_start,
                                 int32_t* o_stop, double* o_h, int32_t* o_n)
{
    int w = 0;
    for (int i = 0; i < cnt; i++) {
        int a = st[i] - mirror;
        const int o = (i + 1 < cnt ? st[i + 1] : end) - 1 - mirror;
        if (o < 0) continue;                                           // wholly inside the mirror
        if (a < 0) a = 0;                                              // straddles it: clamped, height kept
        o_start[w] = a; o_stop[w] = o; o_h[w] = h[i];
        w++;
    }
    *o_n = w;
}

struct TfWork {
    double* p;          // pair p of the current pass
    int32_t* idx;       // sorted pair order
    int32_t* tmp;       // merge sort buffer
    int8_t* flag;       // bit 0: marked for merging, bit 1: visited in sorted order
    double* rec;        // optional: every pair test's p in order (at most rec_cap)
    int rec_cap;
};

// t_test_filter (stepfitting_library.py:1328-1480) on plateaus (S[i], H[i]), i < cnt, that cover [S[0], end) contiguously
// (stop_i = S[i + 1] - 1, the last stop end - 1).  len(plateaus) - 1 passes; a pass that merges nothing returns its input,
// so the loop stops there.  Returns the FSQ_STEPFIT_* status; *n_tests counts the pair tests run.
__device__ int ttest_filter(const double* s, int32_t* S, double* H, int* cnt_io, int end, int nms, bool drop_sort, double thr,
                            const TfWork& wk, int* n_tests)
{
    int cnt = *cnt_io;
    int nt = 0;
    auto stop_of = [&](int i) { return (i + 1 < cnt ? S[i + 1] : end) - 1; };
    auto pair_p = [&](int r) {
        const double p = welch_p<false>(s, S[r], S[r + 1] - S[r], S[r + 1], stop_of(r + 1) - S[r + 1] + 1);
        if (wk.rec && nt < wk.rec_cap) wk.rec[nt] = p;
        nt++;
        return p;
    };
    int st = FSQ_STEPFIT_OK;
    const int passes = cnt - 1;
    for (int pass = 0; pass < passes && cnt >= 2; pass++) {
        bool merged_any = false;
        int w = 0;
        if (drop_sort) {
            const int np = cnt - 1;
            bool any_nan = false;
            for (int r = 0; r < np; r++) {
                const double p = pair_p(r);
                wk.p[r] = p;
                any_nan |= __builtin_isnan(p);
                wk.flag[r] = (p >= thr && stop_of(r) >= nms) ? 1 : 0;
            }
            if (any_nan && np >= 64) { st = FSQ_STEPFIT_UNSUPPORTED; break; }
            if (np < 64) cpython_sort_desc(wk.p, wk.idx, np);
            else stable_sort_desc(wk.p, wk.idx, wk.tmp, np);
            // a marked pair clears the marks of the adjacent pairs sorted after it
            for (int i = 0; i < np; i++) {
                const int r = wk.idx[i];
                wk.flag[r] |= 2;
                if (wk.flag[r] & 1) {
                    if (r > 0 && !(wk.flag[r - 1] & 2)) wk.flag[r - 1] = 0;
                    if (r + 1 < np && !(wk.flag[r + 1] & 2)) wk.flag[r + 1] = 0;
                }
            }
            int r = 0;
            while (r < cnt) {                                          // in place: w <= r
                if (r < np && (wk.flag[r] & 1)) {
                    const int a = S[r], o = stop_of(r + 1);
                    S[w] = a; H[w] = np_mean(s + a, o - a + 1);
                    merged_any = true;
                    r += 2;
                } else {
                    S[w] = S[r]; H[w] = H[r];
                    r += 1;
                }
                w++;
            }
        } else {
            int r = 0;
            while (r < cnt) {
                bool merge = false;
                if (r + 1 < cnt && stop_of(r) >= nms) merge = pair_p(r) >= thr;
                if (merge) {
                    const int a = S[r], o = stop_of(r + 1);           // (read before S[w] is written: w <= r)
                    S[w] = a; H[w] = np_mean(s + a, o - a + 1);
                    merged_any = true;
                    r += 2;
                } else {
                    S[w] = S[r]; H[w] = H[r];
                    r += 1;
                }
                w++;
            }
        }
        cnt = w;
        if (!merged_any) break;
    }
    *cnt_io = cnt;
    *n_tests = nt;
    return st;
}

// one lane per trace.  Plateaus are kept as (start, height): they partition [0, Lm), stop_i = start_{i+1} - 1.
__global__ void __launch_bounds__(64) ksf_plateaus_ttest(const int32_t* __restrict__ len, long long n_traces, Cfg c,
                                                         const double* __restrict__ seqm, const unsigned long long* __restrict__ words,
                                                         int32_t* __restrict__ w_start, double* __restrict__ w_h,
                                                         double* __restrict__ w_p, int32_t* __restrict__ w_idx, int32_t* __restrict__ w_tmp,
                                                         int8_t* __restrict__ w_flag,
                                                         int32_t* __restrict__ pl_start, int32_t* __restrict__ pl_stop,
                                                         double* __restrict__ pl_h, int32_t* __restrict__ pl_n,
                                                         int32_t* __restrict__ tf_start, int32_t* __restrict__ tf_stop,
                                                         double* __restrict__ tf_h, int32_t* __restrict__ tf_n,
                                                         int32_t* __restrict__ status, double* __restrict__ pair_p,
                                                         int32_t* __restrict__ pair_n, int pair_cap)
{
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    if (t >= n_traces) return;
    const int n = len[t];
    if (!trace_valid(c, n)) {
        pl_n[t] = 0; tf_n[t] = 0;
        if (pair_n) pair_n[t] = 0;
        return;
    }
    const int Lm = mirrored_len(c, n);
    const double* s = seqm + t * c.Lmax;
    const unsigned long long* wd = words + t * c.W64;
    int32_t* S = w_start + t * c.Lmax;
    double* H = w_h + t * c.Lmax;
    auto is_step = [wd](int f) { return (wd[f >> 6] >> (f & 63)) & 1ull; };
    // steps grouped by consecutive frames, each group keeping its last frame (:1019-1037); frame 0 is never a step
    int cnt = 1;
    S[0] = 0;
    for (int f = 1; f < Lm; f++)
        if (is_step(f) && !(f + 1 < Lm && is_step(f + 1))) S[cnt++] = f;
    for (int i = 0; i < cnt; i++) {                                    // refit on the unfiltered sequence
        const int stop = (i + 1 < cnt ? S[i + 1] : Lm) - 1;
        H[i] = np_mean(s + S[i], stop - S[i] + 1);
    }
    const long long ob = t * (long long)c.max_frames;
    write_unmirrored(S, H, cnt, Lm, c.mirror, pl_start + ob, pl_stop + ob, pl_h + ob, pl_n + t);
    TfWork wk{w_p + t * c.Lmax, w_idx + t * c.Lmax, w_tmp + t * c.Lmax, w_flag + t * c.Lmax,
              pair_p ? pair_p + t * (long long)pair_cap : nullptr, pair_cap};
    int nt = 0;
    const int st = ttest_filter(s, S, H, &cnt, Lm, c.mirror, c.drop_sort, c.thr, wk, &nt);
    status[t] = st;
    if (pair_n) pair_n[t] = nt;
    if (st != FSQ_STEPFIT_OK) { tf_n[t] = 0; return; }
    write_unmirrored(S, H, cnt, Lm, c.mirror, tf_start + ob, tf_stop + ob, tf_h + ob, tf_n + t);
}

// stand-alone t_test_filter on caller-given contiguous plateaus: one lane per trace
__global__ void __launch_bounds__(64) ksf_ttest_filter(const double* __restrict__ lum, const int32_t* __restrict__ len,
                                                       long long n_traces, int max_frames, const int32_t* __restrict__ in_start,
                                                       const int32_t* __restrict__ in_stop, const double* __restrict__ in_h,
                                                       const int32_t* __restrict__ in_n, double thr, int drop_sort, int nms,
                                                       int32_t* __restrict__ w_start, double* __restrict__ w_h,
                                                       double* __restrict__ w_p, int32_t* __restrict__ w_idx, int32_t* __restrict__ w_tmp,
                                                       int8_t* __restrict__ w_flag, int32_t* __restrict__ tf_start,
                                                       int32_t* __restrict__ tf_stop, double* __restrict__ tf_h,
                                                       int32_t* __restrict__ tf_n, int32_t* __restrict__ status,
                                                       double* __restrict__ pair_p, int32_t* __restrict__ pair_n, int pair_cap)
{
    const long long t = (long long)blockIdx.x * 64 + threadIdx.x;
    if (t >= n_traces) return;
    const long long ob = t * (long long)max_frames;
    const int n = len[t];
    int cnt = in_n[t];
    // valid: 1 <= cnt <= n <= max_frames, 0 <= start_0, stop_i + 1 == start_{i+1}, start_i <= stop_i, stop_last < n
    bool ok = n >= 1 && n <= max_frames && n <= FSQ_STEPFIT_MAX_MIRRORED && cnt >= 1 && cnt <= n && in_start[ob] >= 0;
    for (int i = 0; ok && i < cnt; i++) {
        ok = in_start[ob + i] <= in_stop[ob + i] && in_stop[ob + i] < n;
        if (ok && i + 1 < cnt) ok = in_stop[ob + i] + 1 == in_start[ob + i + 1];
    }
    if (!ok) {
        status[t] = FSQ_STEPFIT_INVALID; tf_n[t] = 0;
        if (pair_n) pair_n[t] = 0;
        return;
    }
    int32_t* S = w_start + ob;
    double* H = w_h + ob;
    for (int i = 0; i < cnt; i++) { S[i] = in_start[ob + i]; H[i] = in_h[ob + i]; }
    const int end = in_stop[ob + cnt - 1] + 1;
    TfWork wk{w_p + ob, w_idx + ob, w_tmp + ob, w_flag + ob, pair_p ? pair_p + t * (long long)pair_cap : nullptr, pair_cap};
    int nt = 0;
    const int st = ttest_filter(lum + ob, S, H, &cnt, end, nms, drop_sort != 0, thr, wk, &nt);
    status[t] = st;
    if (pair_n) pair_n[t] = nt;
    if (st != FSQ_STEPFIT_OK) { tf_n[t] = 0; return; }
    write_unmirrored(S, H, cnt, end, 0, tf_start + ob, tf_stop + ob, tf_h + ob, tf_n + t);
}

struct Layout {
    size_t seqm, ckm, pred, words, wstart, wh, wp, widx, wtmp, wflag, total;
};

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

bool make_cfg(int64_t n_traces, int32_t max_frames, const FsqStepfitParams* prm, Cfg* c)
{
    if (!prm || n_traces < 0 || max_frames < 1 || max_frames > FSQ_STEPFIT_MAX_MIRRORED) return false;
    if (prm->mirror_start < 0 || prm->chung_kennedy < 0 || prm->window_radius < 0 || prm->window_radius > 64) return false;
    if (prm->chung_kennedy > 0) {
        if (prm->p != 2 || prm->M < 1 || prm->M > 64 || prm->n_windows < 1 || prm->n_windows > FSQ_STEPFIT_MAX_WINDOWS) return false;
        for (int k = 0; k < prm->n_windows; k++)
            if (prm->window_lengths[k] < 1 || prm->window_lengths[k] > 64) return false;
    }
    c->max_frames = max_frames;
    c->mirror = prm->mirror_start;
    c->Lmax = max_frames + (prm->mirror_start < max_frames ? prm->mirror_start : max_frames);
    c->ck = prm->chung_kennedy > 0;
    c->nw = c->ck ? prm->n_windows : 0;
    for (int k = 0; k < FSQ_STEPFIT_MAX_WINDOWS; k++) c->wl[k] = k < c->nw ? prm->window_lengths[k] : 0;
    c->M = prm->M;
    c->n_radii = prm->window_radius > 5 ? prm->window_radius - 5 : 0;
    c->drop_sort = prm->drop_sort != 0;
    c->has_min = prm->has_photometry_min != 0;
    c->thr = prm->p_threshold;
    c->pmin = prm->photometry_min;
    c->W64 = (c->Lmax + 63) / 64;
    return true;
}

// the full path uses every region; the stand-alone t-filter only the plateau work tables (rows of max_frames, ck off)
Layout layout(int64_t n, const Cfg& c, bool tfilter_only = false)
{
    Layout l;
    size_t o = 0;
    const size_t rows = (size_t)n * c.Lmax;
    l.seqm = o; o = align256(o + (tfilter_only ? 0 : rows * 8));
    l.ckm = o; o = align256(o + (c.ck ? rows * 8 : 0));
    l.pred = o; o = align256(o + (c.ck ? rows * 16 * c.nw : 0));
    l.words = o; o = align256(o + (tfilter_only ? 0 : (size_t)n * c.W64 * 8));
    l.wstart = o; o = align256(o + rows * 4);
    l.wh = o; o = align256(o + rows * 8);
    l.wp = o; o = align256(o + rows * 8);
    l.widx = o; o = align256(o + rows * 4);
    l.wtmp = o; o = align256(o + rows * 4);
    l.wflag = o; o = align256(o + rows);
    l.total = o;
    return l;
}

bool make_tfilter_cfg(int64_t n_traces, int32_t max_frames, Cfg* c)
{
    FsqStepfitParams p{};
    p.p = 2;
    return make_cfg(n_traces, max_frames, &p, c);                     // mirror 0, no CK: Lmax = max_frames
}

}  // namespace

extern "C" int64_t fsq_stepfit_workspace_bytes(int64_t n_traces, int32_t max_frames, const FsqStepfitParams* prm)
{
    Cfg c;
    if (!make_cfg(n_traces, max_frames, prm, &c)) return -1;
    return (int64_t)layout(n_traces, c).total;
}

extern "C" int fsq_stepfit_traces(const double* d_phot, const int32_t* d_len, int64_t n_traces, int32_t max_frames,
                                  const FsqStepfitParams* prm, double* d_ck, int32_t* d_pl_start, int32_t* d_pl_stop, double* d_pl_h,
                                  int32_t* d_pl_n, int32_t* d_tf_start, int32_t* d_tf_stop, double* d_tf_h, int32_t* d_tf_n,
                                  int32_t* d_status, double* d_p, double* d_pair_p, int32_t* d_pair_n, int32_t pair_cap,
                                  void* d_ws, int64_t ws_bytes, void* stream)
{
    Cfg c;
    if (!make_cfg(n_traces, max_frames, prm, &c)) return FSQ_EINVAL;
    if (n_traces == 0) return FSQ_OK;
    if (!d_phot || !d_len || !d_ck || !d_pl_start || !d_pl_stop || !d_pl_h || !d_pl_n || !d_tf_start || !d_tf_stop || !d_tf_h ||
        !d_tf_n || !d_status || !d_ws)
        return FSQ_EINVAL;
    if ((d_pair_p != nullptr) != (d_pair_n != nullptr) || (d_pair_p && pair_cap < 0)) return FSQ_EINVAL;
    const Layout l = layout(n_traces, c);
    if (ws_bytes < (int64_t)l.total) return FSQ_EINVAL;
    char* ws = (char*)d_ws;
    double* seqm = (double*)(ws + l.seqm);
    double* ckm = (double*)(ws + l.ckm);
    double* pred = (double*)(ws + l.pred);
    unsigned long long* words = (unsigned long long*)(ws + l.words);
    hipStream_t s = (hipStream_t)stream;
    const long long lanes = n_traces * (long long)c.Lmax;
    const unsigned grid = (unsigned)((lanes + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(ksf_prepare, dim3(grid), dim3(BLOCK), 0, s, d_phot, d_len, (long long)n_traces, c, seqm, d_ck, d_status);
    FSQ_HIP_CHECK(hipGetLastError());
    if (c.ck) {
        hipLaunchKernelGGL(ksf_ck_predictors, dim3(grid), dim3(BLOCK), 0, s, d_len, (long long)n_traces, c, seqm, pred);
        FSQ_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(ksf_ck_filter, dim3(grid), dim3(BLOCK), 0, s, d_len, (long long)n_traces, c, seqm, pred, ckm, d_ck);
        FSQ_HIP_CHECK(hipGetLastError());
    }
    const long long wl = n_traces * 64LL * c.W64;
    hipLaunchKernelGGL(ksf_welch_steps, dim3((unsigned)((wl + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, d_len, (long long)n_traces, c,
                       c.ck ? ckm : seqm, words, d_p);
    FSQ_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(ksf_plateaus_ttest, dim3((unsigned)((n_traces + 63) / 64)), dim3(64), 0, s, d_len, (long long)n_traces, c,
                       seqm, words, (int32_t*)(ws + l.wstart), (double*)(ws + l.wh), (double*)(ws + l.wp), (int32_t*)(ws + l.widx),
                       (int32_t*)(ws + l.wtmp), (int8_t*)(ws + l.wflag), d_pl_start, d_pl_stop, d_pl_h, d_pl_n, d_tf_start,
                       d_tf_stop, d_tf_h, d_tf_n, d_status, d_pair_p, d_pair_n, (int)pair_cap);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int64_t fsq_stepfit_ttest_filter_workspace_bytes(int64_t n_traces, int32_t max_frames)
{
    Cfg c;
    if (!make_tfilter_cfg(n_traces, max_frames, &c)) return -1;
    return (int64_t)layout(n_traces, c, true).total;
}

extern "C" int fsq_stepfit_ttest_filter(const double* d_lum, const int32_t* d_len, int64_t n_traces, int32_t max_frames,
                                        const int32_t* d_in_start, const int32_t* d_in_stop, const double* d_in_h,
                                        const int32_t* d_in_n, double p_threshold, int32_t drop_sort, int32_t no_merge_start,
                                        int32_t* d_tf_start, int32_t* d_tf_stop, double* d_tf_h, int32_t* d_tf_n,
                                        int32_t* d_status, double* d_pair_p, int32_t* d_pair_n, int32_t pair_cap, void* d_ws,
                                        int64_t ws_bytes, void* stream)
{
    Cfg c;
    if (!make_tfilter_cfg(n_traces, max_frames, &c)) return FSQ_EINVAL;
    if (n_traces == 0) return FSQ_OK;
    if (!d_lum || !d_len || !d_in_start || !d_in_stop || !d_in_h || !d_in_n || !d_tf_start || !d_tf_stop || !d_tf_h || !d_tf_n ||
        !d_status || !d_ws)
        return FSQ_EINVAL;
    if ((d_pair_p != nullptr) != (d_pair_n != nullptr) || (d_pair_p && pair_cap < 0)) return FSQ_EINVAL;
    const Layout l = layout(n_traces, c, true);
    if (ws_bytes < (int64_t)l.total) return FSQ_EINVAL;
    char* ws = (char*)d_ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(ksf_ttest_filter, dim3((unsigned)((n_traces + 63) / 64)), dim3(64), 0, s, d_lum, d_len, (long long)n_traces,
                       (int)max_frames, d_in_start, d_in_stop, d_in_h, d_in_n, p_threshold, (int)drop_sort, (int)no_merge_start,
                       (int32_t*)(ws + l.wstart), (double*)(ws + l.wh), (double*)(ws + l.wp), (int32_t*)(ws + l.widx),
                       (int32_t*)(ws + l.wtmp), (int8_t*)(ws + l.wflag), d_tf_start, d_tf_stop, d_tf_h, d_tf_n, d_status,
                       d_pair_p, d_pair_n, (int)pair_cap);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
