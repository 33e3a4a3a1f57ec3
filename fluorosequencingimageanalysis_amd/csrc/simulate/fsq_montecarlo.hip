// fsq_montecarlo.hip - the seeded Monte-Carlo PSF fit (C ABI of include/fsq_montecarlo.h).
//
// Reference: pflib._fit_2d_gaussian_monte_carlo (pflib.py:117-177) with _2d_gaussian_function (:93-115), and around it the
// fit_type='monte_carlo' branch of pflib.find_peptides (:441-477).  One wavefront fits one candidate; a block is four of them.
//   - the 25 ROI values sit in LDS, read by every lane at the same address (a broadcast); a lane's 25 model values sit in its
//     own column of an LDS table (consecutive lanes, consecutive doubles) between the pass that finds their maximum and the
//     pass that divides by it;
//   - lane l tries the iterations l, l + 64, ...: six normals from the iteration's own Philox blocks (numpy's polar method,
//     three times), pow(sigmah, 2.0), 25 glibc exps, the maximum, 25 quotients, numpy's 8-accumulator sum of the 25 squared
//     residuals, a square root - and keeps (smallest residual, its iteration), nothing else;
//   - the 64 lane results reduce by the lexicographic minimum of (residual, iteration): the reference's strict `<` keeps the
//     earliest of equal residuals, and a lane only ever holds residuals below the start value, so a NaN is never among them;
//   - the winner's parameters are drawn again from its iteration number (the draws are counter-based), and the lane that owns
//     iteration n_iter - 1 leaves its normalised image in LDS: it is the image the reference returns and measures R^2 on.
#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_montecarlo.h"
#include "../stepfit/fsq_pairwise.h"
#include "fsq_philox.h"

namespace {

constexpr int WAVE = 64;
constexpr int WAVES = 4;                        // candidates per block
constexpr int BLOCK = WAVE * WAVES;
constexpr int MAX_BLOCKS = 1 << 20;
constexpr int REC_WORDS = FSQ_PEAK_RECORD_BYTES / 2;

struct McParams { double H, A, h_0, w_0, sigmah, sigmaw; };

__device__ __forceinline__ double np_clip(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// The six draws of one iteration (pflib.py:151-156); N(loc, scale) is loc + scale * z, product and sum rounded apart.
__device__ __forceinline__ McParams mc_draw(uint32_t it, uint32_t pixel, uint32_t field, uint32_t k0, uint32_t k1, double h0mean,
                                            double w0mean)
{
    McParams p;
    int block = 0;
    double second;
    double z = polar_pair(&block, it, pixel, field, k0, k1, &second);
    p.H = fabs(0.0 + 0.1 * z);
    p.A = fabs(1.0 + 0.2 * second);
    z = polar_pair(&block, it, pixel, field, k0, k1, &second);
    p.h_0 = np_clip(h0mean + 0.3 * z, 0.01, 4.99);
    p.w_0 = np_clip(w0mean + 0.3 * second, 0.01, 4.99);
    z = polar_pair(&block, it, pixel, field, k0, k1, &second);
    p.sigmah = fabs(1.2 + 0.3 * z);
    p.sigmaw = fabs(1.0 + 0.3 * second);
    return p;
}

// One trial (pflib.py:159-163): the model's 25 values go to this lane's column of LDS (gl[i * BLOCK]), *m is their maximum;
// returns sqrt(np.sum((roi - g / m) ** 2)).  The rows are a rolled loop, five exps side by side in each: the 25 values
// never live in registers together (unrolled, the kernel needed 256 VGPRs and scratch).
__device__ __forceinline__ double mc_trial(const McParams& p, const double* roi, double* gl, double* m_out)
{
    const double den = 2.0 * fsq_pow2(p.sigmah);        // a NumPy scalar ** 2: libm's pow
    double b[5];
#pragma unroll
    for (int c = 0; c < 5; c++) {
        const double dw = (double)c - p.w_0;
        b[c] = dw * dw;                                 // an array ** 2: the exact square
    }
    double m = 0.0;
#pragma nounroll
    for (int r = 0; r < 5; r++) {
        const double dh = (double)r - p.h_0, a = dh * dh;
        double g[5];
#pragma unroll
        for (int c = 0; c < 5; c++) g[c] = p.A * fsq_exp(-((a + b[c]) / den)) + p.H;
        if (r == 0) m = g[0];
#pragma unroll
        for (int c = 0; c < 5; c++) {
            m = (g[c] > m || g[c] != g[c]) ? g[c] : m;  // np.max: a NaN stays
            gl[(5 * r + c) * BLOCK] = g[c];
        }
    }
    *m_out = m;
    double r8[8];                                       // np.sum of 25 contiguous doubles: eight accumulators, then the tail
#pragma unroll
    for (int k = 0; k < 8; k++) r8[k] = 0.0;
#pragma nounroll
    for (int j = 0; j < 3; j++)
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const double d = roi[8 * j + k] - gl[(8 * j + k) * BLOCK] / m;
            r8[k] = j == 0 ? d * d : r8[k] + d * d;
        }
    double res = ((r8[0] + r8[1]) + (r8[2] + r8[3])) + ((r8[4] + r8[5]) + (r8[6] + r8[7]));
    const double d24 = roi[24] - gl[24 * BLOCK] / m;
    res += d24 * d24;
    return __builtin_sqrt(res);
}

// pflib.illumina_s_n (pflib.py:261-281) on a float ROI: np.mean / np.std of the 16 edge values (numpy's pairwise leaf)
__device__ __forceinline__ double mc_s_n(const double* s, double vmax)
{
    double op[16];
    int t = 0;
    for (int w = 0; w < 5; w++) op[t++] = s[w];
    for (int w = 0; w < 5; w++) op[t++] = s[20 + w];
    for (int h = 1; h < 4; h++) { op[t++] = s[h * 5]; op[t++] = s[h * 5 + 4]; }
    const double mean = np_mean_short(op, 16);
    double r[8];
    for (int k = 0; k < 8; k++) {
        const double d0 = op[k] - mean, d1 = op[8 + k] - mean;
        r[k] = d0 * d0 + d1 * d1;
    }
    const double res = 0.0 + (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])));
    return (vmax - mean) / __builtin_sqrt(res / 16.0);
}

// grid-stride over groups of WAVES candidates.  FROM_IMAGE: cand / img / first_field are read, else rois / ids.
template <bool FROM_IMAGE>
__global__ void __launch_bounds__(WAVE * WAVES)
kmc_fit(const double* __restrict__ rois, const uint32_t* __restrict__ ids, const uint16_t* __restrict__ img, int n_fields, int H, int W,
        const int32_t* __restrict__ cand, uint32_t first_field, long long n, uint32_t n_iter, uint32_t k0, uint32_t k1,
        FsqRow* __restrict__ rows, double* __restrict__ fit_img, double* __restrict__ rms_out, int32_t* __restrict__ status_out)
{
    __shared__ double s_roi[WAVES][25], s_fit[WAVES][25], s_g[25][BLOCK];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x >> 6;
    double* const roi = s_roi[wave];
    double* const fit = s_fit[wave];
    double* const gl = &s_g[0][threadIdx.x];
    for (long long base = (long long)blockIdx.x * WAVES; base < n; base += (long long)gridDim.x * WAVES) {
        const long long c = base + wave;
        const bool active = c < n;
        uint32_t pixel = 0u, field = 0u;
        int ch = 2, cw = 2, cf = 0;
        if (active) {
            if (FROM_IMAGE) {
                cf = cand[3 * c]; ch = cand[3 * c + 1]; cw = cand[3 * c + 2];
                // (a candidate fsq_detect did not make - no 5x5 neighbourhood inside the stack - is given a NaN ROI: status 2)
                const bool inside = cf >= 0 && cf < n_fields && ch >= 2 && ch <= H - 3 && cw >= 2 && cw <= W - 3;
                pixel = (uint32_t)ch * (uint32_t)W + (uint32_t)cw;
                field = first_field + (uint32_t)cf;
                int v = 0;
                if (inside && lane < 25) v = img[((size_t)cf * H + (ch - 2 + lane / 5)) * W + (cw - 2 + lane % 5)];
                int lo = lane < 25 ? v : 65535, hi = lane < 25 ? v : 0;
#pragma unroll
                for (int d = 1; d < 32; d <<= 1) {      // (the 25 values sit in lanes 0 .. 24: five steps reach lane 0's answer everywhere below 32)
                    lo = min(lo, __shfl_xor(lo, d));
                    hi = max(hi, __shfl_xor(hi, d));
                }
                // pflib.py:446-447: (sub - min) on integers, then / float(max): 0 / 0.0 = NaN for a constant ROI
                if (lane < 25) roi[lane] = inside ? (double)(v - lo) / (double)(hi - lo) : __builtin_nan("");
            } else {
                pixel = ids[2 * c]; field = ids[2 * c + 1];
                if (lane < 25) roi[lane] = rois[25 * c + lane];
            }
            if (lane < 25) fit[lane] = 0.0;
        }
        __syncthreads();
        double vmax = 0.0, start = 0.0, h0mean = 0.0, w0mean = 0.0, best = 0.0;
        int st = FSQ_MC_OK;
        uint32_t best_it = 0u;
        bool have = false;
        if (active) {
            vmax = roi[0];                              // np.max: a NaN stays, and then no pixel equals it (IndexError, :127-128)
#pragma nounroll
            for (int i = 1; i < 25; i++) vmax = (roi[i] > vmax || roi[i] != roi[i]) ? roi[i] : vmax;
            int first = -1;
#pragma nounroll
            for (int i = 24; i >= 0; i--) first = roi[i] == vmax ? i : first;
            if (first < 0) st = FSQ_MC_NO_MAXIMUM;
            else {
                h0mean = (double)(first / 5); w0mean = (double)(first % 5);
                start = 250000000.0 * vmax;             // 10000000 * 25 * np.max(subimage), :147
                best = start;
                for (uint32_t it = (uint32_t)lane; it < n_iter; it += WAVE) {
                    const McParams p = mc_draw(it, pixel, field, k0, k1, h0mean, w0mean);
                    double m;
                    const double rms = mc_trial(p, roi, gl, &m);
                    if (it == n_iter - 1u)
#pragma nounroll
                        for (int i = 0; i < 25; i++) fit[i] = gl[i * BLOCK] / m;
                    if (rms < best) { best = rms; best_it = it; have = true; }
                }
#pragma unroll
                for (int d = 1; d < WAVE; d <<= 1) {
                    const double o_best = __shfl_xor(best, d);
                    const uint32_t o_it = (uint32_t)__shfl_xor((int)best_it, d);
                    const bool o_have = __shfl_xor((int)have, d) != 0;
                    const bool take = o_have && (!have || o_best < best || (o_best == best && o_it < best_it));
                    if (take) { best = o_best; best_it = o_it; have = true; }
                }
            }
        }
        __syncthreads();                                // the last iteration's image is in LDS
        if (active) {
            McParams p = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            double rmse = 0.0, r2 = 0.0, s_n = 0.0, kept = 0.0;
            if (st != FSQ_MC_NO_MAXIMUM) {
                if (have) p = mc_draw(best_it, pixel, field, k0, k1, h0mean, w0mean);
                else st = FSQ_MC_NEVER_IMPROVED;
                kept = best;
                // pflib.py:463-473: Python's sequential sums; np.mean(sub_img) is numpy's pairwise leaf over the 25 values
                const double mean = np_mean_short(roi, 25);
                double num = 0.0, den = 0.0, rm = 0.0;
#pragma nounroll
                for (int i = 0; i < 25; i++) {
                    const double d = roi[i] - fit[i], e = roi[i] - mean;
                    num += d * d;
                    den += e * e;
                    rm += fsq_pow2(d);                  // a NumPy scalar ** 2
                }
                r2 = 1.0 - num / den;
                rmse = __builtin_sqrt(rm / 25.0);
                s_n = mc_s_n(roi, vmax);
            }
            if (lane == 0) {
                FsqRow R;
                R.h0 = p.h_0 + (double)ch - 2.5; R.w0 = p.w_0 + (double)cw - 2.5;
                R.H = p.H; R.A = p.A; R.sigma_h = p.sigmah; R.sigma_w = p.sigmaw; R.theta = 0.0;
                R.rmse = rmse; R.r2 = r2; R.s_n = s_n; R.p2 = p.h_0; R.p3 = p.w_0;
                R.h = ch; R.w = cw; R.field = cf;
                R.status = st; R.niter = have ? (int32_t)best_it : -1; R.nfev = (int32_t)n_iter;
                R.key_h = -1; R.key_w = -1;
                rows[c] = R;
                rms_out[c] = kept;
                status_out[c] = st;
            }
            if (lane < 25) fit_img[25 * c + lane] = fit[lane];
        }
        __syncthreads();                                // (the LDS rows are written again by the next group)
    }
}

// One block per field: the status of its first failing candidate in raster order (the candidates of a field are in that order);
// a failing field keeps nothing, whatever its re-key assertion said.
__global__ void __launch_bounds__(256) kmc_field_status(const int32_t* __restrict__ status, const int32_t* __restrict__ counts,
                                                        const int32_t* __restrict__ offsets, int32_t* __restrict__ nkeep,
                                                        int32_t* __restrict__ field_status)
{
    __shared__ int s_first;
    const int f = blockIdx.x, off = offsets[f], cnt = counts[f];
    if (threadIdx.x == 0) s_first = cnt;
    __syncthreads();
    int mine = cnt;
    for (int i = threadIdx.x; i < cnt; i += blockDim.x)
        if (status[off + i] != FSQ_MC_OK) { mine = i; break; }
    if (mine < cnt) atomicMin(&s_first, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int first = s_first;
        field_status[f] = first < cnt ? status[off + first] : FSQ_MC_OK;
        if (first < cnt) nkeep[f] = 0;
    }
}

__global__ void kmc_total(int32_t* __restrict__ nkeep, int n_fields)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int t = 0;
        for (int f = 0; f < n_fields; f++) t += nkeep[f] > 0 ? nkeep[f] : 0;
        nkeep[n_fields] = t;
    }
}

// One block per field: record r = row (64 words) | the kept candidate's last-iteration image (100 words) | the ROI's 25 pixel words
__global__ void __launch_bounds__(256) kmc_pack_records(const FsqRow* __restrict__ table, const int32_t* __restrict__ out_offsets,
                                                        const int32_t* __restrict__ keep, const int32_t* __restrict__ offsets,
                                                        const double* __restrict__ fit_img, const uint16_t* __restrict__ img, int H, int W,
                                                        long long cap, uint16_t* __restrict__ out)
{
    const int f = blockIdx.x;
    const int r0 = out_offsets[f], nk = out_offsets[f + 1] - r0, off = offsets[f];
    for (int t = threadIdx.x; t < nk * REC_WORDS; t += blockDim.x) {
        const int k = t / REC_WORDS, wd = t - k * REC_WORDS;
        const long long r = (long long)r0 + k;
        if (r >= cap) break;
        uint16_t v;
        if (wd < 64) v = ((const uint16_t*)(table + r))[wd];
        else if (wd < 164) v = ((const uint16_t*)(fit_img + (size_t)keep[off + k] * 25))[wd - 64];
        else {
            const int q = wd - 164, a = q / 5, b = q - 5 * a;
            const FsqRow& R = table[r];
            v = img[((size_t)R.field * H + (R.h - 2 + a)) * W + (R.w - 2 + b)];
        }
        out[(size_t)r * REC_WORDS + wd] = v;
    }
}

size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct McLayout {
    size_t cand, counts, offsets, thr, rows, keep, table, fit, rms, status, stage, total;
};

McLayout mc_layout(int n_fields, int H, int W, int64_t cand_cap, int64_t record_cap)
{
    McLayout L;
    size_t o = 0;
    L.cand = o; o += up256((size_t)cand_cap * 3 * sizeof(int32_t));
    L.counts = o; o += up256(((size_t)n_fields + 1) * sizeof(int32_t));
    L.offsets = o; o += up256(((size_t)n_fields + 1) * sizeof(int32_t));
    L.thr = o; o += up256((size_t)n_fields * sizeof(double));
    L.rows = o; o += up256((size_t)cand_cap * sizeof(FsqRow));
    L.keep = o; o += up256((size_t)cand_cap * sizeof(int32_t));
    L.table = o; o += up256((size_t)record_cap * sizeof(FsqRow));
    L.fit = o; o += up256((size_t)cand_cap * 25 * sizeof(double));
    L.rms = o; o += up256((size_t)cand_cap * sizeof(double));
    L.status = o; o += up256((size_t)cand_cap * sizeof(int32_t));
    const int64_t a = fsq_detect_workspace_bytes(n_fields, H, W), b = fsq_consolidate_workspace_bytes(n_fields, H, W);
    L.stage = o; o += up256((size_t)(a > b ? a : b));
    L.total = o;
    return L;
}

bool n_iter_ok(int64_t n_iter) { return n_iter >= 1 && n_iter <= 2147483647ll; }

unsigned fit_blocks(int64_t n)
{
    const int64_t groups = (n + WAVES - 1) / WAVES;
    return (unsigned)(groups < MAX_BLOCKS ? groups : MAX_BLOCKS);
}

}  // namespace

extern "C" int fsq_mc_fit_rois(const double* d_rois, const uint32_t* d_ids, int64_t n, int64_t n_iter, uint64_t seed, FsqRow* d_rows,
                               double* d_fit_img, double* d_rms, int32_t* d_status, void* stream)
{
    if (n < 0 || !n_iter_ok(n_iter)) return FSQ_EINVAL;
    if (n == 0) return FSQ_OK;
    if (!d_rois || !d_ids || !d_rows || !d_fit_img || !d_rms || !d_status) return FSQ_EINVAL;
    hipLaunchKernelGGL(kmc_fit<false>, dim3(fit_blocks(n)), dim3(WAVE * WAVES), 0, (hipStream_t)stream, d_rois, d_ids,
                       (const uint16_t*)nullptr, 0, 5, 5, (const int32_t*)nullptr, 0u, (long long)n, (uint32_t)n_iter, (uint32_t)seed,
                       (uint32_t)(seed >> 32), d_rows, d_fit_img, d_rms, d_status);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_mc_fit_candidates(const uint16_t* d_img, int n_fields, int H, int W, const int32_t* d_cand, int64_t n,
                                     int64_t n_iter, uint64_t seed, int64_t first_field, FsqRow* d_rows, double* d_fit_img,
                                     double* d_rms, int32_t* d_status, void* stream)
{
    if (n < 0 || !n_iter_ok(n_iter) || n_fields < 1 || H < 5 || W < 5) return FSQ_EINVAL;
    if (first_field < 0 || first_field + (int64_t)n_fields > (1ll << 32) || (int64_t)H * W > (1ll << 32)) return FSQ_EINVAL;
    if (n == 0) return FSQ_OK;
    if (!d_img || !d_cand || !d_rows || !d_fit_img || !d_rms || !d_status) return FSQ_EINVAL;
    hipLaunchKernelGGL(kmc_fit<true>, dim3(fit_blocks(n)), dim3(WAVE * WAVES), 0, (hipStream_t)stream, (const double*)nullptr,
                       (const uint32_t*)nullptr, d_img, n_fields, H, W, d_cand, (uint32_t)first_field, (long long)n, (uint32_t)n_iter,
                       (uint32_t)seed, (uint32_t)(seed >> 32), d_rows, d_fit_img, d_rms, d_status);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int64_t fsq_find_peptides_mc_workspace_bytes(int n_fields, int H, int W, int64_t cand_cap, int64_t record_cap)
{
    if (n_fields < 1 || H < 5 || W < 5 || cand_cap < 1 || record_cap < 1) return FSQ_EINVAL;
    if (fsq_detect_workspace_bytes(n_fields, H, W) < 0) return FSQ_EINVAL;
    return (int64_t)mc_layout(n_fields, H, W, cand_cap, record_cap).total;
}

extern "C" int fsq_find_peptides_mc(const void* d_img, int n_fields, int H, int W, const FsqDetectParams* prm, double r2_threshold,
                                    int radius, int py2_round, int64_t n_iter, uint64_t seed, int64_t first_field, int64_t cand_cap,
                                    void* d_records, int64_t record_cap, int32_t* d_record_offsets, int32_t* d_nkeep,
                                    int32_t* d_field_status, int64_t* n_candidates, int64_t* n_records, void* d_workspace,
                                    int64_t workspace_bytes, void* stream)
{
    if (!d_img || !prm || !d_records || !d_record_offsets || !d_nkeep || !d_field_status || !d_workspace) return FSQ_EINVAL;
    if (n_fields < 1 || H < 5 || W < 5 || cand_cap < 1 || record_cap < 1 || radius < 2 || !n_iter_ok(n_iter)) return FSQ_EINVAL;
    if (first_field < 0 || first_field + (int64_t)n_fields > (1ll << 32) || (int64_t)H * W > (1ll << 32)) return FSQ_EINVAL;
    if (prm->pixel_format != FSQ_PIXELS_U16) return FSQ_ENOTIMPL;
    const int64_t need = fsq_find_peptides_mc_workspace_bytes(n_fields, H, W, cand_cap, record_cap);
    if (need < 0) return FSQ_EINVAL;
    if (workspace_bytes < need) return FSQ_ENOMEM;
    const McLayout L = mc_layout(n_fields, H, W, cand_cap, record_cap);
    unsigned char* ws = (unsigned char*)d_workspace;
    hipStream_t s = (hipStream_t)stream;
    int32_t* cand = (int32_t*)(ws + L.cand);
    int32_t* counts = (int32_t*)(ws + L.counts);
    int32_t* offsets = (int32_t*)(ws + L.offsets);
    FsqRow* rows = (FsqRow*)(ws + L.rows);
    int32_t* keep = (int32_t*)(ws + L.keep);
    FsqRow* table = (FsqRow*)(ws + L.table);
    double* fit = (double*)(ws + L.fit);
    double* rms = (double*)(ws + L.rms);
    int32_t* status = (int32_t*)(ws + L.status);
    if (n_candidates) *n_candidates = 0;
    if (n_records) *n_records = 0;
    int rc = fsq_detect((const uint16_t*)d_img, n_fields, H, W, prm, cand, cand_cap, counts, offsets, (double*)(ws + L.thr),
                        ws + L.stage, (int64_t)(L.total - L.stage), stream);
    if (rc != FSQ_OK) return rc;
    int32_t total = 0;
    FSQ_HIP_CHECK(hipMemcpyAsync(&total, counts + n_fields, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    FSQ_HIP_CHECK(hipStreamSynchronize(s));
    if (total < 0) return FSQ_ENOTIMPL;                 // a response image sums to >= 2^53 (see fsq_detect)
    if (n_candidates) *n_candidates = total;
    if (total > cand_cap) return FSQ_ERANGE;
    rc = fsq_mc_fit_candidates((const uint16_t*)d_img, n_fields, H, W, cand, total, n_iter, seed, first_field, rows, fit, rms, status,
                               stream);
    if (rc != FSQ_OK) return rc;
    rc = fsq_consolidate(rows, counts, offsets, n_fields, H, W, r2_threshold, radius, py2_round, keep, d_nkeep, ws + L.stage,
                         (int64_t)(L.total - L.stage), stream);
    if (rc != FSQ_OK) return rc;
    // the reference raises at the first failing candidate of its loop (:441), before consolidation and the re-key assertion
    hipLaunchKernelGGL(kmc_field_status, dim3(n_fields), dim3(256), 0, s, status, counts, offsets, d_nkeep, d_field_status);
    hipLaunchKernelGGL(kmc_total, dim3(1), dim3(1), 0, s, d_nkeep, n_fields);
    FSQ_HIP_CHECK(hipGetLastError());
    int32_t kept = 0;
    FSQ_HIP_CHECK(hipMemcpyAsync(&kept, d_nkeep + n_fields, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    FSQ_HIP_CHECK(hipStreamSynchronize(s));
    if (kept < 0) kept = 0;
    if (n_records) *n_records = kept;
    if (kept > record_cap) return FSQ_ERANGE;
    rc = fsq_kept_rows(rows, keep, offsets, d_nkeep, n_fields, table, record_cap, d_record_offsets, stream);
    if (rc != FSQ_OK) return rc;
    if (kept > 0) {
        hipLaunchKernelGGL(kmc_pack_records, dim3(n_fields), dim3(256), 0, s, table, d_record_offsets, keep, offsets, fit,
                           (const uint16_t*)d_img, H, W, (long long)record_cap, (uint16_t*)d_records);
        FSQ_HIP_CHECK(hipGetLastError());
    }
    return FSQ_OK;
}
