// fsq_timetrace.hip - the timetrace experiment table (include/fsq_timetrace.h), gfx950.
//
//   ktt_expand<true>   one wavefront per trace (waves stride over the traces): the per-frame columns of
//                      save_experiment_as_csv (flexlibrary.py:3550-3709) and Trace.coefficient_of_determination (:1476-1514).
//                      Lanes run over the frames: each finds its plateau by bisection of the starts, writes the five
//                      columns and evaluates its two pow terms; the terms are then added in frame order (every lane adds
//                      the same 64 values, read from the lanes' registers), as Python's sum does.
//   ktt_expand<false>  the same expansion without photometries: fsq_plateau_values
//   ktt_spot_rows, ktt_photometry_rows   one lane per (trace, frame): the glue between tracking, photometry and step fit
// The mean is np.mean (numpy's pairwise sum / n), pow is glibc's pow(x, 2.0) (cs_pow2); nothing is re-associated.
#include "../fsq_common.h"
#include "../../../include/fsq_timetrace.h"
#include "fsq_pairwise.h"
#include "fsq_plateau_common.h"

namespace {

constexpr int WAVE = 64;
constexpr int WAVES_PER_BLOCK = 4;
constexpr int MAX_BLOCKS = 8192;

// lane j's value in every lane (j is wave-uniform)
__device__ __forceinline__ double lane_value(double v, int j)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), j), hi = __builtin_amdgcn_readlane(__double2hiint(v), j);
    return __hiloint2double(hi, lo);
}

struct TableOut {
    int32_t* index;
    double* height;
    int32_t* length;
    int32_t* step_num;
    double* step_size;
    double* rss;
    double* tss;
    double* r2;
};

template <bool TABLE>
__global__ void __launch_bounds__(WAVE * WAVES_PER_BLOCK) ktt_expand(const double* __restrict__ phot_all, const int32_t* __restrict__ len,
                                                                     long long n_traces, int max_frames,
                                                                     const int32_t* __restrict__ sf_start,
                                                                     const int32_t* __restrict__ sf_stop,
                                                                     const double* __restrict__ sf_h, const int32_t* __restrict__ sf_n,
                                                                     TableOut o, int32_t* __restrict__ status)
{
    const int lane = threadIdx.x % WAVE;
    const long long wave = (long long)blockIdx.x * WAVES_PER_BLOCK + threadIdx.x / WAVE;
    for (long long t = wave; t < n_traces; t += (long long)gridDim.x * WAVES_PER_BLOCK) {
        const long long ob = t * (long long)max_frames;
        const int32_t* st = sf_start + ob;
        const int32_t* so = sf_stop + ob;
        const double* H = sf_h + ob;
        const int cnt = sf_n[t];
        // (every lane walks the same plateaus: the loads are broadcasts, the result is wave-uniform)
        bool ok = cnt >= 1 && cnt <= max_frames;
        const int n = TABLE ? len[t] : (ok ? so[cnt - 1] + 1 : 0);
        ok = ok && plateaus_valid(n, max_frames, cnt, st, so) && st[0] == 0 && so[cnt - 1] == n - 1;
        if (!ok) {
            if (lane == 0) status[t] = FSQ_STEPFIT_INVALID;
            continue;
        }
        const double* p = phot_all + ob;
        double mean = 0.0, rss = 0.0, tss = 0.0;
        if (TABLE) mean = np_mean_flat<7>(p, n);
        const bool first_is_step = cnt == 1 || so[0] == 0;
        for (int base = 0; base < n; base += WAVE) {
            const int f = base + lane;
            double term_r = 0.0, term_t = 0.0;
            if (f < n) {
                int lo = 0, hi = cnt - 1;                              // the last plateau that starts at or before f
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (st[mid] <= f) lo = mid; else hi = mid - 1;
                }
                const int k = lo;
                const double h = H[k];
                o.height[ob + f] = h;
                if (o.index) o.index[ob + f] = k;
                if (TABLE) {
                    o.length[ob + f] = so[k] - st[k] + 1;
                    const bool some = k >= 1 || first_is_step;
                    o.step_num[ob + f] = k >= 1 ? k - 1 : (some ? 0 : -1);
                    o.step_size[ob + f] = k >= 1 ? H[k - 1] : (some ? h : 0.0);
                    const double v = p[f];
                    term_r = cs_pow2(v - h);
                    term_t = cs_pow2(v - mean);
                }
            }
            if (TABLE) {
                const int m = n - base < WAVE ? n - base : WAVE;
                for (int j = 0; j < m; j++) {
                    rss += lane_value(term_r, j);
                    tss += lane_value(term_t, j);
                }
            }
        }
        if (lane == 0) {
            int s = FSQ_STEPFIT_OK;
            if (TABLE) {
                o.rss[t] = rss;
                o.tss[t] = tss;
                if (tss == 0.0) s = FSQ_TIMETRACE_ZERO_TSS;
                else o.r2[t] = x86_nan(1.0 - rss / tss);
            }
            status[t] = s;
        }
    }
}

__global__ void __launch_bounds__(256) ktt_spot_rows(const int32_t* __restrict__ hw, const uint8_t* __restrict__ present,
                                                     long long total, int n_frames, int32_t* __restrict__ fhw)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long t = i / n_frames;
    const int f = (int)(i - t * n_frames);
    long long src = i;
    if (!present[i]) {
        src = -1;
        for (int g = 0; g < n_frames; g++)
            if (present[t * n_frames + g]) { src = t * n_frames + g; break; }
    }
    fhw[3 * i] = f;
    fhw[3 * i + 1] = src >= 0 ? hw[2 * src] : 0;
    fhw[3 * i + 2] = src >= 0 ? hw[2 * src + 1] : 0;
}

__global__ void __launch_bounds__(256) ktt_photometry_rows(const double* __restrict__ values, const uint8_t* __restrict__ present,
                                                           long long total, int n_frames, double* __restrict__ rows,
                                                           int32_t* __restrict__ len)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    rows[i] = present[i] ? values[i] : 0.0;
    if (i % n_frames == 0) len[i / n_frames] = n_frames;
}

bool rows_ok(int64_t n_traces, int32_t max_frames) { return n_traces >= 0 && max_frames >= 1 && max_frames <= FSQ_STEPFIT_MAX_MIRRORED; }

unsigned expand_blocks(int64_t n_traces)
{
    const int64_t b = (n_traces + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    return (unsigned)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

}  // namespace

extern "C" int fsq_timetrace_table(const double* d_phot, const int32_t* d_len, int64_t n_traces, int32_t max_frames,
                                   const int32_t* d_sf_start, const int32_t* d_sf_stop, const double* d_sf_h,
                                   const int32_t* d_sf_n, int32_t* d_plateau_index, double* d_plateau_height,
                                   int32_t* d_plateau_length, int32_t* d_step_num, double* d_step_size, double* d_rss,
                                   double* d_tss, double* d_r2, int32_t* d_status, void* stream)
{
    if (!rows_ok(n_traces, max_frames)) return FSQ_EINVAL;
    if (n_traces == 0) return FSQ_OK;
    if (!d_phot || !d_len || !d_sf_start || !d_sf_stop || !d_sf_h || !d_sf_n || !d_plateau_index || !d_plateau_height ||
        !d_plateau_length || !d_step_num || !d_step_size || !d_rss || !d_tss || !d_r2 || !d_status)
        return FSQ_EINVAL;
    const TableOut o{d_plateau_index, d_plateau_height, d_plateau_length, d_step_num, d_step_size, d_rss, d_tss, d_r2};
    hipLaunchKernelGGL(ktt_expand<true>, dim3(expand_blocks(n_traces)), dim3(WAVE * WAVES_PER_BLOCK), 0, (hipStream_t)stream, d_phot,
                       d_len, (long long)n_traces, (int)max_frames, d_sf_start, d_sf_stop, d_sf_h, d_sf_n, o, d_status);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_plateau_values(const int32_t* d_start, const int32_t* d_stop, const double* d_h, const int32_t* d_n,
                                  int64_t n_traces, int32_t max_frames, double* d_height, int32_t* d_index, int32_t* d_status,
                                  void* stream)
{
    if (!rows_ok(n_traces, max_frames)) return FSQ_EINVAL;
    if (n_traces == 0) return FSQ_OK;
    if (!d_start || !d_stop || !d_h || !d_n || !d_height || !d_status) return FSQ_EINVAL;
    const TableOut o{d_index, d_height, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL(ktt_expand<false>, dim3(expand_blocks(n_traces)), dim3(WAVE * WAVES_PER_BLOCK), 0, (hipStream_t)stream,
                       (const double*)nullptr, (const int32_t*)nullptr, (long long)n_traces, (int)max_frames, d_start, d_stop, d_h,
                       d_n, o, d_status);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_timetrace_spot_rows(const int32_t* d_hw, const uint8_t* d_present, int64_t n_traces, int32_t n_frames,
                                       int32_t* d_fhw, void* stream)
{
    if (n_traces < 0 || n_frames < 1) return FSQ_EINVAL;
    if (n_traces == 0) return FSQ_OK;
    if (!d_hw || !d_present || !d_fhw) return FSQ_EINVAL;
    const long long total = (long long)n_traces * n_frames;
    hipLaunchKernelGGL(ktt_spot_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_hw, d_present,
                       total, (int)n_frames, d_fhw);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_timetrace_photometry_rows(const double* d_values, const uint8_t* d_present, int64_t n_traces,
                                             int32_t n_frames, double* d_rows, int32_t* d_len, void* stream)
{
    if (n_traces < 0 || n_frames < 1) return FSQ_EINVAL;
    if (n_traces == 0) return FSQ_OK;
    if (!d_values || !d_present || !d_rows || !d_len) return FSQ_EINVAL;
    const long long total = (long long)n_traces * n_frames;
    hipLaunchKernelGGL(ktt_photometry_rows, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_values,
                       d_present, total, (int)n_frames, d_rows, d_len);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
