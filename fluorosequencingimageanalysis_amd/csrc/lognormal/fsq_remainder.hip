// fsq_remainder.hip - the remainder correction of track photometries (include/fsq_remainder.h): MCsimlib._remainder_adjust_2
// (:3434-3472) and _remainder_adjust (:3398-3431), with numpy's bits.  Four kernels on one stream:
//
// krm_tracks, one wavefront per track (:3441-3446, :3402-3408): finds the track's segment (a binary search of seg_off) and
//   notes it for krm_apply.  A remainder (all F category bits set) takes a slot of its segment from an atomic counter, which
//   is n_remainders itself, and lane f writes the track's value at frame f to the workspace, segment by segment and frame by
//   frame: ws[F * seg_off[s] + f * cap + slot], cap the segment's tracks.  In RATIO mode the value is (I_f - m) / m with m the
//   track's median: every lane ranks its intensity against the others' (ties by lane) with F wave shuffles, so nothing is
//   indexed at run time and nothing goes to scratch.
// krm_medians, one 256-thread block per (segment, frame) (:3454, :3414): the exact median of the R values, on their
//   order-preserving 64-bit keys: select_median of fsq_select_median.h, in LDS up to FSQ_REMAINDER_LDS_MAX values and a
//   nine-pass radix select over the workspace above.  A NaN among the values gives NaN; R = 0 gives NaN.
// krm_finish, one thread per segment: kept (:3450, :3412) and, in ADDITIVE mode, median_f - median_0 (:3416).
// krm_apply, one thread per value (:3468, :3427): 8 bytes read, 8 written.
//
// Bounds: a segment is used only where 0 <= seg_off[s] <= seg_off[s + 1] <= n; a slot only below the segment's capacity.  With
// that every workspace index is below n * F, whatever seg_off holds.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../fsq_common.h"
#include "../../../include/fsq_remainder.h"
#include "fsq_select_median.h"

namespace {

constexpr int THREADS = SELECT_THREADS;
constexpr int WAVE = SELECT_WAVE;
constexpr int TRACKS_PER_BLOCK = THREADS / WAVE;
static_assert(FSQ_REMAINDER_MAX_FRAMES <= WAVE, "one lane per frame");

__global__ void __launch_bounds__(THREADS)
krm_tracks(const double* __restrict__ intensity, const u64* __restrict__ category, const long long* __restrict__ seg_off,
           long long n, int F, long long S, int mode, int* __restrict__ n_remainders, double* __restrict__ ws_values,
           int* __restrict__ ws_segment)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long i = (long long)blockIdx.x * TRACKS_PER_BLOCK + (threadIdx.x / WAVE);
    if (i >= n) return;                                            // (uniform over the wavefront; the kernel has no barrier)
    long long off = 0, cap = 0;
    const long long s = segment_of(seg_off, S, n, i, &off, &cap);
    if (lane == 0) ws_segment[i] = (int)s;
    const u64 all_on = F == 64 ? ~0ull : ((1ull << F) - 1ull);
    if (s < 0 || (category[i] & all_on) != all_on) return;
    const bool live = lane < F;
    const double x = live ? intensity[i * F + lane] : 0.0;
    double v = x;
    if (mode == FSQ_REMAINDER_RATIO) {
        int rank = 0;                                              // #{g : I_g < I_f, or equal and g < f}
        for (int g = 0; g < F; g++) {
            const double xg = __shfl(x, g, WAVE);
            rank += (xg < x || (xg == x && g < lane)) ? 1 : 0;
        }
        const u64 lo = __ballot(live && rank == (F - 1) / 2), hi = __ballot(live && rank == F / 2);
        // a NaN lane ranks 0 and no other lane counts it, so the finite lanes still fill both middle ranks: np.median gives NaN
        const u64 any_nan = __ballot(live && x != x);
        double m = __builtin_nan("");
        if (lo && hi && !any_nan) m = middle_mean(__shfl(x, __ffsll((long long)lo) - 1, WAVE), __shfl(x, __ffsll((long long)hi) - 1, WAVE), F & 1);
        v = (x - m) / m;
    }
    int slot = 0;
    if (lane == 0) slot = atomicAdd(&n_remainders[s], 1);
    slot = __shfl(slot, 0, WAVE);
    if (live && slot < cap) ws_values[(long long)F * off + lane * cap + slot] = v;
}

// R of segment s and where its tracks start and how many they are; R = 0 for a segment that is not well formed
__device__ __forceinline__ int remainders_of(const long long* __restrict__ seg_off, const int* __restrict__ n_remainders,
                                             long long n, long long s, long long* off, long long* cap)
{
    return clamped_count(seg_off, n, s, n_remainders[s], off, cap);
}

__global__ void __launch_bounds__(THREADS)
krm_medians(const double* __restrict__ ws_values, const long long* __restrict__ seg_off, const int* __restrict__ n_remainders,
            long long n, int F, double* __restrict__ median)
{
    __shared__ SelectShared sh;
    const long long s = blockIdx.x / F;
    const int f = (int)(blockIdx.x % F);
    long long off, cap;
    const int R = remainders_of(seg_off, n_remainders, n, s, &off, &cap);
    select_median(ws_values + (long long)F * off + f * cap, R, median + s * F + f, sh);   // the R values of (segment s, frame f)
}

__global__ void __launch_bounds__(THREADS)
krm_finish(const long long* __restrict__ seg_off, const int* __restrict__ n_remainders, long long n, int F, long long S, int mode,
           int minimum, double* __restrict__ adjustment, unsigned char* __restrict__ kept)
{
    const long long s = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (s >= S) return;
    long long off, cap;
    const int R = remainders_of(seg_off, n_remainders, n, s, &off, &cap);
    kept[s] = (R >= minimum && (mode == FSQ_REMAINDER_RATIO || R >= 1)) ? 1 : 0;
    if (mode == FSQ_REMAINDER_ADDITIVE) {
        const double m0 = adjustment[s * F];
        for (int f = 0; f < F; f++) adjustment[s * F + f] = adjustment[s * F + f] - m0;
    }
}

__global__ void __launch_bounds__(THREADS)
krm_apply(const double* __restrict__ intensity, const int* __restrict__ ws_segment, const double* __restrict__ adjustment,
          const unsigned char* __restrict__ kept, long long total, int F, int mode, double* __restrict__ adjusted)
{
    const long long base = (long long)blockIdx.x * THREADS;        // (uniform: the 64-bit division is the block's, not the lane's)
    const long long i0 = base / F;
    const unsigned t = (unsigned)(base - i0 * F) + threadIdx.x;    // < F + THREADS
    const long long idx = base + threadIdx.x;
    if (idx >= total) return;
    const long long i = i0 + t / (unsigned)F;
    const int f = (int)(t % (unsigned)F);
    const int s = ws_segment[i];
    double r = 0.0;
    if (s >= 0 && kept[s]) {
        const double a = adjustment[(long long)s * F + f], x = intensity[idx];
        r = mode == FSQ_REMAINDER_RATIO ? x * (1.0 - a) : x - a;
    }
    adjusted[idx] = r;
}

bool shape_ok(int64_t n, int F, int64_t S)
{
    return n >= 0 && n < (1ll << 31) && F >= 1 && F <= FSQ_REMAINDER_MAX_FRAMES && S >= 0 && S * (int64_t)F < (1ll << 31);
}

}  // namespace

extern "C" int64_t fsq_remainder_workspace_bytes(int64_t n_tracks, int n_frames, int64_t n_segments)
{
    if (!shape_ok(n_tracks, n_frames, n_segments)) return FSQ_EINVAL;
    return 8 + n_tracks * (int64_t)n_frames * (int64_t)sizeof(double) + n_tracks * (int64_t)sizeof(int);
}

extern "C" int fsq_remainder_adjust(const double* intensity, const uint64_t* category, const int64_t* seg_off, int64_t n, int F,
                                    int64_t S, const FsqRemainderParams* prm, double* adjustment, int32_t* n_remainders,
                                    uint8_t* kept, double* adjusted, void* ws, int64_t ws_bytes, void* stream_)
{
    if (F > FSQ_REMAINDER_MAX_FRAMES) return FSQ_ENOTIMPL;
    if (!shape_ok(n, F, S) || !prm || !seg_off) return FSQ_EINVAL;
    if (prm->mode != FSQ_REMAINDER_RATIO && prm->mode != FSQ_REMAINDER_ADDITIVE) return FSQ_EINVAL;
    if (n > 0 && (!intensity || !category || !adjusted)) return FSQ_EINVAL;
    if (S > 0 && (!adjustment || !n_remainders || !kept)) return FSQ_EINVAL;
    if (!ws || ((uintptr_t)ws & 7) || ws_bytes < fsq_remainder_workspace_bytes(n, F, S)) return FSQ_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    double* ws_values = (double*)ws;
    int* ws_segment = (int*)(ws_values + n * F);
    const int mode = prm->mode;
    if (S > 0) FSQ_HIP_CHECK(hipMemsetAsync(n_remainders, 0, (size_t)S * sizeof(int32_t), stream));
    if (n > 0) {
        hipLaunchKernelGGL(krm_tracks, dim3((unsigned)((n + TRACKS_PER_BLOCK - 1) / TRACKS_PER_BLOCK)), dim3(THREADS), 0, stream,
                           intensity, (const u64*)category, (const long long*)seg_off, (long long)n, F, (long long)S, mode,
                           (int*)n_remainders, ws_values, ws_segment);
        FSQ_HIP_CHECK(hipGetLastError());
    }
    if (S > 0) {
        hipLaunchKernelGGL(krm_medians, dim3((unsigned)(S * F)), dim3(THREADS), 0, stream, (const double*)ws_values,
                           (const long long*)seg_off, (const int*)n_remainders, (long long)n, F, adjustment);
        FSQ_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(krm_finish, dim3((unsigned)((S + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream,
                           (const long long*)seg_off, (const int*)n_remainders, (long long)n, F, (long long)S, mode,
                           (int)prm->minimum_r_per_field, adjustment, (unsigned char*)kept);
        FSQ_HIP_CHECK(hipGetLastError());
    }
    if (n > 0) {
        const long long total = (long long)n * F;
        hipLaunchKernelGGL(krm_apply, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, intensity,
                           (const int*)ws_segment, (const double*)adjustment, (const unsigned char*)kept, total, F, mode, adjusted);
        FSQ_HIP_CHECK(hipGetLastError());
    }
    return FSQ_OK;
}
