// fsq_lognormal_chain.hip - the per-track steps between the two fits of the lognormal chain (include/fsq_lognormal_chain.h):
// last_drop_method_v2's list (:5357-5384), grab_ON_OFFS (:63-84) with its medians and ON_OFF_adjust_photometries (:262-276),
// with numpy's bits.  Five kernels:
//
// kch_last_drops, one wavefront per track and one lane per frame: a ballot of the lanes that give a value.  The counting pass
//   writes its population count; the writing pass puts log(I_f) at the track's offset plus the count of the lanes below, so
//   the values stand in (track, frame) order whatever order the wavefronts run in.
// kch_scatter, one wavefront per track: finds the track's segment and, where the first fit found a sequence, lane f takes a
//   slot of key (segment, f) from an atomic counter, which is on_off_count itself, and writes I_f - alpha to the workspace,
//   segment by segment and frame by frame: ws[(F - 1) * seg_off[s] + f * cap + slot], cap the segment's tracks.
// kch_key_medians, one 256-thread block per key: select_median (fsq_select_median.h) of the key's entries; a key with entries
//   also appends its median to the list of medians (an atomic slot again: the order does not matter to a median).
// kch_median_of_medians, one block: select_median of that list.
// kch_adjust, one thread per value: 8 bytes read, 8 written, the key's median and count from cache.
//
// Bounds: a segment is used only where 0 <= seg_off[s] <= seg_off[s + 1] <= n and a track only in the segment that holds it, so
// a key has at most cap entries; a slot is used only below cap.  With that every workspace index is below n * (F - 1), whatever
// seg_off holds.  The list of medians takes at most one per key, S * (F - 1).
#include <hip/hip_runtime.h>
#include <math.h>

#include "../fsq_common.h"
#include "../fsq_devmath.h"
#include "../../../include/fsq_lognormal_chain.h"
#include "../libm/fsq_glibc_log.h"
#include "fsq_select_median.h"

namespace {

constexpr int THREADS = SELECT_THREADS;
constexpr int WAVE = SELECT_WAVE;
constexpr int TRACKS_PER_BLOCK = THREADS / WAVE;
static_assert(FSQ_CHAIN_MAX_FRAMES <= WAVE, "one lane per frame");

// frame `lane` is ON and the next one is OFF; false for the last frame
__device__ __forceinline__ bool on_then_off(u64 c, int lane, int F)
{
    const int next = lane < 63 ? lane + 1 : 63;
    return lane + 1 < F && ((c >> lane) & 1ull) && !((c >> next) & 1ull);
}

template <bool WRITE>
__global__ void __launch_bounds__(THREADS)
kch_last_drops(const double* __restrict__ intensity, const u64* __restrict__ category, long long n, int F, int truncate,
               const long long* __restrict__ track_off, long long* __restrict__ track_count, double* __restrict__ values,
               long long capacity)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long i = (long long)blockIdx.x * TRACKS_PER_BLOCK + (threadIdx.x / WAVE);
    if (i >= n) return;                                            // (uniform over the wavefront; the kernel has no barrier)
    const double x = lane < F ? intensity[i * F + lane] : 0.0;
    const bool take = lane >= truncate && on_then_off(category[i], lane, F) && x > 0.0;
    const u64 mask = __ballot(take);
    const long long count = __popcll(mask);
    if (!WRITE) {
        if (lane == 0) track_count[i] = count;
        return;
    }
    const long long o = track_off[i];
    if (o < 0 || o > capacity || count > capacity - o) return;
    if (take) values[o + __popcll(mask & ((1ull << lane) - 1ull))] = ln_log(x);
}

__global__ void __launch_bounds__(THREADS)
kch_scatter(const double* __restrict__ intensity, const u64* __restrict__ category, const long long* __restrict__ seg_off,
            const int* __restrict__ fit_status, long long n, int F, long long S, double alpha, int* __restrict__ on_off_count,
            double* __restrict__ ws_values)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const long long i = (long long)blockIdx.x * TRACKS_PER_BLOCK + (threadIdx.x / WAVE);
    if (i >= n) return;                                            // (uniform over the wavefront; the kernel has no barrier)
    long long off = 0, cap = 0;
    const long long s = segment_of(seg_off, S, n, i, &off, &cap);
    if (s < 0 || fit_status[i] != 0) return;
    if (!on_then_off(category[i], lane, F)) return;
    const int K = F - 1;
    const int slot = atomicAdd(&on_off_count[s * K + lane], 1);
    if (slot < cap) ws_values[(long long)K * off + lane * cap + slot] = intensity[i * F + lane] - alpha;
}

__global__ void __launch_bounds__(THREADS)
kch_key_medians(const double* __restrict__ ws_values, const long long* __restrict__ seg_off, const int* __restrict__ on_off_count,
                long long n, int F, double* __restrict__ median, int* __restrict__ n_medians, double* __restrict__ ws_medians)
{
    __shared__ SelectShared sh;
    const int K = F - 1;
    const long long s = blockIdx.x / K;
    const int f = (int)(blockIdx.x % K);
    long long off, cap;
    const int R = clamped_count(seg_off, n, s, on_off_count[s * K + f], &off, &cap);
    double* out = median + s * K + f;
    select_median(ws_values + (long long)K * off + f * cap, R, out, sh);
    if (R > 0 && threadIdx.x == 0) ws_medians[atomicAdd(n_medians, 1)] = *out;     // (thread 0 wrote *out itself; one slot per block)
}

__global__ void __launch_bounds__(THREADS)
kch_median_of_medians(const double* __restrict__ ws_medians, const int* __restrict__ n_medians, long long keys,
                      double* __restrict__ last_beta_median)
{
    __shared__ SelectShared sh;
    const long long have = *n_medians;
    select_median(ws_medians, (int)(have < keys ? have : keys), last_beta_median, sh);
}

__global__ void __launch_bounds__(THREADS)
kch_adjust(const double* __restrict__ intensity, const long long* __restrict__ seg_off, long long n, long long total, int F,
           long long S, double alpha, const double* __restrict__ median, const int* __restrict__ on_off_count,
           const double* __restrict__ last_beta_median, double* __restrict__ adjusted)
{
    const long long base = (long long)blockIdx.x * THREADS;        // (uniform: the 64-bit division is the block's, not the lane's)
    const long long i0 = base / F;
    const unsigned t = (unsigned)(base - i0 * F) + threadIdx.x;    // < F + THREADS
    const long long idx = base + threadIdx.x;
    if (idx >= total) return;
    const long long i = i0 + t / (unsigned)F;
    const int f = (int)(t % (unsigned)F);
    const double x = intensity[idx];
    double r = x;
    if (f < F - 1) {
        long long off = 0, cap = 0;
        const long long s = segment_of(seg_off, S, n, i, &off, &cap);
        if (s >= 0 && on_off_count[s * (F - 1) + f] > 0) r = (x - alpha) * *last_beta_median / median[s * (F - 1) + f];
    }
    adjusted[idx] = r;
}

int shape_rc(int64_t n, int F, int64_t S)
{
    if (F > FSQ_CHAIN_MAX_FRAMES) return FSQ_ENOTIMPL;
    if (n < 0 || n >= (1ll << 31) || F < 1 || S < 0 || S >= (1ll << 31) || S * (int64_t)(F - 1) >= (1ll << 31)) return FSQ_EINVAL;
    return FSQ_OK;
}

unsigned blocks_of(long long items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

}  // namespace

extern "C" int64_t fsq_chain_last_drops_workspace_bytes(int64_t n_tracks, int n_frames, int64_t n_segments)
{
    (void)n_segments;
    return shape_rc(n_tracks, n_frames, 0) != FSQ_OK ? FSQ_EINVAL : 0;
}

extern "C" int64_t fsq_chain_on_off_medians_workspace_bytes(int64_t n_tracks, int n_frames, int64_t n_segments)
{
    if (shape_rc(n_tracks, n_frames, n_segments) != FSQ_OK) return FSQ_EINVAL;
    return 8 + (n_tracks + n_segments) * (int64_t)(n_frames - 1) * (int64_t)sizeof(double);
}

extern "C" int64_t fsq_chain_on_off_adjust_workspace_bytes(int64_t n_tracks, int n_frames, int64_t n_segments)
{
    return shape_rc(n_tracks, n_frames, n_segments) != FSQ_OK ? FSQ_EINVAL : 0;
}

extern "C" int fsq_chain_last_drops(const double* intensity, const uint64_t* category, int64_t n, int F, int truncate,
                                    const int64_t* track_off, int64_t* track_count, double* values, int64_t capacity, void* ws,
                                    int64_t ws_bytes, void* stream_)
{
    (void)ws;
    (void)ws_bytes;
    const int rc = shape_rc(n, F, 0);
    if (rc != FSQ_OK) return rc;
    if (truncate < 0 || capacity < 0) return FSQ_EINVAL;
    if (n > 0 && (!intensity || !category)) return FSQ_EINVAL;
    if (n > 0 && !track_off && !track_count) return FSQ_EINVAL;
    if (n > 0 && track_off && capacity > 0 && !values) return FSQ_EINVAL;
    if (n == 0) return FSQ_OK;
    hipStream_t stream = (hipStream_t)stream_;
    const dim3 grid(blocks_of(n, TRACKS_PER_BLOCK)), block(THREADS);
    if (!track_off)
        hipLaunchKernelGGL(kch_last_drops<false>, grid, block, 0, stream, intensity, (const u64*)category, (long long)n, F, truncate,
                           (const long long*)nullptr, (long long*)track_count, (double*)nullptr, 0ll);
    else
        hipLaunchKernelGGL(kch_last_drops<true>, grid, block, 0, stream, intensity, (const u64*)category, (long long)n, F, truncate,
                           (const long long*)track_off, (long long*)nullptr, values, (long long)capacity);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_chain_on_off_medians(const double* intensity, const uint64_t* category, const int64_t* seg_off,
                                        const int32_t* fit_status, int64_t n, int F, int64_t S, double alpha, double* on_off_median,
                                        int32_t* on_off_count, double* last_beta_median, void* ws, int64_t ws_bytes, void* stream_)
{
    const int rc = shape_rc(n, F, S);
    if (rc != FSQ_OK) return rc;
    if (!seg_off || !last_beta_median) return FSQ_EINVAL;
    if (n > 0 && (!intensity || !category || !fit_status)) return FSQ_EINVAL;
    const int64_t keys = S * (int64_t)(F - 1);
    if (keys > 0 && (!on_off_median || !on_off_count)) return FSQ_EINVAL;
    if (!ws || ((uintptr_t)ws & 7) || ws_bytes < fsq_chain_on_off_medians_workspace_bytes(n, F, S)) return FSQ_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    int* n_medians = (int*)ws;                                     // 8 bytes, then the entries, then the list of medians
    double* ws_values = (double*)ws + 1;
    double* ws_medians = ws_values + n * (int64_t)(F - 1);
    FSQ_HIP_CHECK(hipMemsetAsync(n_medians, 0, 8, stream));
    if (keys > 0) {
        FSQ_HIP_CHECK(hipMemsetAsync(on_off_count, 0, (size_t)keys * sizeof(int32_t), stream));
        if (n > 0) {
            hipLaunchKernelGGL(kch_scatter, dim3(blocks_of(n, TRACKS_PER_BLOCK)), dim3(THREADS), 0, stream, intensity,
                               (const u64*)category, (const long long*)seg_off, (const int*)fit_status, (long long)n, F, (long long)S,
                               alpha, (int*)on_off_count, ws_values);
            FSQ_HIP_CHECK(hipGetLastError());
        }
        hipLaunchKernelGGL(kch_key_medians, dim3((unsigned)keys), dim3(THREADS), 0, stream, (const double*)ws_values,
                           (const long long*)seg_off, (const int*)on_off_count, (long long)n, F, on_off_median, n_medians, ws_medians);
        FSQ_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(kch_median_of_medians, dim3(1), dim3(THREADS), 0, stream, (const double*)ws_medians, (const int*)n_medians,
                       (long long)keys, last_beta_median);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}

extern "C" int fsq_chain_on_off_adjust(const double* intensity, const int64_t* seg_off, int64_t n, int F, int64_t S, double alpha,
                                       const double* on_off_median, const int32_t* on_off_count, const double* last_beta_median,
                                       double* adjusted, void* ws, int64_t ws_bytes, void* stream_)
{
    (void)ws;
    (void)ws_bytes;
    const int rc = shape_rc(n, F, S);
    if (rc != FSQ_OK) return rc;
    if (!seg_off || !last_beta_median) return FSQ_EINVAL;
    if (n > 0 && (!intensity || !adjusted)) return FSQ_EINVAL;
    if (S * (int64_t)(F - 1) > 0 && (!on_off_median || !on_off_count)) return FSQ_EINVAL;
    if (n == 0) return FSQ_OK;
    const long long total = (long long)n * F;
    hipLaunchKernelGGL(kch_adjust, dim3(blocks_of(total, THREADS)), dim3(THREADS), 0, (hipStream_t)stream_, intensity,
                       (const long long*)seg_off, (long long)n, total, F, (long long)S, alpha, on_off_median, (const int*)on_off_count,
                       last_beta_median, adjusted);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
