// fsq_channel_offset.hip - the integer offset between two colour channels from the track positions themselves
// (include/fsq_channel_offset.h): a displacement vote over all fields, scored under the match's own radius, in exact integers.
// Two kernels:
//
// kco_votes, kcl_match's mapping: one lane per a, 256 per block (and lane s < n_seg also proves segment s's offsets); the lane
//   walks its segment's B range from global memory - the lanes of a wave mostly stand in one segment and walk it in step, so
//   their loads of b are one address - and adds one vote per b with |dh| <= W and |dw| <= W to the block's uint32 histogram in
//   LDS, cleared at block start.  At block end the non-zero bins go to the global int64 histogram with 64-bit integer atomics:
//   integer adds commute, so V is exact and the same in every run.
//   No 32-bit counter wraps: a lane votes at most once per b of its segment, a lane whose segment holds 2^24 or more b's votes
//   nothing and sets d_bad, so a bin of a block's histogram receives at most 256 x (2^24 - 1) = 2^32 - 256 votes.
//   The histogram is (2W + 1)^2 words of dynamic LDS: 66 564 B at W = 64, above the 64 KB a launch gets by default, so the
//   entry raises the kernel's limit first (160 KiB per CU leave room for two such blocks).
//
// kco_peak, one block: every lane scores its offsets of the window [-R, R]^2 (S[o] = the sum of V[o + d] over |d|^2 <= tol_sq)
//   and keeps its best under (larger S, smaller dh^2 + dw^2, smaller dh, smaller dw) - a total order, so the block's reduction
//   gives one answer whatever its shape; a second pass scores the window again for runner_up and n_ties and sums V.
//
// Bounds: a range is walked only after 0 <= off[s] <= off[s + 1] <= n was seen for it, with s in 0 .. n_seg - 1; every index of
// a_hw and b_hw is then inside it, whatever a_seg and the offsets hold.  A vote's bin is computed from differences already
// proven to lie in -W .. W.  In kco_peak R + t <= W keeps every tap inside V; the 3 x 3 tests each bin against V's edge.
#include <hip/hip_runtime.h>

#include "../fsq_common.h"
#include "../../../include/fsq_channel_offset.h"

namespace {

constexpr int THREADS = 256;
constexpr long long MAX_SEGMENT_B = 1ll << 24;                     // 256 lanes x 2^24 votes = 2^32: one too many for a uint32 bin

__device__ __forceinline__ bool range_ok(const long long* __restrict__ off, long long s, long long n, long long* lo, long long* hi)
{
    *lo = off[s];
    *hi = off[s + 1];
    return *lo >= 0 && *lo <= *hi && *hi <= n;
}

__global__ void __launch_bounds__(THREADS)
kco_votes(const int2* __restrict__ a_hw, const int* __restrict__ a_seg, const long long* __restrict__ a_off,
          const long long* __restrict__ b_off, const int2* __restrict__ b_hw, int W, long long n_a, long long n_b, long long n_seg,
          unsigned long long* __restrict__ votes, int* __restrict__ d_bad)
{
    extern __shared__ unsigned hist[];
    const int side = 2 * W + 1, bins = side * side;
    for (int k = threadIdx.x; k < bins; k += THREADS) hist[k] = 0u;
    __syncthreads();
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    long long a0, a1, b0, b1;
    if (i < n_seg) {                                               // segment i's offsets, and the two ends
        bool ok = range_ok(a_off, i, n_a, &a0, &a1) && range_ok(b_off, i, n_b, &b0, &b1);
        if (ok && i == 0) ok = a0 == 0 && b0 == 0;
        if (ok && i == n_seg - 1) ok = a1 == n_a && b1 == n_b;
        if (!ok) *d_bad = 1;
    }
    if (i < n_a) {
        const long long s = a_seg[i];
        bool ok = s >= 0 && s < n_seg;
        ok = ok && range_ok(a_off, s, n_a, &a0, &a1) && range_ok(b_off, s, n_b, &b0, &b1) && a0 <= i && i < a1;
        ok = ok && b1 - b0 < MAX_SEGMENT_B;
        if (!ok) {
            *d_bad = 1;
        } else {
            const int2 a = a_hw[i];
            for (long long j = b0; j < b1; j++) {
                const int2 b = b_hw[j];
                const long long dh = (long long)a.x - (long long)b.x, dw = (long long)a.y - (long long)b.y;
                if (dh >= -W && dh <= W && dw >= -W && dw <= W) atomicAdd(&hist[((int)dh + W) * side + (int)dw + W], 1u);
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < bins; k += THREADS) {
        const unsigned v = hist[k];
        if (v) atomicAdd(&votes[k], (unsigned long long)v);
    }
}

// (larger S, smaller d2, smaller dh, smaller dw): whether (s, dh, dw) comes before (bs, bdh, bdw)
__device__ __forceinline__ bool before(long long s, long long dh, long long dw, long long bs, long long bdh, long long bdw)
{
    if (s != bs) return s > bs;
    const long long d2 = dh * dh + dw * dw, bd2 = bdh * bdh + bdw * bdw;
    if (d2 != bd2) return d2 < bd2;
    if (dh != bdh) return dh < bdh;
    return dw < bdw;
}

__device__ __forceinline__ long long score_at(const long long* __restrict__ V, int W, int t, long long tol_sq, int oh, int ow)
{
    const int side = 2 * W + 1;
    long long s = 0;
    for (int dh = -t; dh <= t; dh++)
        for (int dw = -t; dw <= t; dw++)
            if ((long long)(dh * dh + dw * dw) <= tol_sq) s += V[(oh + dh + W) * side + (ow + dw + W)];
    return s;
}

__global__ void __launch_bounds__(THREADS)
kco_peak(const long long* __restrict__ V, int W, int R, int t, long long tol_sq, long long* __restrict__ result,
         long long* __restrict__ scores)
{
    __shared__ long long sh_a[THREADS], sh_b[THREADS], sh_c[THREADS];
    __shared__ unsigned char sh_has[THREADS];
    const int tid = threadIdx.x, win = 2 * R + 1, n_off = win * win, side = 2 * W + 1, bins = side * side;
    // pass 1: S over the window, the lane's best
    long long best_s = 0, best_dh = 0, best_dw = 0;
    bool has = false;
    for (int k = tid; k < n_off; k += THREADS) {
        const int oh = k / win - R, ow = k % win - R;
        const long long s = score_at(V, W, t, tol_sq, oh, ow);
        if (scores) scores[k] = s;
        if (!has || before(s, oh, ow, best_s, best_dh, best_dw)) { best_s = s; best_dh = oh; best_dw = ow; has = true; }
    }
    sh_a[tid] = best_s; sh_b[tid] = best_dh; sh_c[tid] = best_dw; sh_has[tid] = has;
    __syncthreads();
    for (int step = THREADS / 2; step > 0; step >>= 1) {
        if (tid < step && sh_has[tid + step]
            && (!sh_has[tid] || before(sh_a[tid + step], sh_b[tid + step], sh_c[tid + step], sh_a[tid], sh_b[tid], sh_c[tid]))) {
            sh_a[tid] = sh_a[tid + step]; sh_b[tid] = sh_b[tid + step]; sh_c[tid] = sh_c[tid + step]; sh_has[tid] = 1;
        }
        __syncthreads();
    }
    const long long peak_s = sh_a[0];
    const int peak_dh = (int)sh_b[0], peak_dw = (int)sh_c[0];      // (lane 0 holds offset k = 0: the window is never empty)
    __syncthreads();
    // pass 2: the runner-up beyond 2t of the peak, the ties, the sum of V
    long long runner = -1, ties = 0, total = 0;
    for (int k = tid; k < n_off; k += THREADS) {
        const int oh = k / win - R, ow = k % win - R;
        const long long s = score_at(V, W, t, tol_sq, oh, ow);
        const int ch = oh > peak_dh ? oh - peak_dh : peak_dh - oh, cw = ow > peak_dw ? ow - peak_dw : peak_dw - ow;
        if ((ch > cw ? ch : cw) > 2 * t && s > runner) runner = s;
        ties += s == peak_s;
    }
    for (int k = tid; k < bins; k += THREADS) total += V[k];
    sh_a[tid] = runner; sh_b[tid] = ties; sh_c[tid] = total;
    __syncthreads();
    for (int step = THREADS / 2; step > 0; step >>= 1) {
        if (tid < step) {
            if (sh_a[tid + step] > sh_a[tid]) sh_a[tid] = sh_a[tid + step];
            sh_b[tid] += sh_b[tid + step];
            sh_c[tid] += sh_c[tid + step];
        }
        __syncthreads();
    }
    if (tid == 0) {
        result[0] = peak_dh; result[1] = peak_dw; result[2] = peak_s; result[3] = sh_a[0]; result[4] = sh_c[0];
        result[5] = (peak_dh == R || peak_dh == -R || peak_dw == R || peak_dw == -R) ? 1 : 0;
        result[6] = sh_b[0];
    }
    if (tid < 9) {
        const int h = peak_dh + tid / 3 - 1, w = peak_dw + tid % 3 - 1;
        result[7 + tid] = (h >= -W && h <= W && w >= -W && w <= W) ? V[(h + W) * side + (w + W)] : 0;
    }
}

}  // namespace

extern "C" int fsq_channel_offset_votes(const int32_t* a_hw, const int32_t* a_seg, const int64_t* a_off, const int64_t* b_off,
                                        const int32_t* b_hw, int64_t W, int64_t n_a, int64_t n_b, int64_t n_seg, int64_t* votes,
                                        int32_t* d_bad, void* stream_)
{
    const int64_t lim = 1ll << 31;
    if (n_a < 0 || n_b < 0 || n_seg < 0 || W < 0 || W > FSQ_CHANNEL_OFFSET_MAX_W || n_a >= lim || n_b >= lim || n_seg >= lim)
        return FSQ_EINVAL;
    if (!d_bad || !a_off || !b_off || !votes) return FSQ_EINVAL;
    if (n_a > 0 && (!a_hw || !a_seg)) return FSQ_EINVAL;
    if (n_b > 0 && !b_hw) return FSQ_EINVAL;
    if (((uintptr_t)a_hw | (uintptr_t)b_hw | (uintptr_t)a_off | (uintptr_t)b_off | (uintptr_t)votes) & 7) return FSQ_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t bins = (size_t)(2 * W + 1) * (size_t)(2 * W + 1), lds = bins * sizeof(unsigned);
    FSQ_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int32_t), stream));
    FSQ_HIP_CHECK(hipMemsetAsync(votes, 0, bins * sizeof(int64_t), stream));
    const int64_t lanes = n_a > n_seg ? n_a : n_seg;
    if (lanes > 0) {
        if (lds > 48 * 1024)                                       // (above what every launch may have: W = 64 needs 66 564 B)
            FSQ_HIP_CHECK(hipFuncSetAttribute((const void*)kco_votes, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kco_votes, dim3((unsigned)((lanes + THREADS - 1) / THREADS)), dim3(THREADS), lds, stream, (const int2*)a_hw,
                           (const int*)a_seg, (const long long*)a_off, (const long long*)b_off, (const int2*)b_hw, (int)W,
                           (long long)n_a, (long long)n_b, (long long)n_seg, (unsigned long long*)votes, (int*)d_bad);
        FSQ_HIP_CHECK(hipGetLastError());
    }
    return FSQ_OK;
}

extern "C" int fsq_channel_offset_peak(const int64_t* votes, int64_t W, int64_t R, int64_t tol_sq, int64_t* result, int64_t* scores,
                                       void* stream_)
{
    if (W < 0 || W > FSQ_CHANNEL_OFFSET_MAX_W || R < 0 || R > W || tol_sq < 0) return FSQ_EINVAL;
    int64_t t = 0;                                                 // isqrt(tol_sq), as far as it matters
    while (t <= W && (t + 1) * (t + 1) <= tol_sq) t++;
    if (R + t > W) return FSQ_EINVAL;
    if (!votes || !result) return FSQ_EINVAL;
    if (((uintptr_t)votes | (uintptr_t)result | (uintptr_t)scores) & 7) return FSQ_EINVAL;
    hipLaunchKernelGGL(kco_peak, dim3(1), dim3(THREADS), 0, (hipStream_t)stream_, (const long long*)votes, (int)W, (int)R, (int)t,
                       (long long)tol_sq, (long long*)result, (long long*)scores);
    FSQ_HIP_CHECK(hipGetLastError());
    return FSQ_OK;
}
