// fsq_colocalize.hip - which tracks of two colour channels are the same molecule (include/fsq_colocalize.h): the mutual
// nearest neighbours within a radius, field by field, in exact integers.  One kernel:
//
// kcl_match, one lane per a (and lane s < n_seg also proves segment s's offsets): the lane scans its segment's B range for
//   best_b(a), the smallest (d2, index) with d2 <= radius_sq - ascending index and a strict `<`, so a tie stays with the
//   lowest index -, then the segment's A range for an a' that b prefers: (d2(a', b), a') < (d2(a, b), a).  Without one a is
//   best_a(b) and the lane stores match_of_a[a] = b, match_of_b[b] = a, dist_sq_of_a[a] = d2.  best_a(b) is one a, so
//   match_of_b[b] has one writer; the other elements are the lane's own.  Brute force from global memory: the lanes of a wave
//   mostly stand in one segment and walk it in step, so their loads of b (and of a') are the same address.
//
// Bounds: a range is walked only after 0 <= off[s] <= off[s + 1] <= n was seen for it, with s in 0 .. n_seg - 1; every index
// of a_hw, b_hw and match_of_b is then inside it, whatever a_seg and the offsets hold.
#include <hip/hip_runtime.h>

#include "../fsq_common.h"
#include "../../../include/fsq_colocalize.h"

namespace {

constexpr int THREADS = 256;

__device__ __forceinline__ bool range_ok(const long long* __restrict__ off, long long s, long long n, long long* lo, long long* hi)
{
    *lo = off[s];
    *hi = off[s + 1];
    return *lo >= 0 && *lo <= *hi && *hi <= n;
}

__device__ __forceinline__ long long dist_sq(int2 p, int2 q)
{
    const long long dh = (long long)p.x - (long long)q.x, dw = (long long)p.y - (long long)q.y;
    return dh * dh + dw * dw;
}

__global__ void __launch_bounds__(THREADS)
kcl_match(const int2* __restrict__ a_hw, const int* __restrict__ a_seg, const long long* __restrict__ a_off,
          const long long* __restrict__ b_off, const int2* __restrict__ b_hw, long long radius_sq, long long n_a, long long n_b,
          long long n_seg, int* __restrict__ match_of_a, int* __restrict__ match_of_b, long long* __restrict__ dist_sq_of_a,
          int* __restrict__ d_bad)
{
    const long long i = (long long)blockIdx.x * THREADS + threadIdx.x;
    long long a0, a1, b0, b1;
    if (i < n_seg) {                                               // segment i's offsets, and the two ends
        bool ok = range_ok(a_off, i, n_a, &a0, &a1) && range_ok(b_off, i, n_b, &b0, &b1);
        if (ok && i == 0) ok = a0 == 0 && b0 == 0;
        if (ok && i == n_seg - 1) ok = a1 == n_a && b1 == n_b;
        if (!ok) *d_bad = 1;
    }
    if (i >= n_a) return;
    const long long s = a_seg[i];
    bool ok = s >= 0 && s < n_seg;
    ok = ok && range_ok(a_off, s, n_a, &a0, &a1) && range_ok(b_off, s, n_b, &b0, &b1) && a0 <= i && i < a1;
    long long best = -1, best_d = -1;
    if (!ok) {
        *d_bad = 1;
    } else {
        const int2 a = a_hw[i];
        for (long long j = b0; j < b1; j++) {
            const long long d = dist_sq(a, b_hw[j]);
            if (d <= radius_sq && (best < 0 || d < best_d)) { best = j; best_d = d; }
        }
        if (best >= 0) {
            const int2 b = b_hw[best];
            for (long long k = a0; k < a1; k++) {
                const long long d = dist_sq(a_hw[k], b);
                if (d < best_d || (d == best_d && k < i)) { best = -1; best_d = -1; break; }      // b prefers a' = k
            }
        }
    }
    match_of_a[i] = (int)best;
    dist_sq_of_a[i] = best_d;
    if (best >= 0) match_of_b[best] = (int)i;
}

}  // namespace

extern "C" int fsq_colocalize_match(const int32_t* a_hw, const int32_t* a_seg, const int64_t* a_off, const int64_t* b_off,
                                    const int32_t* b_hw, int64_t radius_sq, int64_t n_a, int64_t n_b, int64_t n_seg,
                                    int32_t* match_of_a, int32_t* match_of_b, int64_t* dist_sq_of_a, int32_t* d_bad, void* stream_)
{
    const int64_t lim = 1ll << 31;
    if (n_a < 0 || n_b < 0 || n_seg < 0 || radius_sq < 0 || n_a >= lim || n_b >= lim || n_seg >= lim) return FSQ_EINVAL;
    if (!d_bad || !a_off || !b_off) return FSQ_EINVAL;
    if (n_a > 0 && (!a_hw || !a_seg || !match_of_a || !dist_sq_of_a)) return FSQ_EINVAL;
    if (n_b > 0 && (!b_hw || !match_of_b)) return FSQ_EINVAL;
    if (((uintptr_t)a_hw | (uintptr_t)b_hw | (uintptr_t)a_off | (uintptr_t)b_off | (uintptr_t)dist_sq_of_a) & 7) return FSQ_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    FSQ_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(int32_t), stream));
    if (n_b > 0) FSQ_HIP_CHECK(hipMemsetAsync(match_of_b, 0xFF, (size_t)n_b * sizeof(int32_t), stream));
    const int64_t lanes = n_a > n_seg ? n_a : n_seg;
    if (lanes > 0) {
        hipLaunchKernelGGL(kcl_match, dim3((unsigned)((lanes + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, (const int2*)a_hw,
                           (const int*)a_seg, (const long long*)a_off, (const long long*)b_off, (const int2*)b_hw, (long long)radius_sq,
                           (long long)n_a, (long long)n_b, (long long)n_seg, (int*)match_of_a, (int*)match_of_b,
                           (long long*)dist_sq_of_a, (int*)d_bad);
        FSQ_HIP_CHECK(hipGetLastError());
    }
    return FSQ_OK;
}
