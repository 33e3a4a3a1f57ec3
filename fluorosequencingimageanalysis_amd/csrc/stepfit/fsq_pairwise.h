// fsq_pairwise.h - numpy's pairwise sum (loops_utils.h.src, PW_BLOCKSIZE 128) and np.mean on the device, shared by the
// step-fit kernels (fsq_stepfit.hip, fsq_chisq.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace {

// ---- numpy pairwise sum of g(i), i in [off, off + n) ----------------------------------------------------------
template <class G>
__device__ __forceinline__ double pw_leaf(const G& g, int off, int n)
{
    if (n < 8) {
        double res = 0.;
        for (int i = 0; i < n; i++) res += g(off + i);
        return res;
    }
    double r[8];
#pragma unroll
    for (int k = 0; k < 8; k++) r[k] = g(off + k);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
        for (int k = 0; k < 8; k++) r[k] += g(off + i + k);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; i++) res += g(off + i);
    return res;
}
// n <= 8192: every split leaves at most n / 2 + 8, so 7 levels reach the 128-element leaves
template <int D, class G>
__device__ double pw_sum(const G& g, int off, int n)
{
    if constexpr (D == 0) {
        return pw_leaf(g, off, n);
    } else {
        if (n <= 128) return pw_leaf(g, off, n);
        int n2 = n / 2;
        n2 -= n2 % 8;
        return pw_sum<D - 1>(g, off, n2) + pw_sum<D - 1>(g, off + n2, n - n2);
    }
}
// np.mean: np.add.reduce starts from the identity +0.0 and adds the pairwise sum to it, so frames that are all -0.0 have the
// mean +0.0 (the sum alone would be -0.0 from 8 frames on, where the accumulators start from the frames themselves)
__device__ __forceinline__ double np_mean_short(const double* a, int n)      // n <= 128
{
    return (0.0 + pw_leaf([a](int i) { return a[i]; }, 0, n)) / (double)n;
}
__device__ double np_mean(const double* a, int n)
{
    return (0.0 + pw_sum<8>([a](int i) { return a[i]; }, 0, n)) / (double)n;
}

// The same sum without calls: each level is a two-trip loop over its halves, so a call site holds D + 1 copies of the
// leaf instead of a call tree (a kernel that makes no call needs no scratch frame).  Every split leaves at most n / 2 + 8, so D = 4 serves n <= 1024 and D = 7 serves n <= 8192.
template <int D, class G>
__device__ __forceinline__ double pw_sum_flat(const G& g, int off, int n)
{
    if constexpr (D == 0) {
        return pw_leaf(g, off, n);
    } else {
        if (n <= 128) return pw_leaf(g, off, n);
        int n2 = n / 2;
        n2 -= n2 % 8;
        double acc = 0.0;
#pragma nounroll
        for (int h = 0; h < 2; h++) {
            const double v = pw_sum_flat<D - 1>(g, h ? off + n2 : off, h ? n - n2 : n2);
            acc = h ? acc + v : v;
        }
        return acc;
    }
}
template <int D>
__device__ __forceinline__ double np_mean_flat(const double* a, int n)
{
    return (0.0 + pw_sum_flat<D>([a](int i) { return a[i]; }, 0, n)) / (double)n;
}

}  // namespace
