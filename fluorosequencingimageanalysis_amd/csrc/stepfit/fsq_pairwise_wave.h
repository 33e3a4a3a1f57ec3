// fsq_pairwise_wave.h - numpy's pairwise sum (fsq_pairwise.h) added by one wavefront: the same tree, the same bits.
//
// numpy splits n > 128 entries into n2 = n / 2, n2 -= n2 % 8 and n - n2 and adds `left + right`; at most 128 entries are one
// leaf (pw_leaf).  For every n <= PW_WAVE_MAX the tree has at most 64 leaves and depth at most 6, so the 6 bits of a lane's
// number, read from the top, name a path from the root: bit 5 chooses the root's half, bit 4 the next, and a lane whose node
// stops splitting at depth t owns that leaf when its remaining 6 - t bits are 0.  The tree is not balanced (n = 249 is the
// first whose leaves sit at different depths), so every lane notes its own depth.  The leaves are added at once, one per
// owning lane; then the levels are combined from the deepest up: at level t the owner of a node that split takes the sum of
// its right half from the lane 1 << (5 - t) above it and adds `left + right`.  A lane whose node stopped splitting higher
// up stays out.
#pragma once
#include <hip/hip_runtime.h>

#include "fsq_pairwise.h"

namespace {

constexpr int PW_WAVE_MAX = 6560;                                  // 3^8 - 1; every n up to it has depth <= 6 (checked on the host for all of them)

// numpy's pairwise sum of g(i), i in [0, n), 0 <= n <= PW_WAVE_MAX, in every lane.  The whole wavefront calls it (a workgroup
// of one dimension whose size is a multiple of 64); g is read once per entry.
template <class G>
__device__ __forceinline__ double pw_sum_wave(const G& g, int n)
{
    const int lane = threadIdx.x & 63;
    int off = 0, len = n, depth = 0;
#pragma unroll
    for (int t = 0; t < 6; t++) {
        if (len > 128) {
            int n2 = len / 2;
            n2 -= n2 % 8;
            if ((lane >> (5 - t)) & 1) { off += n2; len -= n2; } else len = n2;
            depth = t + 1;
        }
    }
    const bool owner = (lane & ((1 << (6 - depth)) - 1)) == 0;
    double val = owner ? pw_leaf(g, off, len) : 0.0;
#pragma unroll
    for (int t = 5; t >= 0; t--) {
        const int s = 1 << (5 - t);
        const double right = __shfl_down(val, s, 64);
        if ((lane & (2 * s - 1)) == 0 && depth > t) val = val + right;
    }
    return __shfl(val, 0, 64);
}

// np.mean of g(i), i in [0, n): np.add.reduce starts from +0.0 (fsq_pairwise.h says why); NaN for n = 0
template <class G>
__device__ __forceinline__ double np_mean_wave(const G& g, int n)
{
    return (0.0 + pw_sum_wave(g, n)) / (double)n;
}

}  // namespace
