// fsq_philox.h - the library's own random draws: Philox4x32-10 blocks, CPython's 53-bit uniform and numpy's legacy polar
// normals, shared by the peptide simulation (fsq_peptide_sim.hip) and the Monte-Carlo PSF fit (fsq_montecarlo.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../libm/fsq_glibc_log.h"

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

struct Words { uint32_t w0, w1, w2, w3; };

__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)PHILOX_M0 * c0, p1 = (unsigned long long)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    Words w;
    w.w0 = c0; w.w1 = c1; w.w2 = c2; w.w3 = c3;
    return w;
}

// CPython's random(): ((a >> 5) * 67108864 + (b >> 6)) / 2^53, exact in fp64
__device__ __forceinline__ double uniform53(uint32_t a, uint32_t b)
{
    return (double)(((unsigned long long)(a >> 5) << 26) | (unsigned long long)(b >> 6)) * 0x1p-53;
}

// numpy's legacy_gauss on the blocks (block, c1, c2, c3), block = *block, *block + 1, ...: one block is one attempt (its two
// uniforms).  Returns the value handed out first, fac * x2; *second = fac * x1 is the one numpy caches for the next call.
__device__ __forceinline__ double polar_pair(int* block, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, double* second)
{
    double x1, x2, r2;
    do {
        const Words w = philox4x32_10((uint32_t)*block, c1, c2, c3, k0, k1);
        *block += 1;
        x1 = 2.0 * uniform53(w.w0, w.w1) - 1.0;
        x2 = 2.0 * uniform53(w.w2, w.w3) - 1.0;
        r2 = x1 * x1 + x2 * x2;
    } while (r2 >= 1.0 || r2 == 0.0);
    const double fac = sqrt(-2.0 * ln_log(r2) / r2);
    *second = fac * x1;
    return fac * x2;
}

}  // namespace
