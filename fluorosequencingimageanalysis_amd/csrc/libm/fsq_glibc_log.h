// fsq_glibc_log.h - log(x) as glibc 2.35 computes it on x86-64 with FMA (e_log.c, the ifunc-selected __log_fma), for the
// lognormal fluor-count fit (fsq_lognormal.hip).  Include after ../fsq_devmath.h.
// Every fma below is one the FMA build of e_log.c has (the compiler contracted the C source there; -ffp-contract=off here),
// every other operation is a separately rounded IEEE fp64 add or multiply, so the bits are glibc's.
#pragma once

#include "fsq_log_tables.h"

namespace {

// log(x) for every double: +-0 -> -inf (__math_divzero), x < 0 and NaN -> NaN (__math_invalid), +inf -> +inf.
__device__ __forceinline__ double ln_log(double x)
{
    unsigned long long ix = fsq_bits(x);
    const unsigned top = (unsigned)(ix >> 48);
    if (ix - 0x3fee000000000000ull < 0x3ff1090000000000ull - 0x3fee000000000000ull) {     // 1 - 2^-4 <= x < 1 + 0x1.09p-4
        if (ix == 0x3ff0000000000000ull) return 0.0;
        const double r = x - 1.0;
        const double r2 = r * r;
        const double r3 = r * r2;
        const double q1 = fsq_fma(r2, LOG_B[3], fsq_fma(r, LOG_B[2], LOG_B[1]));
        const double q2 = fsq_fma(r2, LOG_B[6], fsq_fma(r, LOG_B[5], LOG_B[4]));
        double q3 = fsq_fma(r2, LOG_B[9], fsq_fma(r, LOG_B[8], LOG_B[7]));
        q3 = fsq_fma(r3, LOG_B[10], q3);
        double p = fsq_fma(q3, r3, q2);
        p = fsq_fma(p, r3, q1);
        const double t = fsq_fma(r, 0x1p27, r);                  // r + w with w = r * 2^27 ...
        const double rhi = fsq_fma(-0x1p27, r, t);               // ... - w
        const double rlo = r - rhi;
        const double rhi2 = rhi * rhi;
        const double hi = fsq_fma(rhi2, LOG_B[0], r);
        double lo = fsq_fma(rhi2, LOG_B[0], r - hi);
        lo = fsq_fma(LOG_B[0] * rlo, r + rhi, lo);
        const double y = fsq_fma(p, r3, lo);
        return hi + y;
    }
    if (top - 0x0010u >= 0x7ff0u - 0x0010u) {                    // x < 2^-1022, inf or nan
        if (ix * 2 == 0) return -__builtin_inf();
        if (ix == 0x7ff0000000000000ull) return x;
        if ((top & 0x8000u) || (top & 0x7ff0u) == 0x7ff0u) return __builtin_nan("");
        ix = fsq_bits(x * 0x1p52);                               // subnormal: normalise
        ix -= 52ull << 52;
    }
    const unsigned long long tmp = ix - 0x3fe6000000000000ull;
    const int i = (int)((tmp >> 45) & 127);
    const int k = (int)((long long)tmp >> 52);
    const unsigned long long iz = ix - (tmp & (0xfffull << 52));
    const double invc = FSQ_LOG_TAB[i][0], logc = FSQ_LOG_TAB[i][1];
    const double z = fsq_dbl(iz), kd = (double)k;
    const double r = fsq_fma(z, invc, -1.0);
    const double w = fsq_fma(kd, LOG_LN2HI, logc);
    const double hi = w + r;
    const double lo = fsq_fma(kd, LOG_LN2LO, (w - hi) + r);
    const double r2 = r * r;
    const double r3 = r * r2;
    const double p = fsq_fma(fsq_fma(r, LOG_A[4], LOG_A[3]), r2, fsq_fma(r, LOG_A[2], LOG_A[1]));
    const double y = fsq_fma(r3, p, fsq_fma(r2, LOG_A[0], lo));
    return y + hi;
}

}  // namespace
