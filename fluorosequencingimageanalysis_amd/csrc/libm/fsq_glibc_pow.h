// fsq_glibc_pow.h - pow(x, 2.0) and pow(x, -2.0) as glibc 2.35 computes them (e_pow.c, FMA variant), shared by the
// step-fit kernels (fsq_stepfit.hip, fsq_chisq.hip) and the bin search (fsq_binsearch.hip).  Include after ../fsq_devmath.h.
// fsq_devmath.h keeps its own fsq_pow2 for the fit engine and consolidation: that file is part of the hashed kernel sources.
#pragma once

#include "fsq_glibc_exp.h"

namespace {

// pow(x, Y) for Y = 2 or -2.  Negative bases drop their sign (Y is even); 0 / inf / nan give x * x for Y = 2 and
// +inf (__math_divzero) or 1 / (x * x) for Y = -2; tiny results go through exp's specialcase.  INLINE_EXP chooses the
// force-inlined exp of fsq_glibc_exp.h over fsq_devmath.h's fsq_exp_core<true>, which calls fsq_exp_special.
template <int Y, bool INLINE_EXP>
__device__ __forceinline__ double sf_pow(double x)
{
    static_assert(Y == 2 || Y == -2, "the even powers the step-fit reference takes");
    unsigned long long ix = fsq_bits(x);
    unsigned topx = (unsigned)(ix >> 52);
    if (topx - 1u >= 0x7ffu - 1u) {
        if (2 * ix - 1 >= 2 * 0x7ff0000000000000ull - 1) {            // 0, inf, nan
            const double x2 = x * x;
            if (Y > 0) return x2;
            if (2 * ix == 0) return __builtin_inf();
            return 1.0 / x2;                                           // inf -> 0, nan -> nan
        }
        ix &= 0x7fffffffffffffffull;
        topx &= 0x7ff;
        if (topx == 0) {                                               // subnormal x: normalise
            ix = fsq_bits(fsq_dbl(ix) * 0x1p52);
            ix &= 0x7fffffffffffffffull;
            ix -= 52ull << 52;
        }
    }
    unsigned long long tmp = ix - 0x3fe6955500000000ull;
    int i = (int)((tmp >> 45) & 127);
    int k = (int)((long long)tmp >> 52);
    unsigned long long iz = ix - (tmp & (0xfffull << 52));
    double z = fsq_dbl(iz), kd = (double)k;
    double invc = FSQ_POW_LOG_TAB[i][0], logc = FSQ_POW_LOG_TAB[i][1], logctail = FSQ_POW_LOG_TAB[i][2];
    double r = fsq_fma(z, invc, -1.0);
    double t1 = fsq_fma(kd, POW_LN2HI, logc);
    double t2 = t1 + r;
    double lo1 = fsq_fma(kd, POW_LN2LO, logctail);
    double lo2 = t1 - t2 + r;
    double ar = POW_A[0] * r;
    double ar2 = r * ar;
    double ar3 = r * ar2;
    double hi = t2 + ar2;
    double lo3 = fsq_fma(ar, r, -ar2);
    double lo4 = t2 - hi + ar2;
    double p12 = fsq_fma(POW_A[2], r, POW_A[1]);
    double p34 = fsq_fma(POW_A[4], r, POW_A[3]);
    double p56 = fsq_fma(r, POW_A[6], POW_A[5]);
    double q = fsq_fma(p56, ar2, p34);
    q = fsq_fma(ar2, q, p12);
    double lo = ((lo1 + lo2) + lo3) + lo4;
    lo = fsq_fma(ar3, q, lo);
    double y = hi + lo;
    double tail = hi - y + lo;
    const double Yd = (double)Y;
    double ehi = Yd * y;                                               // y * hi, y * lo + fma(y, hi, -ehi) of e_pow.c
    double elo = fsq_fma(Yd, tail, fsq_fma(y, Yd, -ehi));
    return INLINE_EXP ? sf_exp<true>(ehi, elo) : fsq_exp_core<true>(ehi, elo);
}

}  // namespace
