// fsq_glibc_exp.h - exp(x) and pow's exp tail as glibc 2.35 computes them (e_exp.c, e_pow.c's exp_inline, FMA variant):
// fsq_exp_special / fsq_exp_core of fsq_devmath.h, force-inlined, since a kernel that makes no call needs no scratch frame.
// Include after ../fsq_devmath.h, which keeps its own copy for the fit engine: that file is part of the hashed kernel sources.
// (the "subnormal" cases of tests/golden/lognormal_tracks.npz pin the special-case tail)
#pragma once

namespace {

__device__ __forceinline__ double sf_exp_special(double tmp, unsigned long long sbits, unsigned long long ki)
{
    double scale, y;
    if ((ki & 0x80000000ull) == 0) {
        sbits -= 1009ull << 52;
        scale = fsq_dbl(sbits);
        return 0x1p1009 * fsq_fma(scale, tmp, scale);
    }
    sbits += 1022ull << 52;
    scale = fsq_dbl(sbits);
    y = scale + scale * tmp;
    if (y < 1.0) {
        double hi, lo;
        lo = scale - y + scale * tmp;
        hi = 1.0 + y;
        lo = 1.0 - hi + y + lo;
        y = (hi + lo) - 1.0;
        if (y == 0.0) y = 0.0;
    }
    return 0x1p-1022 * y;
}

// POW: exp(x + xtail) of pow, whose x is finite.  !POW: exp(x) of every double (xtail is not read).
template <bool POW>
__device__ __forceinline__ double sf_exp(double x, double xtail)
{
    unsigned abstop = (unsigned)(fsq_bits(x) >> 52) & 0x7ff;
    if (__builtin_expect(abstop - 0x3c9u >= 0x3fu, 0)) {
        if (abstop - 0x3c9u >= 0x80000000u) return 1.0 + x;
        if (abstop >= 0x409u) {
            if (!POW) {
                if (fsq_bits(x) == 0xfff0000000000000ull) return 0.0;
                if (abstop >= 0x7ffu) return 1.0 + x;
            }
            return (fsq_bits(x) >> 63) ? 0.0 : __builtin_inf();   // __math_uflow / __math_oflow values
        }
        abstop = 0;
    }
    double kd = fsq_fma(x, EXP_INVLN2N, EXP_SHIFT);
    unsigned long long ki = fsq_bits(kd);
    kd -= EXP_SHIFT;
    double r = fsq_fma(kd, EXP_NEGLN2HIN, x);
    r = fsq_fma(kd, EXP_NEGLN2LON, r);
    if (POW) r = xtail + r;
    unsigned idx = 2u * ((unsigned)ki & 127u);
    unsigned long long top = ki << 45;
    double tail = fsq_dbl(FSQ_EXP_TAB[idx]);
    unsigned long long sbits = FSQ_EXP_TAB[idx + 1] + top;
    double r2 = r * r;
    double p23 = fsq_fma(EXP_C3, r, EXP_C2);
    double p45 = fsq_fma(r, EXP_C5, EXP_C4);
    double t = r + tail;
    double tmp = fsq_fma(p23, r2, t);
    tmp = fsq_fma(r2 * r2, p45, tmp);
    if (__builtin_expect(abstop == 0, 0)) return sf_exp_special(tmp, sbits, ki);
    double scale = fsq_dbl(sbits);
    return fsq_fma(scale, tmp, scale);
}

}  // namespace
