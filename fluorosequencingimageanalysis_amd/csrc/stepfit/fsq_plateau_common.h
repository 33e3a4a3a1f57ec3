// fsq_plateau_common.h - what the kernels that take caller-given plateau tables share (fsq_chisq.hip, fsq_timetrace.hip):
// glibc's pow(x, 2.0) without a call, the reference machine's NaN, the plateau-table check and the ordered residual sum.
#pragma once
#include "../fsq_devmath.h"
#include "../../../include/fsq_stepfit.h"
#include "../libm/fsq_glibc_pow.h"

namespace {

// pow(x, 2.0) as glibc, with the exp tail inlined so that the kernels make no call (a call costs a scratch frame)
__device__ __forceinline__ double cs_pow2(double x) { return sf_pow<2, true>(x); }

// No input is a NaN, so a NaN result is one an invalid operation made (0 / 0 for R^2 of a flat trace, inf / inf).  The
// reference ran on x86-64, whose default NaN has the sign bit set; the GPU's has not.  Results are compared bit for bit.
__device__ __forceinline__ double x86_nan(double v) { return v != v ? fsq_dbl(0xfff8000000000000ull) : v; }

// valid: 1 <= cnt <= n <= max_frames, 0 <= start_0, stop_i + 1 == start_{i+1}, start_i <= stop_i, stop_last < n
__device__ __forceinline__ bool plateaus_valid(int n, int max_frames, int cnt, const int32_t* st, const int32_t* so)
{
    bool ok = n >= 1 && n <= max_frames && n <= FSQ_STEPFIT_MAX_MIRRORED && cnt >= 1 && cnt <= n && st[0] >= 0;
    for (int i = 0; ok && i < cnt; i++) {
        ok = st[i] <= so[i] && so[i] < n;
        if (ok && i + 1 < cnt) ok = so[i] + 1 == st[i + 1];
    }
    return ok;
}

// _plateau_squared_residuals for lum[a..b] around h
__device__ __forceinline__ double seq_residual(const double* lum, int a, int b, double h)
{
    double r = 0.0;
    for (int f = a; f <= b; f++) r += cs_pow2(lum[f] - h);
    return r;
}

}  // namespace
