// fsq_evalguard.h - one range proof per model evaluation instead of three checks per pixel.
//
// The fast fit kernels evaluate E = exp(-(u^2 + v^2) / 2), u = nu / sigma_h, v = nv / sigma_w on the 25 pixels of a ROI
// with the hoisted-reciprocal quotient and the branch-free exp of fsq_devmath.h.  Those equal `/` and exp() bit for bit
// only inside operand ranges, which used to be checked on every pixel (exponent of nu and nv, |e| < 512).  All of them
// follow from the handful of per-fit scalars an evaluation starts from, so they are proved here once per evaluation:
//
//   nu = fl(rcx - xp), nv = fl(rcy - yp),  xp = fl(fl(x c) - fl(y s)), yp = fl(fl(x s) + fl(y c)),  x, y in {0 .. 4},
//   (c, s) the rotation, (rcx, rcy) the rotated centre, all in fp64, round to nearest.
//
// fsq_evalguard_ok(c, s, rcx, rcy, sigma_h, sigma_w) returns true only if
//   (a) each of c, s, rcx, rcy is exactly 0 or has magnitude >= 2^-400 (and is finite),
//   (b) |c|, |s| <= 1 and |rcx|, |rcy| <= 8,
//   (c) 0.75 <= |sigma| < 2^250 for both divisors.
// What follows from it, for every pixel:
//   1. Grid.  A double that is 0 or of magnitude >= 2^-400 is an integer multiple of 2^-452 (its ulp is >= 2^-452).  The
//      exact sum, difference or small-integer multiple of such multiples is again one, and rounding a multiple of 2^-452
//      to nearest gives a multiple of 2^-452 (below 2^-399 such a number has at most 53 significant bits and is exact;
//      above, the result's ulp is >= 2^-452).  So fl(x c), fl(y s), xp, yp, nu and nv are all multiples of 2^-452:
//      every NON-ZERO numerator has magnitude >= 2^-452, i.e. frexp exponent >= -451 > -FSQ_DIV_EN = -500.
//   2. Size.  |xp|, |yp| <= fl(4 + 4) = 8 and |rcx|, |rcy| <= 8 give |nu|, |nv| <= 16 < 2^100 (the old centre limit).
//   3. Quotients.  With 2^-452 <= |n| <= 16 and 0.75 <= |d| < 2^250 (inside FSQ_DIV_ED) the quotient is a normal number
//      (>= 2^-703), so v_div_scale would not rescale and the hoisted-reciprocal quotient equals n / d; for n = 0 it is a
//      zero (of either sign).
//   4. exp.  |u|, |v| <= 16 / 0.75 < 21.34, so u^2 + v^2 <= 910.3 with all roundings, and e = -(u^2 + v^2) / 2 lies in
//      [-455.2, 0]: inside (-512, 512), where the branch-free exp equals exp().
//   5. Finite.  (a)-(c) are false for NaN and infinity, so every operand above is finite.
// The perturbed evaluations of fdjac2 (centre + h, sigma + h, theta + h) are covered by calling the predicate on THEIR
// scalars - nothing is inferred from the unperturbed point.  Inside the fit's box (centre in [2, 3], sigma in
// [0.75, 2], theta in [0, 360] degrees) the predicate holds: |rcx|, |rcy| <= 6 + rounding, sin / cos of a double are 0
// or far above 2^-400 unless theta itself is a non-zero number below 2^-394 (such a fit takes the exact kernel), and
// fdjac2's sigma + h stays >= 0.75 because h = +eps |sigma| unless sigma > 2 - h.
//
// Plain C++ (bit patterns only) so that a host program can test the proof: tests/test_evalguard_host.py.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FSQ_EG_FN __host__ __device__ inline
#else
#define FSQ_EG_FN inline
#endif

#define FSQ_EG_MIN_EXP (-400)     // non-zero c, s, rcx, rcy: magnitude >= 2^FSQ_EG_MIN_EXP
#define FSQ_EG_MAX_CENTRE 8.0     // |rcx|, |rcy|
#define FSQ_EG_MIN_SIGMA 0.75     // = fsq_llim(4), fsq_llim(5) of fsq_lm_core.h (static_assert in kA_jacobian)
#define FSQ_EG_MAX_SIGMA 0x1p250  // (exclusive) FSQ_DIV_ED: frexp exponent <= 250

FSQ_EG_FN uint64_t fsq_eg_bits(double v)
{
    uint64_t u;
    memcpy(&u, &v, sizeof u);
    return u;
}

// v is exactly 0, or 2^FSQ_EG_MIN_EXP <= |v| <= limit (false for NaN and infinity)
FSQ_EG_FN bool fsq_eg_zero_or_within(double v, double limit)
{
    const uint64_t a = fsq_eg_bits(v) & 0x7fffffffffffffffull;                 // |v|
    const uint64_t lo = (uint64_t)(1023 + FSQ_EG_MIN_EXP) << 52;               // 2^-400
    return a == 0 || (a >= lo && a <= fsq_eg_bits(limit));                     // (|doubles| order like their bit patterns)
}

FSQ_EG_FN bool fsq_eg_sigma_ok(double sigma)
{
    const uint64_t a = fsq_eg_bits(sigma) & 0x7fffffffffffffffull;
    return a >= fsq_eg_bits(FSQ_EG_MIN_SIGMA) && a < fsq_eg_bits(FSQ_EG_MAX_SIGMA);
}

FSQ_EG_FN bool fsq_eg_rotation_ok(double c, double s) { return fsq_eg_zero_or_within(c, 1.0) && fsq_eg_zero_or_within(s, 1.0); }
FSQ_EG_FN bool fsq_eg_centre_ok(double rcx, double rcy)
{
    return fsq_eg_zero_or_within(rcx, FSQ_EG_MAX_CENTRE) && fsq_eg_zero_or_within(rcy, FSQ_EG_MAX_CENTRE);
}

FSQ_EG_FN bool fsq_evalguard_ok(double c, double s, double rcx, double rcy, double sigma_h, double sigma_w)
{
    return fsq_eg_rotation_ok(c, s) && fsq_eg_centre_ok(rcx, rcy) && fsq_eg_sigma_ok(sigma_h) && fsq_eg_sigma_ok(sigma_w);
}
