// check_log_host.cpp - csrc/libm/fsq_glibc_log.h compiled for the host, against this machine's log(): the restatement
// holds only plain IEEE fp64 operations and explicit fmas, so the host build computes what the device computes.
//
//   g++ -O2 -mfma -ffp-contract=off -o check_log_host tools/check_log_host.cpp && ./check_log_host [N]
//
// Compares bit for bit on N (default 20 000 000) random bit patterns, N arguments within 2^-3 of 1, the integers below
// N / 4, N / 4 subnormals and the special values; prints the number of differences and exits with 1 if there are any.
// Equal on glibc 2.35 (x86-64, a CPU with FMA and AVX2: the variant fsq_glibc_log.h follows).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#define __device__
#define __forceinline__ inline
static inline unsigned long long fsq_bits(double x) { unsigned long long u; memcpy(&u, &x, 8); return u; }
static inline double fsq_dbl(unsigned long long u) { double x; memcpy(&x, &u, 8); return x; }
static inline double fsq_fma(double a, double b, double c) { return __builtin_fma(a, b, c); }
#include "../fluorosequencingimageanalysis_amd/csrc/libm/fsq_glibc_log.h"

int main(int argc, char** argv)
{
    const long n = argc > 1 ? atol(argv[1]) : 20000000;
    std::mt19937_64 g(1);
    long bad = 0, total = 0;
    auto chk = [&](double x) {
        const double a = ln_log(x), b = log(x);
        ++total;
        if (fsq_bits(a) != fsq_bits(b) && !(a != a && b != b)) {
            if (bad < 5) printf("x = %a: got %a, libm %a\n", x, a, b);
            ++bad;
        }
    };
    for (long i = 0; i < n; ++i) chk(fsq_dbl(g()));
    for (long i = 0; i < n; ++i) chk(1.0 + (double)(int64_t)g() * 0x1p-63 * 0x1p-3);
    for (long i = 1; i < n / 4; ++i) chk((double)i);
    for (long i = 0; i < n / 4; ++i) chk(fsq_dbl(g() & 0x000fffffffffffffull));
    const double special[] = {0.0, -0.0, INFINITY, -INFINITY, NAN, 1.0, -1.0, 0x1p-1074, 1.7976931348623157e308};
    for (double x : special) chk(x);
    printf("%ld arguments, %ld differences\n", total, bad);
    return bad != 0;
}
