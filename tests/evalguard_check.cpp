// Host check of csrc/fsq_evalguard.h (built and run by tests/test_evalguard_host.py): whenever the per-evaluation range
// predicate accepts the scalars of a Jacobian round, every condition the fit kernels used to check on each pixel holds for
// all 25 pixels of all six evaluations of that round (base point = the step round's trial point, the two perturbed
// centres, the two perturbed sigmas, the perturbed rotation), and the facts the unfixed quotient relies on hold too.
// It also counts the tuples INSIDE the fit's box that the predicate rejects (must be 0: no legitimate fit may be sent to
// the exact path by it), and confirms on the real sin / cos that the box's rotations are 0 or at least the guard's 2^-400.
// The same real sin / cos, with centres and sigmas on and inside the box's bounds, also go through the predicate as a whole
// round (trig_rejected, must be 0).  No x0 / x1 / pixel draws: they matter only to the quotient loop of fdjac2, whose
// tracking was not hoisted and is still checked per numerator by the kernel.
// usage: evalguard_check [tuples = 10000000]     prints "tuples=.. accepted=.. inbox=.. bad=.. inbox_rejected=.. trig_bad=.. trig_rounds=.. trig_rejected=.."
// Compile with -ffp-contract=off (the kernels are): every product below is rounded before it is added.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>
#include <vector>

#include "../fluorosequencingimageanalysis_amd/csrc/fsq_evalguard.h"

namespace {

struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    double unit() { return (double)(next() >> 11) * 0x1p-53; }                 // [0, 1)
    double range(double a, double b) { return a + (b - a) * unit(); }
    int below(int n) { return (int)(next() % (uint64_t)n); }
    double sign() { return (next() & 1) ? 1.0 : -1.0; }
};

double from_bits(uint64_t u) { double v; memcpy(&v, &u, sizeof v); return v; }
double ulps(double v, int k) { return from_bits(fsq_eg_bits(v) + (uint64_t)(int64_t)k); }     // (v > 0)

// one of c, s: [-1, 1] drawn as a double, not through sin - with the values a proof has to survive
double draw_trig(Rng& r)
{
    switch (r.below(12)) {
    case 0: return r.below(2) ? 0.0 : -0.0;
    case 1: return r.sign();
    case 2: return r.sign() * from_bits(r.next() & 0xfffffffffffffull);        // subnormal (or 0)
    case 3: return r.sign() * ldexp(1.0 + r.unit(), -1000 + r.below(621));     // 2^-1000 .. 2^-380
    case 4: return r.sign() * ulps(0x1p-400, r.below(3) - 1);                  // one ulp either side of the guard's floor
    case 5: return r.sign() * ulps(1.0, r.below(3) - 1);                       // ... and of its ceiling
    case 6: return r.sign() * ldexp(1.0 + r.unit(), -r.below(80));             // log-uniform down to 2^-80
    case 7: return r.below(2) ? NAN : r.sign() * INFINITY;
    default: return r.range(-1.0, 1.0);
    }
}

double draw_centre(Rng& r)
{
    switch (r.below(12)) {
    case 0: return 2.0;
    case 1: return 3.0;
    case 2: return r.sign() * ulps(8.0, r.below(3) - 1);                       // (with c = 1, s = 0 this IS the rotated centre)
    case 3: return r.sign() * ldexp(1.0 + r.unit(), -1080 + r.below(1300));    // anything from subnormal-adjacent to 2^220
    case 4: return r.sign() * ulps(0x1p-400, r.below(3) - 1);
    case 5: return r.below(3) == 0 ? NAN : r.below(2) ? INFINITY : 0.0;
    case 6: return r.range(-10.0, 10.0);
    default: return r.range(2.0, 3.0);
    }
}

double draw_sigma(Rng& r)
{
    switch (r.below(12)) {
    case 0: return ulps(0.75, r.below(3) - 1);
    case 1: return 2.0;
    case 2: return ulps(2.0, r.below(3) - 1);
    case 3: return r.sign() * ldexp(1.0 + r.unit(), -1080 + r.below(2100));
    case 4: return ulps(0x1p250, r.below(3) - 1);
    case 5: return r.below(3) == 0 ? NAN : r.below(2) ? INFINITY : 0.0;
    case 6: return r.range(-3.0, 3.0);
    default: return r.range(0.75, 2.0);
    }
}

// fdjac2's step (mpfit.py:1582-1587) for a parameter with upper limit ul
double step(double x, double ul)
{
    const double eps = 1.4901161193847656e-08;
    double h = eps * fabs(x);
    if (h == 0) h = eps;
    if (x > ul - h) h = -h;
    return h;
}

// v_frexp_exp_i32_f64: exponent e of v = m 2^e, 0.5 <= |m| < 1; 0 for zero, infinity and NaN
int expo(double v)
{
    if (v == 0 || !isfinite(v)) return 0;
    int e;
    frexp(v, &e);
    return e;
}
bool divisor_in_range(double d) { return (unsigned)(expo(d) + 250) <= 500u; }

// what the kernels checked on every pixel of one evaluation, plus what the unfixed quotient needs; false = a violation
bool pixels_ok(double c, double s, double rcx, double rcy, double sh, double sw)
{
    if (!divisor_in_range(sh) || !divisor_in_range(sw)) return false;          // (checked per fit then and now)
    for (int xi = 0; xi < 5; xi++)
        for (int yi = 0; yi < 5; yi++) {
            const double x = xi, y = yi;
            const double xc = x * c, ys = y * s, xs = x * s, yc = y * c;
            const double xp = xc - ys, yp = xs + yc;
            const double nu = rcx - xp, nv = rcy - yp;
            if (!isfinite(nu) || !isfinite(nv)) return false;
            if (expo(nu) < -500 || expo(nv) < -500) return false;              // em = min(em, fsq_expo(n)); em < -FSQ_DIV_EN
            if (!(fabs(nu) <= 0x1p102) || !(fabs(nv) <= 0x1p102)) return false;      // (what the 2^100 centre limit stood for)
            const double u = nu / sh, v = nv / sw;
            if ((u != 0 && fabs(u) < 0x1p-1022) || (v != 0 && fabs(v) < 0x1p-1022)) return false;    // quotient normal or zero
            const double uu = u * u, vv = v * v;
            const double e = -(uu + vv) / 2.;
            if (!(fabs(e) < 512.0)) return false;                              // fsq_exp_bf's flag
        }
    return true;
}

struct Tally { long long accepted = 0, inbox = 0, bad = 0, inbox_rejected = 0; };

void run_chunk(uint64_t seed, long long n, Tally* t)
{
    Rng r{seed};
    for (long long i = 0; i < n; i++) {
        double c, s, ct, st, x2, x3, s4, s5;
        const bool all_in_box = r.below(4) == 0;        // a quarter of the tuples lie wholly inside the box
        if (all_in_box) {
            // rotations as the box can produce them: 0, +-1, anything in between down to 2^-399 (see check_trig)
            auto t1 = [&]() { const int k = r.below(6); return k == 0 ? 0.0 : k == 1 ? r.sign() : k == 2 ? r.sign() * ldexp(1.0 + r.unit(), -1 - r.below(399)) : r.range(-1.0, 1.0); };
            c = t1(); s = t1(); ct = t1(); st = t1();
            auto b = [&](double lo, double hi) { const int k = r.below(5); return k == 0 ? lo : k == 1 ? hi : r.range(lo, hi); };
            x2 = b(2.0, 3.0); x3 = b(2.0, 3.0); s4 = b(0.75, 2.0); s5 = b(0.75, 2.0);
        } else {
            c = draw_trig(r); s = draw_trig(r);
            if (r.below(2)) { ct = draw_trig(r); st = draw_trig(r); } else { ct = c + r.range(-1e-7, 1e-7); st = s + r.range(-1e-7, 1e-7); }
            x2 = draw_centre(r); x3 = draw_centre(r); s4 = draw_sigma(r); s5 = draw_sigma(r);
        }
        // the scalars of the round, formed as kA_jacobian forms them
        const double x2p = x2 + step(x2, 3.0), x3p = x3 + step(x3, 3.0), s4p = s4 + step(s4, 2.0), s5p = s5 + step(s5, 2.0);
        const double rcx = x3 * c - x2 * s, rcy = x3 * s + x2 * c;
        const double rcx2 = x3 * c - x2p * s, rcy2 = x3 * s + x2p * c;
        const double rcx3 = x3p * c - x2 * s, rcy3 = x3p * s + x2 * c;
        const double rcxt = x3 * ct - x2 * st, rcyt = x3 * st + x2 * ct;
        // ... and the predicate, called as kA_jacobian calls it (kB_step's trial point is the first call alone)
        const bool ok = fsq_evalguard_ok(c, s, rcx, rcy, s4, s5) && fsq_eg_centre_ok(rcx2, rcy2) && fsq_eg_centre_ok(rcx3, rcy3) &&
                        fsq_eg_sigma_ok(s4p) && fsq_eg_sigma_ok(s5p) && fsq_eg_rotation_ok(ct, st) && fsq_eg_centre_ok(rcxt, rcyt);
        if (all_in_box) { t->inbox++; if (!ok) t->inbox_rejected++; }
        if (!ok) continue;
        t->accepted++;
        const bool fine = pixels_ok(c, s, rcx, rcy, s4, s5) && pixels_ok(c, s, rcx2, rcy2, s4, s5) && pixels_ok(c, s, rcx3, rcy3, s4, s5) &&
                          pixels_ok(c, s, rcx, rcy, s4p, s5) && pixels_ok(c, s, rcx, rcy, s4, s5p) && pixels_ok(ct, st, rcxt, rcyt, s4, s5);
        if (!fine) t->bad++;
    }
}

// sin / cos of theta pi / 180 around the multiples of 90 degrees and at the small end of the box: 0 or >= 2^-400 in magnitude unless
// theta is itself a non-zero number below 2^-394 (which no fit reaches: such a fit would only take the exact path)
long long g_trig_rounds = 0, g_trig_rejected = 0;

// a whole round at angle th (degrees, as the kernel forms it) with box centres and sigmas: predicate as kA_jacobian calls it
void trig_round(double th, double x2, double x3, double s4, double s5)
{
    const double pi180 = 0.017453292519943295;
    const double c = cos(pi180 * th), s = sin(pi180 * th);
    const double tht = th + step(th, 360.0), ct = cos(pi180 * tht), st = sin(pi180 * tht);
    const double x2p = x2 + step(x2, 3.0), x3p = x3 + step(x3, 3.0), s4p = s4 + step(s4, 2.0), s5p = s5 + step(s5, 2.0);
    const double rcx = x3 * c - x2 * s, rcy = x3 * s + x2 * c;
    const double rcx2 = x3 * c - x2p * s, rcy2 = x3 * s + x2p * c;
    const double rcx3 = x3p * c - x2 * s, rcy3 = x3p * s + x2 * c;
    const double rcxt = x3 * ct - x2 * st, rcyt = x3 * st + x2 * ct;
    const bool ok = fsq_evalguard_ok(c, s, rcx, rcy, s4, s5) && fsq_eg_centre_ok(rcx2, rcy2) && fsq_eg_centre_ok(rcx3, rcy3) &&
                    fsq_eg_sigma_ok(s4p) && fsq_eg_sigma_ok(s5p) && fsq_eg_rotation_ok(ct, st) && fsq_eg_centre_ok(rcxt, rcyt);
    g_trig_rounds++;
    if (!ok) g_trig_rejected++;
}

long long check_trig()
{
    long long bad = 0;
    const double pi180 = 0.017453292519943295;
    auto one = [&](double th) {
        if (!(th >= 0.0 && th <= 360.0)) return;
        const double a = pi180 * th, v[2] = {sin(a), cos(a)};
        for (double w : v) if (w != 0 && fabs(w) < 0x1p-400 && !(th != 0 && th < 0x1p-394)) bad++;
        if (th == 0 || th >= 0x1p-393) {            // (the perturbed angle th (1 + eps) is then >= 2^-394 too)
            const double lim[3] = {2.0, 2.5, 3.0}, sg[3] = {0.75, 1.3, 2.0};
            const int k = (int)(g_trig_rounds % 9);
            trig_round(th, lim[k % 3], lim[k / 3], sg[(k + 1) % 3], sg[(k / 3 + 2) % 3]);
            trig_round(th, 3.0, 3.0, 0.75, 0.75);
            trig_round(th, 2.0, 3.0, 2.0, 0.75);
        }
    };
    for (int q = 0; q <= 4; q++)
        for (int k = -20000; k <= 20000; k++) one(q == 0 ? from_bits((uint64_t)(k + 20000)) : ulps(90.0 * q, k));
    for (int e = -1074; e <= 8; e++) { one(ldexp(1.0, e)); one(ldexp(1.5, e)); }
    return bad;
}

}  // namespace

int main(int argc, char** argv)
{
    const long long total = argc > 1 ? atoll(argv[1]) : 10000000ll;
    const int chunks = 64;                      // fixed, so that the draw does not depend on the number of threads
    std::vector<Tally> tally(chunks);
    std::atomic<int> next{0};
    unsigned nt = std::thread::hardware_concurrency();
    nt = nt == 0 ? 1 : nt > 8 ? 8 : nt;
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < nt; t++)
        pool.emplace_back([&]() {
            for (int k; (k = next.fetch_add(1)) < chunks;)
                run_chunk(0x5eedull + 1000003ull * (uint64_t)k, total / chunks + (k < total % chunks ? 1 : 0), &tally[k]);
        });
    for (auto& th : pool) th.join();
    Tally sum;
    for (const Tally& t : tally) { sum.accepted += t.accepted; sum.inbox += t.inbox; sum.bad += t.bad; sum.inbox_rejected += t.inbox_rejected; }
    const long long trig_bad = check_trig();
    printf("tuples=%lld accepted=%lld inbox=%lld bad=%lld inbox_rejected=%lld trig_bad=%lld trig_rounds=%lld trig_rejected=%lld\n", total,
           sum.accepted, sum.inbox, sum.bad, sum.inbox_rejected, trig_bad, g_trig_rounds, g_trig_rejected);
    return 0;
}
