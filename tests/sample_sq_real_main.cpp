// The host-side part of ttx_sample_sq_real.h as a program of its own (also built with the address and undefined-behaviour sanitizers
// by tests/test_sample_sq_real_cpu.py): the mass matrix's bidiagonal Cholesky factor against M = U^T U, and the cubic inversion
// sqr_invert against the cubic itself in long double, on random inputs and at the edges.  Prints "bad factors inversions worst" on
// its last line, worst = the largest residual in units of the bound.
//
// The bound of the residual |Q(lambda) - sp|, relative to M = max(q0, |qm|, q1), with u = 2^-53 and to first order in u.  The
// scaling by a power of two is exact.  d1 = qm - q0: |d1| <= 2 M, error 2 M u.  d2 = (q0 - 2 qm) + q1: errors 3 M u + 4 M u.  d3 =
// d2 / 3: |d3| <= 4 M / 3, error 7 M u / 3 + 4 M u / 3 < 4 M u.  Horner at l in [0, 1]: l d3 (error < 4 M u + 4 M u / 3), + d1 (the
// sum is at most 10 M / 3: + 2 M u + 10 M u / 3, 10.7 M u so far), times l (+ 10 M u / 3: 14 M u), + q0 (at most 13 M / 3: + 13 M u / 3:
// 18.4 M u), times l (+ 13 M u / 3: 22.7 M u), - sp (at most 16 M / 3: 28 M u).  So the computed f differs from Q(l) - sp by at most
// 28 M u.  The iteration ends with f = 0 (residual <= 28 M u), with a Newton step below half a unit in the last place of l (|f| <=
// 2 u l q(l) <= 2 M u more), or on a bracket of neighbouring numbers around a sign change of the computed f (|Q(l) - sp| <= 2 u M + 28
// M u); the early returns 0 and 1 have residuals of at most 3 M u.  Where the 64 iterations run out, on the flat cubic of a touching
// zero, the residual is of third order in (2/3)^64.  BOUND = 32 M u covers all of them.  By the mean value theorem the residual is
// q(xi) times the distance to the root: where q is of the order of M this is the distance in u; where q touches zero the root itself
// is ill-conditioned and only the residual, the mass actually missed, means anything.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>
#include "ttx_sample_sq_real.h"

static const double U = 1.1102230246251565e-16, BOUND = 32.0;
static long long bad = 0, factors = 0, inversions = 0;
static double worst = 0.0;

static void factor_case(const std::vector<double> &t)
{
    const int n = (int)t.size();
    std::vector<double> dg(n, -7.0), sp(n, -7.0);
    sqr_mass_cholesky(t.data(), n, dg.data(), sp.data());
    factors++;
    if (n == 1) { bad += dg[0] != 1.0 || sp[0] != 0.0; return; }
    bad += sp[n - 1] != 0.0;
    for (int i = 0; i < n; i++) {
        const long double hl = i ? (long double)t[i] - t[i - 1] : 0.0L, hr = i + 1 < n ? (long double)t[i + 1] - t[i] : 0.0L;
        const long double diag = (hl + hr) / 3.0L, got = (long double)dg[i] * dg[i] + (i ? (long double)sp[i - 1] * sp[i - 1] : 0.0L);
        bad += !(dg[i] > 0.0) || !(fabsl(got - diag) <= 6.0L * U * diag);      // the subtraction, the root and the square; h and /3 once each
        if (i + 1 < n) bad += !(fabsl((long double)dg[i] * sp[i] - hr / 6.0L) <= 4.0L * U * hr / 6.0L);
    }
}

// the cubic in long double from the unscaled numbers, Bernstein form
static long double cubic(long double q0, long double qm, long double q1, long double l)
{
    const long double b1 = q0 / 3.0L, b2 = (q0 + qm) / 3.0L, b3 = (q0 + qm + q1) / 3.0L, m = 1.0L - l;
    return 3.0L * b1 * l * m * m + 3.0L * b2 * l * l * m + b3 * l * l * l;
}
static void invert_case(double q0, double qm, double q1, double sp)
{
    const double l = sqr_invert(q0, qm, q1, sp);
    inversions++;
    if (!(l >= 0.0 && l <= 1.0)) { bad++; return; }
    double M = q0 > q1 ? q0 : q1;
    M = fabs(qm) > M ? fabs(qm) : M;
    // in units of M, so that 1e300 does not overflow the cubic's sums
    const long double res = fabsl(cubic((long double)q0 / M, (long double)qm / M, (long double)q1 / M, l) - (long double)sp / M);
    const double r = (double)(res / (BOUND * U));
    worst = r > worst ? r : worst;
    bad += !(r <= 1.0);
}

int main()
{
    std::mt19937_64 rng(20222);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    // factors: random node rows, uniform rows, strongly graded rows, one and two nodes
    for (int it = 0; it < 2000; it++) {
        const int n = it < 2 ? 1 + it : 2 + (int)(rng() % (it % 50 == 0 ? 1100 : 40));
        std::vector<double> t(n);
        double x = -3.0 + uni(rng);
        for (int i = 0; i < n; i++) { t[i] = x; x += it % 3 == 0 ? 0.125 : it % 3 == 1 ? 1e-3 + uni(rng) : ldexp(1.0, -(int)(rng() % 30)); }
        factor_case(t);
    }
    // inversions: s0, s1 >= 0, c inside Cauchy-Schwarz, a defensive term that is often zero, sp across [0, Q(1)]
    const double scales[] = {1.0, 1e-300, 1e300, 3.7e-5, 2.9e11};
    for (int it = 0; it < 200000; it++) {
        const double sc = scales[it % 5];
        double s0 = uni(rng), s1 = uni(rng);
        if (it % 11 == 0) s0 = 0.0;
        if (it % 13 == 0) s1 = 0.0;
        if (it % 17 == 0) s1 = s0;
        if (it % 19 == 0) s1 = s0 * 1e-12;
        const double lim = sqrt(s0) * sqrt(s1);
        double c = (2.0 * uni(rng) - 1.0) * lim;
        if (it % 3 == 0) c = -lim;                                              // q touches zero inside the cell
        if (it % 7 == 0) c = lim;
        const double g = it % 2 ? 0.0 : uni(rng) * (it % 4 ? 1e-3 : 1.0);
        const double q0 = (s0 + g) * sc, qm = (c + g) * sc, q1 = (s1 + g) * sc, Q1 = ((q0 + qm) + q1) / 3.0;
        double v = uni(rng);
        if (it % 23 == 0) v = 0.0;
        if (it % 29 == 0) v = 1.0;
        if (it % 31 == 0) v = ldexp(v, -40);
        if (it % 37 == 0) v = 1.0 - ldexp(v, -40);
        if (!(fabs(qm) > 0.0 || q0 > 0.0 || q1 > 0.0)) { bad += sqr_invert(q0, qm, q1, 0.0) != 0.0; inversions++; continue; }
        invert_case(q0, qm, q1, v * Q1);
    }
    // the exact touching zero at a representable point: q = (1 - 2 l)^2 has q0 = 1, qm = -1, q1 = 1 and the triple point at l = 0.5
    for (int it = 0; it <= 64; it++) invert_case(1.0, -1.0, 1.0, (1.0 / 3.0) * (it / 64.0));
    invert_case(4.0, -2.0, 1.0, 1.0); invert_case(4.0, -2.0, 1.0, 0.8888888888888888); invert_case(1.0, -2.0, 4.0, 0.1111111111111111);
    for (double e : {1.0, 1e-300, 1e300}) { invert_case(e, e, e, 0.0); invert_case(e, e, e, e); invert_case(e, e, e, 0.25 * e); invert_case(0.0, 0.0, e, e / 6.0); invert_case(e, 0.0, 0.0, e / 6.0); }
    // what is not a number ends as 0; an infinite entry too
    const double nan = NAN, inf = INFINITY;
    const double evil[][4] = {{nan, 1, 1, 0.5}, {1, nan, 1, 0.5}, {1, 1, nan, 0.5}, {1, 1, 1, nan}, {inf, 1, 1, 0.5}, {1, inf, 1, 0.5}, {1, -inf, 1, 0.5},
                              {1, 1, inf, 0.5}, {0, 0, 0, 0}, {0, 0, 0, 1}, {1, 1, 1, -1.0}, {-0.0, -0.0, -0.0, 0.0}};
    for (const auto &q : evil) { bad += sqr_invert(q[0], q[1], q[2], q[3]) != 0.0; inversions++; }
    bad += sqr_invert(1.0, 1.0, 1.0, inf) != 1.0; inversions++;                 // a finite density and all the mass: the cell's end
    bad += sqr_invert(1.0, 1.0, 1.0, 2.0) != 1.0; inversions++;
    printf("%lld %lld %lld %.3f\n", bad, factors, inversions, worst);
    return bad ? 1 : 0;
}
