// sqr_cdf of ttx_sample_sq_real.h, the cubic CDF of a cell that ttx_rosenblatt_sq_real evaluates, as a program of its own (also built
// with the address and undefined-behaviour sanitizers by tests/test_rosenblatt_cpu.py): the round trip through the inversion the
// sampler uses, on tests/sample_sq_real_main.cpp's grid of coefficients and at the edges.  Prints "bad cases worst" on its last line,
// worst = the largest miss in units of the bound.
//
// The condition is |sqr_cdf(q, sqr_invert(q, s')) - s'| <= 32 u qmax, qmax = max(q0, |qm|, q1), u = 2^-53.  sqr_cdf scales by the
// power of two sqr_invert scales by and evaluates the very Horner form sqr_invert iterates on, so in scaled numbers sqr_cdf(l) - s' is
// the inversion's own f at the l it returned before the one rounding of the subtraction: where the iteration ended on f = 0 the round
// trip is exact, elsewhere it is the residual tests/sample_sq_real_main.cpp bounds by 32 u qmax (its derivation counts the 28 u of the
// computed f against the exact cubic; here both sides are the computed one).  Scaling back by ldexp is exact, except below the
// normal range, where the result is rounded to the grid s' itself lies on.
#include <cmath>
#include <cstdio>
#include <random>
#include "ttx_sample_sq_real.h"

static const double U = 1.1102230246251565e-16, BOUND = 32.0;
static long long bad = 0, cases = 0;
static double worst = 0.0;

static double qmax(double q0, double qm, double q1)
{
    double M = q0 > q1 ? q0 : q1;
    return fabs(qm) > M ? fabs(qm) : M;
}
static void trip_case(double q0, double qm, double q1, double sp)
{
    const double l = sqr_invert(q0, qm, q1, sp), back = sqr_cdf(q0, qm, q1, l), M = qmax(q0, qm, q1);
    cases++;
    if (!(l >= 0.0 && l <= 1.0) || !(back >= 0.0)) { bad++; return; }
    const double r = (double)(fabsl((long double)back / M - (long double)sp / M) / (BOUND * U));     // in units of M: 1e300 does not overflow
    worst = r > worst ? r : worst;
    bad += !(r <= 1.0);
}
// l = 0 gives 0, l = 1 the whole cell, beyond either end the same; the value never leaves [0, Q(1)] by more than the bound
static void ends_case(double q0, double qm, double q1)
{
    const double Q1 = ((q0 + qm) + q1) / 3.0, M = qmax(q0, qm, q1);
    cases++;
    bad += sqr_cdf(q0, qm, q1, 0.0) != 0.0 || sqr_cdf(q0, qm, q1, -0.0) != 0.0 || sqr_cdf(q0, qm, q1, -1.0) != 0.0 || sqr_cdf(q0, qm, q1, -INFINITY) != 0.0;
    const double one = sqr_cdf(q0, qm, q1, 1.0);
    // the same three operations on scaled numbers; below the normal range each of Q1's own and the result round to the grid of 2^-1074
    bad += !(fabsl((long double)one / M - (long double)Q1 / M) <= 4.0 * U + 3.0 * 4.9406564584124654e-324 / M);
    bad += sqr_cdf(q0, qm, q1, 2.0) != one || sqr_cdf(q0, qm, q1, INFINITY) != one;
    for (int i = 1; i < 16; i++) {
        const double v = sqr_cdf(q0, qm, q1, i / 16.0);
        bad += !(v / M >= -BOUND * U && v / M <= Q1 / M + BOUND * U);
    }
}

int main()
{
    std::mt19937_64 rng(20222);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    // the sibling's grid: s0, s1 >= 0, c inside Cauchy-Schwarz, a defensive term that is often zero, s' across [0, Q(1)]; 1e-310 is
    // below the normal range
    const double scales[] = {1.0, 1e-300, 1e300, 3.7e-5, 2.9e11, 1e-310};
    for (int it = 0; it < 240000; it++) {
        const double sc = scales[it % 6];
        double s0 = uni(rng), s1 = uni(rng);
        if (it % 11 == 0) s0 = 0.0;
        if (it % 13 == 0) s1 = 0.0;
        if (it % 17 == 0) s1 = s0;
        if (it % 19 == 0) s1 = s0 * 1e-12;
        const double lim = sqrt(s0) * sqrt(s1);
        double c = (2.0 * uni(rng) - 1.0) * lim;
        if (it % 5 == 0) c = -lim;                                              // q touches zero inside the cell: qm = -sqrt(q0 q1)
        if (it % 7 == 0) c = lim;
        const double g = it % 2 ? 0.0 : uni(rng) * (it % 4 ? 1e-3 : 1.0);
        const double q0 = (s0 + g) * sc, qm = (c + g) * sc, q1 = (s1 + g) * sc, Q1 = ((q0 + qm) + q1) / 3.0;
        double v = uni(rng);
        if (it % 23 == 0) v = 0.0;
        if (it % 29 == 0) v = 1.0;
        if (it % 31 == 0) v = ldexp(v, -40);
        if (it % 37 == 0) v = 1.0 - ldexp(v, -40);
        if (!(fabs(qm) > 0.0 || q0 > 0.0 || q1 > 0.0)) { bad += sqr_cdf(q0, qm, q1, 0.5) != 0.0; cases++; continue; }
        trip_case(q0, qm, q1, v * Q1);
        if (it % 64 == 0) ends_case(q0, qm, q1);
    }
    // the exact touching zero at a representable point: q = (1 - 2 l)^2
    for (int it = 0; it <= 64; it++) trip_case(1.0, -1.0, 1.0, (1.0 / 3.0) * (it / 64.0));
    trip_case(4.0, -2.0, 1.0, 1.0); trip_case(4.0, -2.0, 1.0, 0.8888888888888888); trip_case(1.0, -2.0, 4.0, 0.1111111111111111);
    for (double e : {1.0, 1e-300, 1e300, 1e-310}) {
        trip_case(e, e, e, 0.0); trip_case(e, e, e, e); trip_case(e, e, e, 0.25 * e); trip_case(0.0, 0.0, e, e / 6.0); trip_case(e, 0.0, 0.0, e / 6.0);
        ends_case(e, e, e); ends_case(e, -e, e); ends_case(0.0, 0.0, e); ends_case(e, 0.0, 0.0);
    }
    // a constant density: the CDF is l itself
    for (int i = 0; i <= 16; i++) { bad += fabs(sqr_cdf(2.0, 2.0, 2.0, i / 16.0) - 2.0 * (i / 16.0)) > 8.0 * U; cases++; }
    // what is not a number ends as 0; an infinite coefficient too; no density, no mass
    const double nan = NAN, inf = INFINITY;
    const double evil[][4] = {{nan, 1, 1, 0.5}, {1, nan, 1, 0.5}, {1, 1, nan, 0.5}, {1, 1, 1, nan}, {inf, 1, 1, 0.5}, {1, inf, 1, 0.5}, {1, -inf, 1, 0.5},
                              {1, 1, inf, 0.5}, {0, 0, 0, 0}, {0, 0, 0, 1}, {nan, nan, nan, nan}, {-0.0, -0.0, -0.0, 0.5}};
    for (const auto &q : evil) { bad += sqr_cdf(q[0], q[1], q[2], q[3]) != 0.0; cases++; }
    printf("%lld %lld %.3f\n", bad, cases, worst);
    return bad ? 1 : 0;
}
