// Stand-alone host program for the host-callable part of ttcross_amd/csrc/ttx_sample_real.h: sr_invert, sr_trapezoid, sr_hat_cell, sr_held_mode.
// Prints "bad ninvert nchecks" on its last line; bad = 0 when every check held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>
#include "ttx_sample_real.h"

static int bad = 0, nchk = 0, ninv = 0;
#define CHECK(c, ...) do { nchk++; if (!(c)) { bad++; printf(__VA_ARGS__); printf("\n"); } } while (0)

static double ulp(double m) { return std::nextafter(m, std::numeric_limits<double>::infinity()) - m; }

// lambda in [0, 1], and p0 l + D l^2 / 2 returns sp within 4 ulp of max(p0, p1) (the residual in long double)
static void invert_case(double p0, double p1, double sp)
{
    const double l = sr_invert(p0, p1, sp);
    ninv++;
    CHECK(l >= 0.0 && l <= 1.0, "lambda %.17g out of [0, 1] at p0 %.17g p1 %.17g sp %.17g", l, p0, p1, sp);
    const double m = p0 > p1 ? p0 : p1;
    if (!(m > 0.0)) { CHECK(l == 0.0, "lambda %.17g for a cell without density", l); return; }
    const long double L = l, res = (long double)p0 * L + ((long double)p1 - (long double)p0) * L * L / 2.0L - (long double)sp;
    CHECK(fabsl(res) <= 4.0L * (long double)ulp(m), "residual %.3Le > 4 ulp (%.3e) at p0 %.17g p1 %.17g sp %.17g lambda %.17g", res, 4.0 * ulp(m), p0, p1, sp, l);
}

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static double rnd()                           // splitmix64 -> [0, 1)
{
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-53;
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity(), den = 4.9406564584124654e-324;
    // the named cases, each at s' = 0, the middle, just below the full mass and the full mass (p0 + p1) / 2
    const double pairs[][2] = {{0.0, 1.0}, {1.0, 0.0}, {0.7, 0.7}, {0.3, 0.9}, {0.9, 0.3}, {1e-300, 1e-300}, {1e-300, 3e-300}, {3e-300, 0.0}, {0.0, 1e-300},
                               {1e300, 1e300}, {1e300, 0.0}, {0.0, 1e300}, {1e-310, 1e-310}, {3e-320, 1e-320}, {0.0, 64 * den}, {64 * den, 0.0}, {1024 * den, 1024 * den},
                               {1.0, 1e-17}, {1e-17, 1.0}, {1.0, 1.0 + 0x1.0p-52}, {0.0, 0.0}};
    for (const auto &pp : pairs) {
        const double full = 0.5 * pp[0] + 0.5 * pp[1];
        for (double f : {0.0, 0x1.0p-60, 1e-9, 0.25, 0.5, 0.75, 1.0 - 0x1.0p-53, 1.0}) invert_case(pp[0], pp[1], f * full);
    }
    // subnormal masses under ordinary densities
    for (double sp : {den, 3 * den, 1e-310}) { invert_case(1.0, 2.0, sp); invert_case(0.0, 1.0, sp); invert_case(1e-300, 0.0, sp > 0.5e-300 ? 0.5e-300 : sp); }
    // a seeded sweep over magnitudes
    for (int t = 0; t < 200000; t++) {
        const double sc = std::ldexp(1.0, (int)(rnd() * 1800.0) - 900), p0 = rnd() < 0.1 ? 0.0 : sc * rnd(), p1 = rnd() < 0.1 ? 0.0 : sc * rnd() * std::ldexp(1.0, (int)(rnd() * 8.0) - 4);
        invert_case(p0, p1, rnd() * (0.5 * p0 + 0.5 * p1));
    }
    // what is not a number gives 0 or NaN, never an out-of-range value; so does an sp outside the cell
    const double vals[] = {nan, inf, -inf, -1.0, 0.0, 1.0, 1e-300, 1e300};
    for (double a : vals) for (double b : vals) for (double c : vals) {
        const double l = sr_invert(a, b, c);
        CHECK(l != l || (l >= 0.0 && l <= 1.0), "sr_invert(%g, %g, %g) = %g", a, b, c, l);
    }
    // trapezoid weights: the sum is t(n-1) - t(0) (to n roundings of the larger node), the ends are half cells, one node carries 1.0
    for (int n : {2, 3, 5, 64, 65, 1025}) {
        std::vector<double> t(n), om(n);
        double x = -1.5;
        for (int i = 0; i < n; i++) { x += 0.01 + rnd(); t[i] = x; }
        sr_trapezoid(t.data(), n, om.data());
        long double s = 0.0L;
        for (int i = 0; i < n; i++) { s += om[i]; CHECK(om[i] > 0.0, "weight %d of %d is %g", i, n, om[i]); }
        CHECK(fabsl(s - ((long double)t[n - 1] - t[0])) <= (long double)n * ulp(fabs(t[n - 1]) + fabs(t[0])), "trapezoid weights of %d nodes sum to %.17Lg, not %.17g", n, s, t[n - 1] - t[0]);
        CHECK(om[0] == 0.5 * (t[1] - t[0]) && om[n - 1] == 0.5 * (t[n - 1] - t[n - 2]), "end weights of %d nodes", n);
        // the hat cell: inside 0 .. n-2 for every coordinate, the last node with t_i <= x between the ends
        for (double q : {-inf, -1e300, t[0], std::nextafter(t[0], inf), t[n / 2], std::nextafter(t[n / 2], -inf), t[n - 1], std::nextafter(t[n - 1], -inf), 1e300, inf, nan}) {
            const int i = sr_hat_cell(t.data(), n, q);
            CHECK(i >= 0 && i <= n - 2, "hat cell %d of %d nodes at %g", i, n, q);
            if (q > t[0] && q < t[n - 1]) CHECK(t[i] <= q && q < t[i + 1], "hat cell %d does not contain %.17g", i, q);
        }
        for (int i = 0; i < n - 1; i++) {
            CHECK(sr_hat_cell(t.data(), n, t[i]) == i, "hat cell of node %d", i);
            CHECK(sr_hat_cell(t.data(), n, 0.5 * t[i] + 0.5 * t[i + 1]) == i, "hat cell of the middle of cell %d", i);
        }
    }
    double one = 3.25, w1 = 0.0;
    sr_trapezoid(&one, 1, &w1);
    CHECK(w1 == 1.0 && sr_hat_cell(&one, 1, 7.0) == 0 && sr_hat_cell(&one, 1, nan) == 0, "a mode of one node");
    // the record of a held mode: sr_hat_cell's cell and ttx_basis_entry's two hat values there, every other entry of the row 0 and the row summing to 1;
    // a coordinate below the first node, above the last, on a node (an inner one, the first, the last), inside a cell
    for (int n : {2, 3, 17, 66}) {
        std::vector<double> t(n);
        double x = -2.25;
        for (int i = 0; i < n; i++) { x += 0.01 + rnd(); t[i] = x; }
        for (double q : {t[0] - 1.0, -1e300, t[n - 1] + 0.5, 1e300, t[n / 2], t[0], t[n - 1], 0.25 * t[n / 2 - 1] + 0.75 * t[n / 2], std::nextafter(t[n - 1], -inf)}) {
            const SrMode M = sr_held_mode(t.data(), n, q, 40 + (size_t)n);
            CHECK(M.held == 1 && M.xh == q && M.noff == 40 + (size_t)n, "held mode of %d nodes at %.17g: held %d xh %.17g noff %zu", n, q, M.held, M.xh, M.noff);
            CHECK(M.cell == sr_hat_cell(t.data(), n, q) && M.cell >= 0 && M.cell <= n - 2, "held mode of %d nodes at %.17g: cell %d", n, q, M.cell);
            CHECK(M.phi0 == ttx_basis_entry(2, 0, 0.0, 0.0, t.data(), n, q, M.cell) && M.phi1 == ttx_basis_entry(2, 0, 0.0, 0.0, t.data(), n, q, M.cell + 1),
                  "held mode of %d nodes at %.17g: hat values %.17g %.17g", n, q, M.phi0, M.phi1);
            for (int j = 0; j < n; j++)
                if (j != M.cell && j != M.cell + 1) CHECK(ttx_basis_entry(2, 0, 0.0, 0.0, t.data(), n, q, j) == 0.0, "held mode of %d nodes at %.17g: entry %d outside the cell", n, q, j);
            CHECK(M.phi0 >= 0.0 && M.phi1 >= 0.0 && fabs(M.phi0 + M.phi1 - 1.0) <= 0x1.0p-52, "held mode of %d nodes at %.17g: %.17g + %.17g", n, q, M.phi0, M.phi1);
        }
    }
    const SrMode M1 = sr_held_mode(&one, 1, 7.0, 3);
    CHECK(M1.held == 1 && M1.cell == 0 && M1.phi0 == 1.0 && M1.phi1 == 0.0 && M1.xh == 7.0 && M1.noff == 3, "the held record of a mode of one node");
    CHECK(M1.phi0 == ttx_basis_entry(2, 0, 0.0, 0.0, &one, 1, 7.0, 0), "a mode of one node: the entry");
    printf("%d %d %d\n", bad, ninv, nchk);
    return bad != 0;
}
