// Host check of cl_ordered_sum (ttcross_amd/csrc/ttx_cluster_rules.h), the ordered residual sum of the cluster sweep kernel:
// for every length n = 0 .. 70 and both batch sizes the helper asks its loader for exactly n operands, hands operand s to
// term s, and visits s = 0 .. n-1 in ascending order -- so a functor that accumulates performs the plain loop's operations in
// its order.  The same on doubles: sums over data with infinities, zeros of both signs and huge / tiny magnitudes equal the
// plain loop bit for bit (-ffp-contract=off as in the library's build).  Prints "<bad> <checks>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "ttx_cluster_rules.h"

static long bad = 0, nchk = 0;
static void check(bool ok) { nchk++; if (!ok) bad++; }
static uint64_t bits(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }

template <int B>
static void order(int n)
{
    int loads = 0, next = 0;
    bool ok = true;
    cl_ordered_sum<B>(n, [&] { return loads++; }, [&](int s, int v) { ok = ok && s == next && v == s; next++; });
    check(ok); check(loads == n); check(next == n);
}

template <int B>
static void sums(int n, const std::vector<double> &c, const std::vector<double> &w, const std::vector<double> &x)
{
    struct D2 { double a, b; };
    double b0 = 0.75, t0 = 0.0, l0 = 0.0;                       // the plain loops of the column, row and lottery residuals
    for (int s = 0; s < n; s++) { b0 = b0 + (-x[s]) * c[s]; t0 = t0 + w[s] * x[s]; l0 = l0 + c[s] * w[s]; }
    double b1 = 0.75, t1 = 0.0, l1 = 0.0;
    const double *pc = c.data(), *pw = w.data(), *qc = c.data(), *qw = w.data();
    cl_ordered_sum<B>(n, [&] { return *pc++; }, [&](int s, double cv) { b1 = b1 + (-x[s]) * cv; });
    cl_ordered_sum<B>(n, [&] { return *pw++; }, [&](int s, double wv) { t1 = t1 + wv * x[s]; });
    cl_ordered_sum<B>(n, [&] { const double cv = *qc++; return D2{cv, *qw++}; }, [&](int, D2 e) { l1 = l1 + e.a * e.b; });
    check(bits(b0) == bits(b1)); check(bits(t0) == bits(t1)); check(bits(l0) == bits(l1));
}

int main()
{
    for (int n = 0; n <= 70; n++) { order<8>(n); order<16>(n); }
    const double inf = std::numeric_limits<double>::infinity();
    const double special[] = {0.0, -0.0, 1.0, -1.0, inf, -inf, 1e308, -1e308, 4.9e-324, 1e-300, 0.1, -0.3};
    uint64_t st = 88172645463325252ull;
    auto rnd = [&] { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; };
    for (int rep = 0; rep < 200; rep++) {
        std::vector<double> c(70), w(70), x(70);
        for (int s = 0; s < 70; s++) {
            auto pick = [&] { const uint64_t r = rnd(); return (r & 7) == 0 ? special[(r >> 8) % 12] : ((double)(int64_t)(r >> 11) / 4503599627370496.0 - 1.0) * ((r & 8) ? 1e3 : 1e-3); };
            c[s] = pick(); w[s] = pick(); x[s] = pick();
        }
        for (int n = 0; n <= 70; n++) { sums<8>(n, c, w, x); sums<16>(n, c, w, x); }
    }
    std::printf("%ld %ld\n", bad, nchk);
    return bad != 0;
}
