// Stand-alone host program for the rule part of ttcross_amd/csrc/ttx_bondstep.h (built and run by test_bondstep_cpu.py,
// plain and under -fsanitize=address,undefined).  Prints "<failures> <rook sequences compared> <other checks>".
#include <climits>
#include <cmath>
#include <cstdio>
#include <vector>
#include "ttx_bondstep.h"

static long bad = 0, nseq = 0, nchk = 0;
#define CHECK(c, ...) do { nchk++; if (!(c)) { if (bad++ < 10) { printf("line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Step { int iscol, resid, done_turn, done, ii, jj, kk, qq; };
static bool same(const Step &a, const Step &b)
{ return a.iscol == b.iscol && a.resid == b.resid && a.done_turn == b.done_turn && a.done == b.done && a.ii == b.ii && a.jj == b.jj && a.kk == b.kk && a.qq == b.qq; }

// The arg-max of residual fiber number t of a bond step (t counts the residuals taken): bit t of `rep` set = the position of
// the current pivot again, else the next position (cyclically) -- a different one, the fibers here have more than one entry.
static int scripted(unsigned rep, int t, int cur, int nf) { return ((rep >> t) & 1u) ? cur : (cur + 1) % nf; }

// the kernels' form: H = 2 piv half-steps (2 for piv = 0), each one rook_turn and, with a residual, one take_pivot
static std::vector<Step> by_rules(int piv, int dir, unsigned rep, int r0, int n1, int n2, int r2, int ii, int jj, int kk, int qq)
{
    std::vector<Step> out;
    int crs = 0, havecol = 0, haverow = 0, done = 0, t = 0;
    const int H = (piv == 0) ? 2 : 2 * piv, mode = (piv == 0) ? 1 : 0;
    for (int h = 0; h < H && !done; h++) {
        const RookTurn tn = rook_turn(piv, mode, h, dir, crs, havecol, haverow);
        crs = tn.crs; havecol = tn.havecol; haverow = tn.haverow; done = tn.done;
        if (tn.resid) {
            const int ix = tn.iscol ? scripted(rep, t, (ii - 1) + r0 * (jj - 1), r0 * n1) : scripted(rep, t, (kk - 1) + n2 * (qq - 1), n2 * r2);
            t++;
            done = take_pivot(tn.iscol, ix, r0, n2, havecol, haverow, ii, jj, kk, qq);
        }
        out.push_back(Step{tn.iscol ? 1 : 0, tn.resid ? 1 : 0, tn.done ? 1 : 0, done ? 1 : 0, ii, jj, kk, qq});
    }
    return out;
}

// the reference's loop shape (lib/dmrgg.f90:492-513 for piv = 0, :516-582): column unless the first turn of a left-going
// step skips it, then row, until done
static std::vector<Step> by_loop(int piv, int dir, unsigned rep, int r0, int n1, int n2, int r2, int ii, int jj, int kk, int qq)
{
    std::vector<Step> out;
    bool done = false, havecol = false, haverow = false;
    if (piv == 0) {                                  // both fibers, no residual, no search
        out.push_back(Step{1, 0, 0, 0, ii, jj, kk, qq});
        out.push_back(Step{0, 0, 1, 1, ii, jj, kk, qq});
        done = havecol = haverow = true;
    }
    int crs = 0, t = 0;
    bool skipcol = (dir == 2);
    while (!done) {
        if (!skipcol) {
            havecol = true; crs = crs + 1;
            done = havecol && haverow && (crs >= 2 * piv);
            const bool stop = done;
            if (!done) {
                const int ij = scripted(rep, t++, (ii - 1) + r0 * (jj - 1), r0 * n1);
                const int j = ij / r0 + 1, i = ij - (j - 1) * r0 + 1;
                done = havecol && haverow && (i == ii && j == jj);
                ii = i; jj = j;
            }
            out.push_back(Step{1, stop ? 0 : 1, stop ? 1 : 0, done ? 1 : 0, ii, jj, kk, qq});
        }
        skipcol = false;
        if (!done) {
            haverow = true; crs = crs + 1;
            done = havecol && haverow && (crs >= 2 * piv);
            const bool stop = done;
            if (!done) {
                const int kq = scripted(rep, t++, (kk - 1) + n2 * (qq - 1), n2 * r2);
                const int q = kq / n2 + 1, k = kq - (q - 1) * n2 + 1;
                done = havecol && haverow && (k == kk && q == qq);
                kk = k; qq = q;
            }
            out.push_back(Step{0, stop ? 0 : 1, stop ? 1 : 0, done ? 1 : 0, ii, jj, kk, qq});
        }
    }
    return out;
}

static void rook_sequences()
{
    const int shapes[3][4] = {{3, 5, 4, 2}, {1, 2, 2, 1}, {7, 3, 3, 7}};      // r0, n1, n2, r2 (every fiber longer than one entry)
    for (int piv = 0; piv <= 5; piv++)
        for (int dir = 1; dir <= 2; dir++)
            for (int sh = 0; sh < 3; sh++) {
                const int r0 = shapes[sh][0], n1 = shapes[sh][1], n2 = shapes[sh][2], r2 = shapes[sh][3];
                const int nres = (piv == 0) ? 0 : 2 * piv;            // a bond step takes fewer residuals than half-steps
                for (unsigned rep = 0; rep < (1u << nres); rep++) {   // the arg-max repeats the pivot at any subset of them
                    const std::vector<Step> a = by_rules(piv, dir, rep, r0, n1, n2, r2, r0, 1, 1, r2);
                    const std::vector<Step> b = by_loop(piv, dir, rep, r0, n1, n2, r2, r0, 1, 1, r2);
                    bool eq = a.size() == b.size();
                    for (size_t s = 0; eq && s < a.size(); s++) eq = same(a[s], b[s]);
                    nseq++;
                    CHECK(eq, "piv %d dir %d shape %d rep %#x: %zu turns by the rules, %zu by the loop", piv, dir, sh, rep, a.size(), b.size());
                    CHECK(!a.empty() && a.back().done == 1, "piv %d dir %d rep %#x: the last turn does not stop", piv, dir, rep);
                    CHECK((int)a.size() <= ((piv == 0) ? 2 : 2 * piv), "piv %d dir %d rep %#x: %zu turns", piv, dir, rep, a.size());
                }
            }
}

static void pivot_taking()
{
    int ii, jj, kk, qq, d;
    // r0 = 1: every column position is (1, j)
    ii = 1; jj = 1; kk = 2; qq = 3;
    d = take_pivot(true, 4, 1, 5, 1, 1, ii, jj, kk, qq);
    CHECK(ii == 1 && jj == 5 && kk == 2 && qq == 3 && d == 0, "r0 = 1: %d %d %d %d done %d", ii, jj, kk, qq, d);
    // n2 = 1: every row position is (1, q)
    d = take_pivot(false, 6, 4, 1, 1, 1, ii, jj, kk, qq);
    CHECK(ii == 1 && jj == 5 && kk == 1 && qq == 7 && d == 0, "n2 = 1: %d %d %d %d done %d", ii, jj, kk, qq, d);
    // the last position of a 3 x 4 column fiber and of a 5 x 2 row fiber
    d = take_pivot(true, 3 * 4 - 1, 3, 5, 1, 1, ii, jj, kk, qq);
    CHECK(ii == 3 && jj == 4 && d == 0, "last column position: %d %d done %d", ii, jj, d);
    d = take_pivot(false, 5 * 2 - 1, 3, 5, 1, 1, ii, jj, kk, qq);
    CHECK(kk == 5 && qq == 2 && d == 0, "last row position: %d %d done %d", kk, qq, d);
    // the same pivot again stops only once both types were seen
    d = take_pivot(true, 3 * 4 - 1, 3, 5, 1, 0, ii, jj, kk, qq);
    CHECK(ii == 3 && jj == 4 && d == 0, "repeat before a row was seen: done %d", d);
    d = take_pivot(true, 3 * 4 - 1, 3, 5, 1, 1, ii, jj, kk, qq);
    CHECK(ii == 3 && jj == 4 && d == 1, "repeat with both seen: done %d", d);
    d = take_pivot(false, 5 * 2 - 1, 3, 5, 1, 1, ii, jj, kk, qq);
    CHECK(kk == 5 && qq == 2 && d == 1, "row repeat with both seen: done %d", d);
    // nothing compared (every residual a NaN): the first position
    d = take_pivot(true, INT_MAX, 3, 5, 1, 1, ii, jj, kk, qq);
    CHECK(ii == 1 && jj == 1 && kk == 5 && qq == 2 && d == 0, "INT_MAX column: %d %d %d %d done %d", ii, jj, kk, qq, d);
    d = take_pivot(false, INT_MAX, 3, 5, 1, 1, ii, jj, kk, qq);
    CHECK(ii == 1 && jj == 1 && kk == 1 && qq == 1 && d == 0, "INT_MAX row: %d %d %d %d done %d", ii, jj, kk, qq, d);
    d = take_pivot(true, INT_MAX, 3, 5, 1, 1, ii, jj, kk, qq);
    CHECK(ii == 1 && jj == 1 && d == 1, "INT_MAX at (1,1) is the same pivot again: done %d", d);
}

static void acceptance()
{
    const double se = 0x1p-10, sp = 0x1p-20;
    CHECK(!accept_pivot(se * 3.0, 3.0, 0.0, se, sp), "|pivot| == small_element * amax is refused");
    CHECK(!accept_pivot(-se * 3.0, 3.0, 0.0, se, sp), "the same for a negative pivot");
    CHECK(accept_pivot(nextafter(se * 3.0, 1.0), 3.0, 0.0, se, sp), "one ulp above is accepted");
    CHECK(!accept_pivot(sp * 7.0, 0.0, 7.0, se, sp), "|pivot| == small_pivot * pivotmax_prev is refused");
    CHECK(accept_pivot(-nextafter(sp * 7.0, 1.0), 0.0, 7.0, se, sp), "one ulp above is accepted");
    CHECK(!accept_pivot(NAN, 1.0, 1.0, se, sp), "a NaN pivot is refused");
    CHECK(!accept_pivot(NAN, 0.0, -1.0, se, sp), "a NaN pivot is refused in a first sweep");
    CHECK(!accept_pivot(1.0, NAN, 1.0, se, sp), "a NaN amax refuses");
    // first sweep: pivotmax_prev = -1 makes the second bound negative, so only the first decides
    CHECK(accept_pivot(0x1p-1074, 0.0, -1.0, se, sp), "first sweep: the smallest pivot above a zero amax is accepted");
    CHECK(!accept_pivot(0.0, 0.0, -1.0, se, sp), "first sweep: a zero pivot is refused by the first bound");
    CHECK(!accept_pivot(se, 1.0, -1.0, se, sp), "first sweep: equality with the first bound is refused");
}

static void range_and_traffic()
{
    double mx = -1.0, mn = -1.0;
    pivot_range(mx, mn, 3.0); CHECK(mx == 3.0 && mn == 3.0, "first value: %g %g", mx, mn);
    pivot_range(mx, mn, 5.0); CHECK(mx == 5.0 && mn == 3.0, "larger: %g %g", mx, mn);
    pivot_range(mx, mn, 2.0); CHECK(mx == 5.0 && mn == 2.0, "smaller: %g %g", mx, mn);
    pivot_range(mx, mn, 0.0); CHECK(mx == 5.0 && mn == 0.0, "zero is a value, not 'none yet': %g %g", mx, mn);
    // 8 bytes per double: nf x r1 factor slab + r1 vector + fiber in and out with a residual, else the fiber written once
    // (integers below 2^53: exact in fp64 whatever the order of the sums)
    const int cases[5][2] = {{1, 1}, {33, 12}, {64 * 101, 64}, {6464, 1}, {5, 63}};
    for (int c = 0; c < 5; c++) {
        const long long nf = cases[c][0], r1 = cases[c][1];
        CHECK(halfstep_traffic((int)nf, (int)r1, true) == (double)(8 * (nf * r1 + r1 + 2 * nf)), "traffic with residual nf %lld r1 %lld", nf, r1);
        CHECK(halfstep_traffic((int)nf, (int)r1, false) == (double)(8 * nf), "traffic without residual nf %lld", nf);
    }
}

int main()
{
    rook_sequences();
    pivot_taking();
    acceptance();
    range_and_traffic();
    printf("%ld %ld %ld\n", bad, nseq, nchk);
    return bad != 0;
}
