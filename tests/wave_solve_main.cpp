// Host check of the append's two triangular wave solves (ttcross_amd/csrc/ttx_wave_solve.h): wave_solve_L, wave_solve_rdg and
// wave_solve_U run here with a 64-lane wave as an array.  The lanes run one after the other in ascending order -- step s of a solve
// needs the value of lane s only, and lane s has finished by then -- and "the value of lane k" is a lookup of what lane k handed
// in at its own step.  Asked for a lane that has not run yet, or for a lane of the other solve of the wave, the lookup answers
// with a NaN, and so does the LU lookup for a request the lane has declared unused: a result that took either in cannot equal
// the plain substitution.  For every rank 1 .. 64 with one solve per wave, and 1 .. 32 with two (the second absent, with the same
// and with a different right-hand side): results equal to the plain forward / backward substitution bit for bit
// (-ffp-contract=off as in the library's build), every LU index asked for inside the packed r x r block, every entry of L (of U,
// and every diagonal entry for the reciprocals) used exactly once per solve and no other entry used.  Prints "<bad> <checks>".
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>
#include "ttx_wave_solve.h"

static long bad = 0, nchk = 0;
static void check(bool ok) { nchk++; if (!ok) bad++; }
static uint64_t bits(double x) { uint64_t b; std::memcpy(&b, &x, 8); return b; }
static const double POISON = std::numeric_limits<double>::quiet_NaN();

static uint64_t st = 88172645463325252ull;
static uint64_t rnd() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; }
static double unit() { return (double)(int64_t)(rnd() >> 11) / 4503599627370496.0 - 1.0; }      // [-1, 1)

// the plain substitutions (lib/dmrgg.f90:715-749 as the kernels state them)
static void plain_L(const std::vector<double> &lu, int r, const double *a, double *x)
{
    for (int l = 0; l < r; l++) {
        double tmp = 0.0;
        for (int s = 0; s < l; s++) tmp = tmp + x[s] * lu[l * l + s];
        x[l] = (l == 0) ? a[0] : a[l] + (-1.0) * tmp;
    }
}
static void plain_U(const std::vector<double> &lu, int r, const double *y0, double *y)
{
    for (int l = 0; l < r; l++) y[l] = y0[l];
    for (int s = 0; s < r; s++) {
        y[s] = (1.0 / lu[(s + 1) * (s + 1) - 1]) * y[s];
        for (int l = s + 1; l < r; l++) y[l] = y[l] + (-lu[l * l + l + s]) * y[s];
    }
}

struct Wave {                 // what the lanes that have run handed in, and the LU requests of the lane that runs
    double rec[64]; bool have[64]; int cur, lw;
    const std::vector<double> *lu; int r; bool inside;
    std::vector<int> uses[2];
    void start(const std::vector<double> &lu_, int r_, int lw_)
    { lu = &lu_; r = r_; lw = lw_; inside = true; for (int k = 0; k < 64; k++) have[k] = false; uses[0].assign(r * r, 0); uses[1].assign(r * r, 0); }
};
struct LaneOf { Wave &w; double operator()(double x, int k) const {
    if (k == w.cur) { w.rec[k] = x; w.have[k] = true; return x; }
    return (k < w.cur && k / w.lw == w.cur / w.lw && w.have[k]) ? w.rec[k] : POISON; } };
struct LuOf { Wave &w; double operator()(int i, bool used) const {
    if (i < 0 || i >= w.r * w.r) { w.inside = false; return POISON; }
    if (!used) return POISON;
    w.uses[w.cur / w.lw][i]++; return (*w.lu)[i]; } };

// second: 0 the second solve of the wave absent (its lanes pass 0), 1 present with the same right-hand side, 2 with another
template <int PK>
static void one(int r, int second)
{
    const int lw = 64 / PK;
    std::vector<double> lu(r * r);
    for (int l = 0; l < r; l++) {
        for (int s = 0; s < 2 * l; s++) lu[l * l + s] = unit();
        const double d = 1.0 + 0.5 * (unit() + 1.0);                 // diagonal of U in [1, 2), either sign: well conditioned
        lu[(l + 1) * (l + 1) - 1] = (rnd() & 1) ? d : -d;
    }
    double rhs[2][64] = {}, in[64], xL[64], yU[64], refL[2][64] = {}, refU[2][64] = {};
    for (int l = 0; l < r; l++) { rhs[0][l] = unit() * 3.0; rhs[1][l] = (PK == 1 || second == 0) ? 0.0 : second == 1 ? rhs[0][l] : unit() * 3.0; }
    for (int h = 0; h < PK; h++) { plain_L(lu, r, rhs[h], refL[h]); plain_U(lu, r, rhs[h], refU[h]); }
    for (int L = 0; L < 64; L++) in[L] = (L % lw < r) ? rhs[L / lw][L % lw] : 0.0;
    Wave w;
    // role C
    w.start(lu, r, lw);
    for (int L = 0; L < 64; L++) { w.cur = L; xL[L] = wave_solve_L<PK>(LuOf{w}, r, in[L], L % lw, L / lw, LaneOf{w}); }
    bool same = true, once = true;
    for (int h = 0; h < PK; h++) {
        for (int l = 0; l < r; l++) same = same && bits(xL[h * lw + l]) == bits(refL[h][l]);
        for (int l = 0; l < r; l++) for (int s = 0; s < 2 * l + 1; s++) once = once && w.uses[h][l * l + s] == (s < l ? 1 : 0);
    }
    check(same); check(once); check(w.inside);
    // role D
    w.start(lu, r, lw);
    for (int L = 0; L < 64; L++) {
        w.cur = L;
        const double rdg = wave_solve_rdg(LuOf{w}, r, L % lw);
        yU[L] = wave_solve_U<PK>(LuOf{w}, r, in[L], rdg, L % lw, L / lw, LaneOf{w});
    }
    same = true; once = true;
    for (int h = 0; h < PK; h++) {
        for (int l = 0; l < r; l++) same = same && bits(yU[h * lw + l]) == bits(refU[h][l]);
        for (int l = 0; l < r; l++) for (int s = 0; s < 2 * l + 1; s++) once = once && w.uses[h][l * l + s] == ((s >= l) ? 1 : 0);
    }
    check(same); check(once); check(w.inside);
}

int main()
{
    for (int rep = 0; rep < 4; rep++) {
        for (int r = 1; r <= 64; r++) one<1>(r, 0);
        for (int r = 1; r <= 32; r++) for (int second = 0; second < 3; second++) one<2>(r, second);
    }
    std::printf("%ld %ld\n", bad, nchk);
    return bad != 0;
}
