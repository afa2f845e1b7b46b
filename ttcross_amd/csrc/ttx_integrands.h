// ttx_integrands.h -- the built-in integrands of the reference's drivers and the index sources they are evaluated from: one multi-index
// (f_*, eval_fun), three or four index rows of a fiber element (Src3 / Src4, eval_src3 / eval_src4), rows of VALUES (chain8*).
// Compiled with -ffp-contract=off: every product and sum below is an individual IEEE fp64 rounding, in the
// order of the netlib reference BLAS the oracle restates, so pivot paths are reproducible bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include "ttx_cdf.h"
#include "ttx_dev.h"
#include "ttx_exp.h"
#include "ttx_fast.h"     // TTX_ARITH=fast: re-associated evaluation of the heavy integrands (tolerance-checked mode)

// ------------------------------------------------------------------------------------------------
// integrands (reference drivers' callbacks).  idx(s), s = 1..m, returns the 1-based mode index of dim s.
// ------------------------------------------------------------------------------------------------
template <class IDX>
__device__ __forceinline__ double f_ising(int id, int m, int n1, const double *par, IDX idx, bool unit = false)
{
    // test_crs_ising.f90:176-218.  unit (all nodes in [0,1]): a row of the pair triangle ends where the running product has reached
    // 2^-54 -- from there on every factor is EXACTLY 1 in fp64 (see f_ising_de), so leaving them out changes no bit
    const double *nodes = par - 1, *weights = par + n1 - 1;
    double a = 1.0, b = 0.0, f;
    if (id == 2 || id == 3) {
        for (int i = 0; i <= m; i++) {
            double uij = 1.0;
            for (int j = i + 1; j <= m; j++) {
                uij = uij * nodes[idx(j)];
                if (unit && uij <= 0x1p-54) break;
                double t = (uij - 1.0) / (uij + 1.0);
                a = a * (t * t);
            }
        }
    }
    if (id == 1 || id == 2) {
        double v = 1.0, w = 1.0, vk = 1.0, wk = 1.0;
        for (int i = 1; i <= m; i++) {
            vk = vk * nodes[idx(m - i + 1)];
            wk = wk * nodes[idx(i)];
            v = v + vk;
            w = w + wk;
        }
        b = 1.0 / (v * w);
    }
    f = (id == 1) ? 2 * b : (id == 2) ? 2 * a * b : 2 * a;
    for (int i = 1; i <= m; i++) f = f * weights[idx(i)];
    return f;
}

// TTX_ARITH=fast, any multi-index (initial cross, boundary corners, dtt_accchk): rho by de_fast_rho, then the b-part and
// the weights as above; f = (2 rho b w_1 ... w_m) rho keeps rho^2 out of the intermediate results (more range than a itself)
template <class IDX>
__device__ __forceinline__ double f_ising_fast(int id, int m, int n1, const double *par, IDX idx)
{
    const double *nodes = par - 1, *weights = par + n1 - 1;
    const double rho = de_fast_rho(m, nodes, idx);
    double b = 1.0;
    if (id == 2) {
        double v = 1.0, w = 1.0, vk = 1.0, wk = 1.0;
        for (int i = 1; i <= m; i++) {
            vk = vk * nodes[idx(m - i + 1)];
            wk = wk * nodes[idx(i)];
            v = v + vk;
            w = w + wk;
        }
        b = 1.0 / (v * w);
    }
    double f = 2 * rho * b;
    for (int i = 1; i <= m; i++) f = f * weights[idx(i)];
    return f * rho;
}

template <class IDX>
__device__ __forceinline__ double f_stdnorm(int m, const double *par, IDX idx)
{
    // test_crs_stdnorm.f90:154-170
    double s = 0.0;
    for (int i = 1; i <= m; i++) { double x = par[idx(i) - 1]; s = s + x * x; }
    return ttx_exp(-s);
}

template <class IDX>
__device__ __forceinline__ double f_mvn(int m, const double *par, const double *aux, double norm, IDX idx)
{
    // test_crs_mvn.f90:156-172 + lib/mvn_pdf.f90:63-83
    const double *mu = aux, *ic = aux + m;
    double ex = 0.0;
    for (int i = 1; i <= m; i++) {
        double di = par[idx(i) - 1] - mu[i - 1];
        for (int j = 1; j <= m; j++) {
            double dj = par[idx(j) - 1] - mu[j - 1];
            ex = ex + di * ic[(i - 1) + (size_t)m * (j - 1)] * dj;
        }
    }
    return ttx_exp(-0.5 * ex) / norm;
}

// The same quadratic form from rows of DIFFERENCES x - mu staged in LDS: dims 1..A from da, dim A+1 = d1, (NS == 2:
// dim A+2 = d2,) the remaining nb dims from db.  Term order and association are those of f_mvn / mvn_pdf
// (lib/mvn_pdf.f90:74-80): ex = ex + (diff(i) * inv_cov(i,j)) * diff(j), i outer, j inner -- only the O(d) index
// decoding per term is gone (the inverse covariance is read with wave-uniform addresses).
template <int NS, class FN>
__device__ __forceinline__ void mvn_dims(const double *da, int A, double d1, double d2, const double *db, int nb, FN fn)
{
#pragma unroll 8
    for (int t = 0; t < A; t++) fn(da[t]);
    fn(d1);
    if (NS == 2) fn(d2);
#pragma unroll 8
    for (int t = 0; t < nb; t++) fn(db[t]);
}
template <int NS>
__device__ __forceinline__ double f_mvn_rows(int m, const double *icT, double norm, const double *da, int A, double d1, double d2,
                                             const double *db)
{
    const int nb = m - A - NS;
    double ex = 0.0;
    int i = 0;
    mvn_dims<NS>(da, A, d1, d2, db, nb, [&](double di) {
        const double *row = icT + (size_t)m * i;       // icT[j + m*i] = inv_cov(i,j): the j loop walks contiguous memory
        int j = 0;
        mvn_dims<NS>(da, A, d1, d2, db, nb, [&](double dj) { ex = ex + di * row[j] * dj; j++; });
        i++;
    });
    return ttx_exp(-0.5 * ex) / norm;
}

// host integrand: pass 1 records the multi-index of the point in slot `slot`, pass 2 returns the host's value
template <class IDX>
__device__ __forceinline__ double f_host(const DevProb &P, IDX idx, long slot)
{
    if (P.hostpass == 1) {
        short *row = P.hidx + (size_t)slot * P.d;
        for (int s = 1; s <= P.d; s++) row[s - 1] = (short)idx(s);
        P.hreq[slot] = 1;
        return 0.0;
    }
    return P.hval[slot];
}
#define HOST_PASS1(FUN, P) ((FUN) == FUN_HOST && (P).hostpass == 1)

template <int FUN, class IDX>
__device__ __forceinline__ double eval_fun(const DevProb &P, const double *par, IDX idx, long slot = -1)
{
    if (FUN == FUN_HOST) return f_host(P, idx, slot);
    if (FUN == FUN_ISING) return (P.arith && P.ising_id != 1) ? f_ising_fast(P.ising_id, P.d, P.n[1], par, idx) : f_ising(P.ising_id, P.d, P.n[1], par, idx, P.de_unit != 0);
    if (FUN == FUN_STDNORM) return f_stdnorm(P.d, par, idx);
    return f_mvn(P.d, par, P.aux, P.mvn_norm, idx);
}

// Index source of one superblock entry: dims 1..A from pa[0..A-1], dim A+1 = self, dims A+2..m from pb[0..].
// The flattened tables are staged in LDS with one CONTIGUOUS row per thread; this replaces the reference's
// nested vip walk (dmrgg_fun, lib/dmrgg.f90:1062-1075).
struct Src3 {
    const short *pa; int A, self; const short *pb;
    __device__ __forceinline__ int operator()(int s) const
    { return (s <= A) ? (int)pa[s - 1] : (s == A + 1) ? self : (int)pb[s - A - 2]; }
};
// the same with two explicit dims (A+1 = s1, A+2 = s2): a lottery candidate (i,j,k,q) read straight from the
// transposed pivot tables, pa = row of left pivot i, pb = row of right pivot q
struct Src4 {
    const short *pa; int A, s1, s2; const short *pb;
    __device__ __forceinline__ int operator()(int s) const
    { return (s <= A) ? (int)pa[s - 1] : (s == A + 1) ? s1 : (s == A + 2) ? s2 : (int)pb[s - A - 3]; }
};

// 8 indices with one 128-bit LDS read (rows are 16-byte aligned and padded with the valid index 1)
struct __align__(16) Short8 { short v[8]; };
__device__ __forceinline__ Short8 ld8(const short *p) { return *reinterpret_cast<const Short8 *>(__builtin_assume_aligned(p, 16)); }

// One dependent recurrence over n table entries addressed by a 16-byte-aligned, padded index row: per chunk of
// 8 dims one 128-bit index read and 8 independent table reads precede the 8 dependent fp64 steps; only the
// chunk that holds the row's end is predicated.
template <bool DESC, class STEP>
__device__ __forceinline__ void chain8(const short *p, int n, const double *tab, STEP step)
{
    if (n <= 0) return;
    const int nfull = n >> 3, rem = n & 7;
    if (DESC && rem) {
        Short8 ix = ld8(p + 8 * nfull); double x[8];
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = tab[ix.v[k]];
#pragma unroll
        for (int k = 7; k >= 0; k--) if (k < rem) step(x[k]);
    }
#pragma unroll 2
    for (int ch = 0; ch < nfull; ch++) {
        const int c = 8 * (DESC ? nfull - 1 - ch : ch);
        Short8 ix = ld8(p + c); double x[8];
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = tab[ix.v[k]];
#pragma unroll
        for (int k = 0; k < 8; k++) step(x[DESC ? 7 - k : k]);
    }
    if (!DESC && rem) {
        Short8 ix = ld8(p + 8 * nfull); double x[8];
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = tab[ix.v[k]];
#pragma unroll
        for (int k = 0; k < 8; k++) if (k < rem) step(x[k]);
    }
}

// ---- Ising D / E (id 2, 3) over aligned index rows ----------------------------------------------------------
// The O(d^2) product a = prod_{i<j} ((u_ij-1)/(u_ij+1))^2 (test_crs_ising.f90:186-195) is one IEEE division per
// step on a sequential chain; the generic accessor exposed two dependent LDS latencies (index, node value) plus
// scalar control flow in every step.  Here the dims are walked as branch-free ranges of the staged rows with
// 8-wide chunk loads (one 128-bit index read + 8 independent table reads ahead of the 8 dependent steps).
// Layout: dims 1..A from pa, then NS explicit dims (s1[, s2]), then dims A+NS+1..m from pb.
template <class STEP>
__device__ __forceinline__ void seg_range(const short *p, int lo, int hi, const double *tab, STEP step)
{   // elements [lo, hi) of an aligned, padded row, ascending
#pragma unroll 2
    for (int c = lo & ~7; c < hi; c += 8) {
        Short8 ix = ld8(p + c); double x[8];
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = tab[ix.v[k]];
        if (c >= lo && c + 8 <= hi) {
#pragma unroll
            for (int k = 0; k < 8; k++) step(x[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) if (c + k >= lo && c + k < hi) step(x[k]);
        }
    }
}
template <int NS, class STEP>
__device__ __forceinline__ void dims_asc(const short *pa, int A, int s1, int s2, const short *pb, int m, const double *tab,
                                         int jlo, int jhi, STEP step)
{   // dims jlo..jhi (1-based, inclusive), ascending
    if (jlo > jhi) return;
    const int a1 = jhi < A ? jhi : A;
    if (jlo <= a1) seg_range(pa, jlo - 1, a1, tab, step);
    if (jlo <= A + 1 && A + 1 <= jhi) step(tab[s1]);
    if (NS == 2 && jlo <= A + 2 && A + 2 <= jhi) step(tab[s2]);
    const int b0 = jlo > A + NS + 1 ? jlo : A + NS + 1;
    if (b0 <= jhi) seg_range(pb, b0 - A - NS - 1, jhi - A - NS, tab, step);
}
// b-part (id 2) and the weights of the D / E integrand once the pair product a is known (:197-218)
template <int NS>
__device__ __forceinline__ double de_finish(int id, double a, int m, int n1, const double *par, const short *pa, int A, int s1, int s2, const short *pb);

// IEEE-exact fp64 division for operands in the "unit" range of the Ising integrands: with all nodes in [0,1] every
// running product u lies in [0,1], so d = u+1 is in [1,2] and n = u-1 in [-1,0].  The compiler's a/b is
// v_div_scale x2, v_rcp, 4 fma, mul, fma, v_div_fmas, v_div_fixup; for such operands neither v_div_scale rescales nor
// does v_div_fixup change anything but the sign it would set anyway, so the Newton core alone -- the same v_rcp_f64 and
// the same fused operations in the same order -- returns the identical bits with four instructions fewer.
// (P.de_unit is set by the host only after checking the nodes; any other node set takes the plain division.)
__device__ __forceinline__ double fdiv_unit(double n, double d)
{
    double r = __builtin_amdgcn_rcp(d);
    double e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-d, r, 1.0);
    r = __builtin_fma(r, e, r);
    const double q = n * r;
    const double rem = __builtin_fma(-d, q, n);
    return __builtin_fma(rem, r, q);
}
template <bool FAST>
__device__ __forceinline__ double de_t2(double u)
{   // ((u-1)/(u+1))^2, test_crs_ising.f90:190-191
    const double n = u - 1.0, d = u + 1.0;
    const double t = FAST ? fdiv_unit(n, d) : n / d;
    return t * t;
}
// W independent pair factors at once, written STAGE BY STAGE.  One division is a chain of nine dependent fp64
// instructions, most of them FMAs with two or three VGPR operands, which a lone wave issues only every ~8.5 cycles
// (profiles/r02_probe_dpp.txt: 3.5 ns per instruction against 1.9 ns with constant operands).  Measured per pair on one
// wave: 85 ns with one chain, 57 with two, 42 with four (what the compiler makes of four de_t2 calls), 35 with eight
// chains interleaved -- the SIMD's own limit with several resident waves is 29 ns.  Same operations per element as
// de_t2 / fdiv_unit, so the same bits.
template <bool FAST, int W>
__device__ __forceinline__ void de_t2xw(const double (&u)[W], double (&t)[W])
{
    if (!FAST) {
#pragma unroll
        for (int k = 0; k < W; k++) t[k] = de_t2<false>(u[k]);
        return;
    }
    double n[W], d[W], r[W], e[W], q[W];
#pragma unroll
    for (int k = 0; k < W; k++) { n[k] = u[k] - 1.0; d[k] = u[k] + 1.0; }
#pragma unroll
    for (int k = 0; k < W; k++) r[k] = __builtin_amdgcn_rcp(d[k]);
#pragma unroll
    for (int k = 0; k < W; k++) e[k] = __builtin_fma(-d[k], r[k], 1.0);
#pragma unroll
    for (int k = 0; k < W; k++) r[k] = __builtin_fma(r[k], e[k], r[k]);
#pragma unroll
    for (int k = 0; k < W; k++) e[k] = __builtin_fma(-d[k], r[k], 1.0);
#pragma unroll
    for (int k = 0; k < W; k++) r[k] = __builtin_fma(r[k], e[k], r[k]);
#pragma unroll
    for (int k = 0; k < W; k++) q[k] = n[k] * r[k];
#pragma unroll
    for (int k = 0; k < W; k++) e[k] = __builtin_fma(-d[k], q[k], n[k]);
#pragma unroll
    for (int k = 0; k < W; k++) q[k] = __builtin_fma(e[k], r[k], q[k]);
#pragma unroll
    for (int k = 0; k < W; k++) t[k] = q[k] * q[k];
}
template <bool FAST>
__device__ __forceinline__ void de_t2x4(double u1, double u2, double u3, double u4, double &t1, double &t2, double &t3, double &t4)
{
    const double u[4] = {u1, u2, u3, u4}; double t[4];
    de_t2xw<FAST, 4>(u, t);
    t1 = t[0]; t2 = t[1]; t3 = t[2]; t4 = t[3];
}

// Pair product of an element (left pivot row il | s1 | s2 | right pivot row q) from the per-bond tables built by
// k_de_tables: the factor ((u_ij-1)/(u_ij+1))^2 of a pair depends only on the dims i+1..j, so every pair that lies
// entirely in the left pivot's dims (TL) or entirely in the right pivot's dims (TR) is shared by all elements through
// that pivot and is only MULTIPLIED here -- in the reference's order, so the product is bit-identical; the IEEE
// divisions are left for the pairs that span the bond (about a third of all pairs on average).
// TLc / ULc / TRc point at the pivot's own CONTIGUOUS row of the [pivot][pair] tables (this thread streams it);
// rix[ro .. ro+B): the right pivot's index entries (rix itself 16-byte aligned and padded).
template <bool FAST>
__device__ __forceinline__ double de_pairs_tab(int m, const double *nodes, int A, const double *TLc, const double *ULc,
                                               int s1, int s2, const short *rix, int ro, const double *TRc)
{
    const int B = m - A - 2;
    const double x1 = nodes[s1], x2 = nodes[s2];
    double a = 1.0;
    size_t pr = 0;
    auto run = [&](double u) {                          // the bond-spanning tail of a row: ... s2, right dims
        auto step = [&](double xv) { u = u * xv; a = a * de_t2<FAST>(u); };
        step(x2);
        seg_range(rix, ro, ro + B, nodes, step);
    };
    for (int i = 0; i <= A; i++) {
        const int cnt = A - i;
#pragma unroll 8
        for (int t = 0; t < cnt; t++) a = a * TLc[pr + t];
        pr += cnt;
        double u = ULc[i];
        u = u * x1; a = a * de_t2<FAST>(u);
        run(u);
    }
    run(1.0);                                           // i = A+1: starts after s1
    const size_t nr = (size_t)B * (B + 1) / 2;          // i >= A+2: pairs inside the right pivot's dims
#pragma unroll 8
    for (size_t t = 0; t < nr; t++) a = a * TRc[t];
    return a;
}

// ... the same walk that STOPS a row once the running product has reached the unit cut (`done()` is asked after every chunk
// of 8 dims and after the explicit dims).  Exact mode with all nodes in [0,1] (P.de_unit): the running product u_ij never grows,
// and at u_ij <= 2^-54 the factor is EXACTLY 1 in fp64 -- u-1 rounds to -1, u+1 to 1, (-1/1)^2 = 1, a*1 = a -- so the rest of
// the row changes no bit of the product (the factors between the cut and the end of its chunk are multiplied: they are 1 too).
// At the drivers' Gauss-Legendre nodes a row ends after ~16 dims: 12 % of the 32 640 pairs of D_256 are left
// (oracle: ttxo_set_unit_skip, tests/test_oracle_golden.py::test_unit_skip_changes_no_bit).
template <class STEP, class DONE>
__device__ __forceinline__ bool seg_range_cut(const short *p, int lo, int hi, const double *tab, STEP step, DONE done)
{
    for (int c = lo & ~7; c < hi; c += 8) {
        Short8 ix = ld8(p + c); double x[8];
#pragma unroll
        for (int k = 0; k < 8; k++) x[k] = tab[ix.v[k]];
        if (c >= lo && c + 8 <= hi) {
#pragma unroll
            for (int k = 0; k < 8; k++) step(x[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) if (c + k >= lo && c + k < hi) step(x[k]);
        }
        if (done()) return true;
    }
    return false;
}
template <int NS, class STEP, class DONE>
__device__ __forceinline__ void dims_asc_cut(const short *pa, int A, int s1, int s2, const short *pb, int m, const double *tab,
                                             int jlo, int jhi, STEP step, DONE done)
{
    if (jlo > jhi) return;
    const int a1 = jhi < A ? jhi : A;
    if (jlo <= a1 && seg_range_cut(pa, jlo - 1, a1, tab, step, done)) return;
    if (jlo <= A + 1 && A + 1 <= jhi) step(tab[s1]);
    if (NS == 2 && jlo <= A + 2 && A + 2 <= jhi) step(tab[s2]);
    if (done()) return;
    const int b0 = jlo > A + NS + 1 ? jlo : A + NS + 1;
    if (b0 <= jhi) seg_range_cut(pb, b0 - A - NS - 1, jhi - A - NS, tab, step, done);
}
// ... and from the COMPACT tables of k_de_ctables (P.de_cut: nodes in [0,1]): a row of the pair triangle is tabulated only up to the
// unit cut (CLc[i] factors for start i; CLc[m] / CRc[m] = totals), ULc[i] = running product of the start's row through the last left
// dim, or 0 when the row has ended inside the pivot's dims; the bond-spanning tail of a row ends at the cut as well.  Every factor
// left out is exactly 1: the product is bit-identical to de_pairs_tab's and to the reference's.
__device__ __forceinline__ double de_pairs_ctab(int m, const double *nodes, int A, const double *TLc, const int *CLc, const double *ULc,
                                                int s1, int s2, const short *rix, int ro, const double *TRc, const int *CRc)
{
    const int B = m - A - 2;
    const double x1 = nodes[s1], x2 = nodes[s2];
    double a = 1.0, u = 1.0;
    size_t pr = 0;
    auto step = [&](double xv) { u = u * xv; a = a * de_t2<true>(u); };
    auto done = [&]() { return u <= 0x1p-54; };
    auto run = [&]() {                                  // the bond-spanning tail of a row from s2 on (u holds the product so far)
        u = u * x2;
        if (u <= 0x1p-54) return;
        a = a * de_t2<true>(u);
        seg_range_cut(rix, ro, ro + B, nodes, step, done);
    };
    // one run of tabulated factors in order, 16 loads in flight ahead of the 16 dependent multiplies
    auto stream = [&](const double *T, int n) {
        int t = 0;
        for (; t + 16 <= n; t += 16) {
            double f[16];
#pragma unroll
            for (int k = 0; k < 16; k++) f[k] = T[t + k];
#pragma unroll
            for (int k = 0; k < 16; k++) a = a * f[k];
        }
        for (; t < n; t++) a = a * T[t];
    };
    const int i0 = (int)ULc[m], pre = CLc[m - 1];       // rows before i0 end inside the left pivot's dims
    stream(TLc, pre);
    pr = pre;
    for (int i = i0; i <= A; i++) {
        const int cnt = (i < A) ? CLc[i] : 0;
        stream(TLc + pr, cnt);
        pr += cnt;
        u = ULc[i] * x1;
        if (u > 0x1p-54) { a = a * de_t2<true>(u); run(); }
    }
    u = 1.0; run();                                     // i = A+1: starts after s1
    stream(TRc, CRc[m]);                                // i >= A+2: pairs inside the right pivot's dims
    return a;
}

template <int NS>
__device__ __forceinline__ double f_ising_de(int id, int m, int n1, const double *par, const short *pa, int A, int s1, int s2, const short *pb, bool unit = false)
{
    const double *nodes = par - 1;
    double a = 1.0;
    if (unit) {
        for (int i = 0; i <= m; i++) {
            double uij = 1.0;
            const int jlo = i + 1, jhi = m;
            if (jlo > jhi) continue;
            dims_asc_cut<NS>(pa, A, s1, s2, pb, m, nodes, jlo, jhi, [&](double xv) {
                uij = uij * xv;
                a = a * de_t2<true>(uij);
            }, [&]() { return uij <= 0x1p-54; });
        }
        return de_finish<NS>(id, a, m, n1, par, pa, A, s1, s2, pb);
    }
    for (int i = 0; i <= m; i++) {                                   // :186-195
        double uij = 1.0;
        const int jlo = i + 1, jhi = m;
        if (jlo > jhi) continue;
        dims_asc<NS>(pa, A, s1, s2, pb, m, nodes, jlo, jhi, [&](double xv) {
            uij = uij * xv;
            const double t = (uij - 1.0) / (uij + 1.0);
            a = a * (t * t);
        });
    }
    return de_finish<NS>(id, a, m, n1, par, pa, A, s1, s2, pb);
}
template <int NS>
__device__ __forceinline__ double de_finish(int id, double a, int m, int n1, const double *par, const short *pa, int A, int s1, int s2, const short *pb)
{
    const double *nodes = par - 1, *weights = par + n1 - 1;
    const int nb = m - A - NS;
    double b = 0.0;
    if (id == 2) {                                                   // :197-205
        double v = 1.0, w = 1.0, vk = 1.0, wk = 1.0;
        auto vstep = [&](double xv) { vk = vk * xv; v = v + vk; };
        auto wstep = [&](double xv) { wk = wk * xv; w = w + wk; };
        chain8<true>(pb, nb, nodes, vstep);
        if (NS == 2) vstep(nodes[s2]);
        vstep(nodes[s1]);
        chain8<true>(pa, A, nodes, vstep);
        chain8<false>(pa, A, nodes, wstep);
        wstep(nodes[s1]);
        if (NS == 2) wstep(nodes[s2]);
        chain8<false>(pb, nb, nodes, wstep);
        b = 1.0 / (v * w);
    }
    double f = (id == 2) ? 2 * a * b : 2 * a;
    auto fstep = [&](double xv) { f = f * xv; };
    chain8<false>(pa, A, weights, fstep);
    fstep(weights[s1]);
    if (NS == 2) fstep(weights[s2]);
    chain8<false>(pb, nb, weights, fstep);
    return f;
}

// Ising C (id 1) over aligned rows.  Same arithmetic as f_ising: the v- and w-recurrences of
// test_crs_ising.f90:199-204 are independent, so they run as separate loops.
__device__ __forceinline__ double f_ising_c3(int m, int n1, const double *par, const Src3 &S)
{
    const double *nodes = par - 1, *weights = par + n1 - 1;
    const int A = S.A, nb = m - A - 1;
    double v = 1.0, w = 1.0, vk = 1.0, wk = 1.0;
    auto vstep = [&](double xv) { vk = vk * xv; v = v + vk; };
    auto wstep = [&](double xv) { wk = wk * xv; w = w + wk; };
    chain8<true>(S.pb, nb, nodes, vstep);
    vstep(nodes[S.self]);
    chain8<true>(S.pa, A, nodes, vstep);
    chain8<false>(S.pa, A, nodes, wstep);
    wstep(nodes[S.self]);
    chain8<false>(S.pb, nb, nodes, wstep);
    double b = 1.0 / (v * w);
    double f = 2 * b;
    auto fstep = [&](double xv) { f = f * xv; };
    chain8<false>(S.pa, A, weights, fstep);
    fstep(weights[S.self]);
    chain8<false>(S.pb, nb, weights, fstep);
    return f;
}
__device__ __forceinline__ double f_ising_c4(int m, int n1, const double *par, const Src4 &S)
{
    const double *nodes = par - 1, *weights = par + n1 - 1;
    const int A = S.A, nb = m - A - 2;
    double v = 1.0, w = 1.0, vk = 1.0, wk = 1.0;
    auto vstep = [&](double xv) { vk = vk * xv; v = v + vk; };
    auto wstep = [&](double xv) { wk = wk * xv; w = w + wk; };
    chain8<true>(S.pb, nb, nodes, vstep);
    vstep(nodes[S.s2]); vstep(nodes[S.s1]);
    chain8<true>(S.pa, A, nodes, vstep);
    chain8<false>(S.pa, A, nodes, wstep);
    wstep(nodes[S.s1]); wstep(nodes[S.s2]);
    chain8<false>(S.pb, nb, nodes, wstep);
    double b = 1.0 / (v * w);
    double f = 2 * b;
    auto fstep = [&](double xv) { f = f * xv; };
    chain8<false>(S.pa, A, weights, fstep);
    fstep(weights[S.s1]); fstep(weights[S.s2]);
    chain8<false>(S.pb, nb, weights, fstep);
    return f;
}
template <int FUN>
__device__ __forceinline__ double eval_src4(const DevProb &P, const double *par, const Src4 &S, long slot = -1)
{
    if (FUN == FUN_ISING && P.ising_id == 1) return f_ising_c4(P.d, P.n[1], par, S);
    if (FUN == FUN_ISING && P.arith) return f_ising_fast(P.ising_id, P.d, P.n[1], par, S);
    if (FUN == FUN_ISING) return f_ising_de<2>(P.ising_id, P.d, P.n[1], par, S.pa, S.A, S.s1, S.s2, S.pb, P.de_unit != 0);
    return eval_fun<FUN>(P, par, S, slot);
}

// Same recurrences over rows of VALUES (node / weight doubles staged in LDS, 16-byte aligned, padded): a step
// is one LDS read (two doubles per ds_read_b128) + the dependent multiply(+add).  A lone wave issues one VALU
// instruction per 4 cycles, so the instruction count per step -- not the fp64 latency -- bounds these chains.
struct __align__(16) Double2 { double a, b; };
template <bool DESC, class STEP>
__device__ __forceinline__ void chain8v(const double *p, int n, STEP step)
{
    if (n <= 0) return;
    const int nfull = n >> 3, rem = n & 7;
    if (DESC && rem) {
        double x[8];
#pragma unroll
        for (int k = 0; k < 4; k++) { Double2 t = *reinterpret_cast<const Double2 *>(p + 8 * nfull + 2 * k); x[2 * k] = t.a; x[2 * k + 1] = t.b; }
#pragma unroll
        for (int k = 7; k >= 0; k--) if (k < rem) step(x[k]);
    }
#pragma unroll 4
    for (int ch = 0; ch < nfull; ch++) {
        const int c = 8 * (DESC ? nfull - 1 - ch : ch);
        double x[8];
#pragma unroll
        for (int k = 0; k < 4; k++) { Double2 t = *reinterpret_cast<const Double2 *>(p + c + 2 * k); x[2 * k] = t.a; x[2 * k + 1] = t.b; }
#pragma unroll
        for (int k = 0; k < 8; k++) step(x[DESC ? 7 - k : k]);
    }
    if (!DESC && rem) {
        double x[8];
#pragma unroll
        for (int k = 0; k < 4; k++) { Double2 t = *reinterpret_cast<const Double2 *>(p + 8 * nfull + 2 * k); x[2 * k] = t.a; x[2 * k + 1] = t.b; }
#pragma unroll
        for (int k = 0; k < 8; k++) if (k < rem) step(x[k]);
    }
}
// chain8v with the LDS reads of the NEXT chunk issued before the dependent steps of the current one (two register sets, the
// loop unrolled by two so that they swap roles without copies).  Same values in the same order.
__device__ __forceinline__ void ld8d(const double *p, double (&x)[8])
{
#pragma unroll
    for (int k = 0; k < 4; k++) { const Double2 t = *reinterpret_cast<const Double2 *>(p + 2 * k); x[2 * k] = t.a; x[2 * k + 1] = t.b; }
}
template <bool DESC, class STEP>
__device__ __forceinline__ void chain8p(const double *p, int n, STEP step)
{
    if (n <= 0) return;
    const int nfull = n >> 3, rem = n & 7;
    double x[8], y[8];
    auto base = [&](int ch) { return 8 * (DESC ? nfull - 1 - ch : ch); };
    if (DESC && rem) {
        ld8d(p + 8 * nfull, x);
        if (nfull) ld8d(p + base(0), y);
#pragma unroll
        for (int k = 7; k >= 0; k--) if (k < rem) step(x[k]);
    } else if (nfull) ld8d(p + base(0), y);
    int ch = 0;
    for (; ch + 1 < nfull; ch += 2) {
        ld8d(p + base(ch + 1), x);
#pragma unroll
        for (int k = 0; k < 8; k++) step(y[DESC ? 7 - k : k]);
        if (ch + 2 < nfull) ld8d(p + base(ch + 2), y); else if (!DESC && rem) ld8d(p + 8 * nfull, y);
#pragma unroll
        for (int k = 0; k < 8; k++) step(x[DESC ? 7 - k : k]);
    }
    if (ch < nfull) {                      // one full chunk left (in y); the ascending remainder is requested under it
        if (!DESC && rem) ld8d(p + 8 * nfull, x);
#pragma unroll
        for (int k = 0; k < 8; k++) step(y[DESC ? 7 - k : k]);
        if (!DESC && rem) {
#pragma unroll
            for (int k = 0; k < 8; k++) if (k < rem) step(x[k]);
        }
    } else if (!DESC && rem) {             // the remainder sits in y (requested above) -- or nothing was requested yet (nfull == 0)
        if (nfull == 0) ld8d(p, y);
#pragma unroll
        for (int k = 0; k < 8; k++) if (k < rem) step(y[k]);
    }
}
// dims 1..A: (an, aw); dim A+1: (sn, sw); dims A+2..m: (bn, bw)   [n = node values, w = weight values]
__device__ __forceinline__ double f_ising_c3v(int m, int A, const double *an, const double *aw, double sn, double sw,
                                              const double *bn, const double *bw)
{
    const int nb = m - A - 1;
    double v = 1.0, w = 1.0, vk = 1.0, wk = 1.0;
    auto vstep = [&](double xv) { vk = vk * xv; v = v + vk; };
    auto wstep = [&](double xv) { wk = wk * xv; w = w + wk; };
    chain8v<true>(bn, nb, vstep);
    vstep(sn);
    chain8v<true>(an, A, vstep);
    chain8v<false>(an, A, wstep);
    wstep(sn);
    chain8v<false>(bn, nb, wstep);
    double b = 1.0 / (v * w);
    double f = 2 * b;
    auto fstep = [&](double xv) { f = f * xv; };
    chain8v<false>(aw, A, fstep);
    fstep(sw);
    chain8v<false>(bw, nb, fstep);
    return f;
}

// aligned = rows are 16-byte aligned and padded (half-step / lottery staging); else the generic accessor
template <int FUN, bool ALIGNED>
__device__ __forceinline__ double eval_src3(const DevProb &P, const double *par, const Src3 &S, long slot = -1)
{
    if (ALIGNED && FUN == FUN_ISING && P.ising_id == 1) return f_ising_c3(P.d, P.n[1], par, S);
    if (ALIGNED && FUN == FUN_ISING && P.arith) return f_ising_fast(P.ising_id, P.d, P.n[1], par, S);
    if (ALIGNED && FUN == FUN_ISING) return f_ising_de<1>(P.ising_id, P.d, P.n[1], par, S.pa, S.A, S.self, 0, S.pb, P.de_unit != 0);
    return eval_fun<FUN>(P, par, S, slot);
}
