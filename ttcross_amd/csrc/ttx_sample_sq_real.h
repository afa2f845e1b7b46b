// ttx_sample_sq_real.h -- REAL-valued samples drawn from the SQUARE of the piecewise-multilinear interpolant of the resident train
// (ttx_sample_sq_real / ttx_sample_sq_real_dev): the squared-density sampler (SIRT) of Cui and Dolgov (2022) on a continuous
// domain.  Every conditional is the square of a piecewise-linear vector function, a quadratic per cell, so it is non-negative
// whatever the signs of the cores; its CDF is a cubic per cell.
//
// The definition is in include/ttx.h.  The head pass is ttx_sample_sq's (sq_head) with the rows of the QR generalised from
// sqrt(e(i)) H_k(a, i, :) to dg(i) H_k(a, i, :) + sp(i) H_k(a, i+1, :): dg and sp are the upper bidiagonal Cholesky factor of the hat
// functions' mass matrix (sqr_mass_cholesky, on the host) for a drawn mode and the hat row of the coordinate for a held one.  Per
// chunk and per mode k = d .. 1:
//   k_sqr_rows_mfma / _exact   s(c, i) = sum_a m(a, i)^2 and c(c, j) = sum_a m(a, j) m(a, j+1), m(a, i) = sum_b H_k(a, i, b) x_c(b), to
//                      two sheets [chunk][n_k]
//   k_sqr_pick         one wave per sample: the cell masses from the sheets, the scan and the search of k_sr_draw, the root of the
//                      cubic inside the cell (sqr_invert), x_k, the cell and the hat values of the rounded x_k, the log term
//   k_sqr_step         one wave per sample: the two-term chain step of k_sr_draw (sr_chain_step); the states stay in work space
// The way back, ttx_rosenblatt_sq_real / _dev (x -> u, logq, val: the forward Rosenblatt map), is the same frame with one kernel exchanged:
//   k_sqr_cdf          in k_sqr_pick's place, one wave per point: the hat cell and values of the GIVEN x_k, one pass of running sums over
//                      the cell masses (sm_wave_before), the cubic inside the cell evaluated, not inverted (sqr_cdf), u_k, the log term
// then k_sr_count (ttx_sample_real.h) counts the failed samples.  No atomics and no sum whose order depends on the grid, the chunk
// or the other samples: a call repeats bit for bit.  Every index comes from lane numbers and counts, never from a value.
// Open: per-sample weights, ranks above 128.
// The first part of this file is plain C++ a host compiler accepts (tests/sample_sq_real_main.cpp and tests/rosenblatt_main.cpp run it on
// the CPU).
#pragma once
#include <math.h>
#include <stddef.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TTX_SQR_HD __host__ __device__ inline
#else
#define TTX_SQR_HD static inline
#endif

// The upper bidiagonal Cholesky factor U (M = U^T U, U(i, i) = dg(i), U(i, i+1) = sp(i)) of the mass matrix of the hat functions on n
// strictly ascending nodes: M(i, i) = (h_(i-1) + h_i) / 3 with one term at each end, M(i, i+1) = h_i / 6, h_i = t_(i+1) - t_i.  Plain
// double, one operation at a time: numpy restates it bit for bit.  A single node has no cell: dg = 1, sp = 0 (the mode is held).
TTX_SQR_HD void sqr_mass_cholesky(const double *t, int n, double *dg, double *sp)
{
    if (n == 1) { dg[0] = 1.0; sp[0] = 0.0; return; }
    double diag = (t[1] - t[0]) / 3.0;
    dg[0] = sqrt(diag);
    for (int i = 0; i < n - 1; i++) {
        const double h = t[i + 1] - t[i], off = h / 6.0;
        sp[i] = off / dg[i];
        diag = i + 1 < n - 1 ? (h + (t[i + 2] - t[i + 1])) / 3.0 : h / 3.0;
        dg[i + 1] = sqrt(diag - sp[i] * sp[i]);
    }
    sp[n - 1] = 0.0;
}

// lambda in [0, 1] with Q(lambda) = sp, Q(l) = q0 l + (qm - q0) l^2 + (q0 - 2 qm + q1) l^3 / 3: the position inside a cell whose
// density is q(l) = q0 (1-l)^2 + 2 qm l (1-l) + q1 l^2 (q0, q1 >= 0, |qm| <= sqrt(q0 q1) up to the defensive term, so q >= 0) at
// which the mass per unit length sp = s / h is reached, 0 <= sp <= Q(1) = (q0 + qm + q1) / 3.  The four numbers are first scaled by
// the power of two that takes max(q0, |qm|, q1) into [0.5, 1): lambda has no scale and the scaling is exact.  Then a safeguarded
// Newton iteration on the bracket [0, 1]: the bracket shrinks with the sign of Q(l) - sp at every iterate, and a step that leaves
// its interior, or starts where q <= 0, is replaced by the bracket's midpoint.  At most 64 iterations; it ends when lambda no
// longer changes.  Where q touches zero inside the cell (a sign change of the interpolant, qm = -sqrt(q0 q1)) Q is flat and Newton
// converges linearly with ratio 2/3: the residual Q - sp, of third order in the distance, is below 1e-30 max(q) after 64 steps.
// sp <= 0 gives 0, sp >= Q(1) gives 1; anything that is not a number ends as 0.
TTX_SQR_HD double sqr_invert(double q0, double qm, double q1, double sp)
{
    if (!(q0 == q0) || !(qm == qm) || !(q1 == q1) || !(sp == sp)) return 0.0;
    double m = q0 > q1 ? q0 : q1;
    const double am = fabs(qm);
    m = am > m ? am : m;
    if (!(m > 0.0) || m > 1.7976931348623157e308) return 0.0;
    int e;
    (void)frexp(m, &e);
    q0 = ldexp(q0, -e); qm = ldexp(qm, -e); q1 = ldexp(q1, -e); sp = ldexp(sp, -e);
    if (!(sp > 0.0)) return 0.0;
    if (sp >= ((q0 + qm) + q1) / 3.0) return 1.0;
    const double d1 = qm - q0, d2 = ((q0 - 2.0 * qm) + q1), d3 = d2 / 3.0;
    double lo = 0.0, hi = 1.0, l = 0.5;
    for (int it = 0; it < 64; it++) {
        const double f = l * (q0 + l * (d1 + l * d3)) - sp;
        if (f > 0.0) hi = l; else lo = l;
        if (f == 0.0) break;
        const double ql = q0 + l * (2.0 * d1 + l * d2);
        double ln = l - f / ql;
        if (!(ql > 0.0) || !(ln > lo && ln < hi)) ln = 0.5 * (lo + hi);
        if (ln == l) break;
        l = ln;
    }
    return l;
}

// Q(l) h^-1 the other way round: the mass per unit length of the cell's density q (sqr_invert's q0, qm, q1) from the cell's left
// node up to the position l, Q(l) = l (q0 + l ((qm - q0) + l (((q0 - 2 qm) + q1) / 3))) in the Horner form sqr_invert iterates on.
// The three coefficients are scaled by sqr_invert's power of two, the result is scaled back by ldexp: the relative error has no
// scale.  l <= 0 gives 0, l >= 1 the whole cell ((q0 + qm) + q1) / 3; anything that is not a number ends as 0.
TTX_SQR_HD double sqr_cdf(double q0, double qm, double q1, double l)
{
    if (!(q0 == q0) || !(qm == qm) || !(q1 == q1) || !(l == l)) return 0.0;
    double m = q0 > q1 ? q0 : q1;
    const double am = fabs(qm);
    m = am > m ? am : m;
    if (!(m > 0.0) || m > 1.7976931348623157e308) return 0.0;
    int e;
    (void)frexp(m, &e);
    q0 = ldexp(q0, -e); qm = ldexp(qm, -e); q1 = ldexp(q1, -e);
    if (!(l > 0.0)) return 0.0;
    const double Q = l >= 1.0 ? ((q0 + qm) + q1) / 3.0 : l * (q0 + l * ((qm - q0) + l * (((q0 - 2.0 * qm) + q1) / 3.0)));
    return ldexp(Q, e);
}

#if defined(__HIPCC__)
#include "ttx_sample_real.h"   // SrMode, sr_chain_step, sr_place, k_sr_count
#include "ttx_sample_sq.h"     // SqPlan, the head pass kernels, TTX_SQ_SHEET, TTX_SQ_AUTO_FLOPS
#include "ttx_ttops.h"         // dbl4

// EXACT, one index i of one sample with the state x: m(a, i) and m(a, i+1) by sums over ascending b from 0.0, s = sum_a m(a, i)^2 and
// c = sum_a m(a, i) m(a, i+1) over ascending a from 0.0, separate multiplies and adds.  The caller of i + 1 forms m(a, i+1) again by
// the same operations.  For i = n - 1 the neighbour is i itself and cr is not to be used.  One text for k_sqr_rows_exact and for the
// one-wave transport of ttx_pullback.h.
__device__ inline void sqr_rows_one(const double *H, int l, int n, int r1, const double *x, int i, double &s, double &cr)
{
    const bool nb = i + 1 < n;
    const double *Hi = H + i, *Hj = H + (nb ? i + 1 : i);
    s = 0.0; cr = 0.0;
    for (int a = 0; a < l; a++) {
        double m = 0.0, mn = 0.0;
#pragma unroll 4
        for (int b = 0; b < r1; b++) { const double xb = x[b]; m = m + Hi[(size_t)n * (a + (size_t)l * b)] * xb; mn = mn + Hj[(size_t)n * (a + (size_t)l * b)] * xb; }
        s = s + m * m;
        cr = cr + m * mn;
    }
}
// EXACT: one thread per pair (c, i), grid-stride, sqr_rows_one each.  c(n-1) is not written and never read.
__global__ __launch_bounds__(256) void k_sqr_rows_exact(const double *H, int l, int n, int r1, const double *X, int ldx, int C, double *S, double *Cs)
{
    const long long M = (long long)C * n;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < M; q += (long long)gridDim.x * 256) {
        const int c = (int)(q / n), i = (int)(q % n);
        double s, cr;
        sqr_rows_one(H, l, n, r1, X + (size_t)c * ldx, i, s, cr);
        S[q] = s;
        if (i + 1 < n) Cs[q] = cr;
    }
}

// MFMA: k_sq_rows_mfma's frame and lane maps (ttx_sample_sq.h).  A tile still feeds 16 consecutive indices to the A operand, but
// the tiles advance by 15, so that every cell has both of its nodes in one tile: tile t holds the indices 15 t .. 15 t + 15 and the
// cells 15 t .. 15 t + 14.  A lane holds the result rows kq + 4 reg of its column; the accumulator of the next row is, for kq < 3,
// the same register of lane + 16 and, for kq = 3, the next register of lane - 48.  Both are lane (lane + 16) mod 64: a lane with
// kq = 0 hands out its next register, every other lane the same one, and one cross-lane move (ds_bpermute, no LDS memory) per
// register fetches the neighbour.  Products and sums over a stay in registers.  s(i) is stored by the tile whose cell i is (rows 0
// .. 14) and, for the last index, by the tile that ends there; c(j) by rows 0 .. 14.  Rows >= n load index 0 and are never stored.
template <int KS>
__global__ __launch_bounds__(256) void k_sqr_rows_mfma(const double *H, int l, int n, int r1, const double *X, int ldx, int C, int tper, double *S, double *Cs)
{
    const int wave = threadIdx.x >> 6, ln = threadIdx.x & 63, col = ln & 15, kq = ln >> 4;
    const int c0 = 64 * blockIdx.y + 16 * wave;
    if (c0 >= C) return;
    const int c = c0 + col;
    const bool cok = c < C;
    const double *xp = X + (size_t)(cok ? c : 0) * ldx;
    double xb[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ks++) { const int b = 4 * ks + kq; xb[ks] = (cok && b < r1) ? xp[b] : 0.0; }
    const int nt = n > 1 ? (n + 13) / 15 : 1, t1 = min(nt, (int)(blockIdx.x + 1) * tper);
    const int src = (ln + 16) & 63;
    const unsigned ln_ = (unsigned)l * (unsigned)n;
    for (int t = blockIdx.x * tper; t < t1; t++) {
        const int ia = 15 * t + col;                                            // the index this lane loads for the A operand
        const double *Hi = H + (ia < n ? ia : 0);
        dbl4 sq = dbl4{0.0, 0.0, 0.0, 0.0}, cr = dbl4{0.0, 0.0, 0.0, 0.0};
        for (int a = 0; a < l; a++) {
            const double *Ha = Hi + (size_t)n * a;
            dbl4 acc = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < KS; ks++)
                if (4 * ks < r1) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ha[(unsigned)(4 * ks + kq) * ln_], xb[ks], acc, 0, 0, 0);
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const double give = (kq == 0 && reg < 3) ? acc[reg < 3 ? reg + 1 : 3] : acc[reg];
                const double nb = __shfl(give, src);
                sq[reg] = sq[reg] + acc[reg] * acc[reg];
                cr[reg] = cr[reg] + acc[reg] * nb;
            }
        }
        if (cok) {
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int rw = kq + 4 * reg, i = 15 * t + rw;
                if (i < n && (rw < 15 || i == n - 1)) S[(size_t)c * n + i] = sq[reg];
                if (rw < 15 && i < n - 1) Cs[(size_t)c * n + i] = cr[reg];
            }
        }
    }
}

// what a sample carries from one launch to the next: logq, the failure flag, and from k_sqr_pick to k_sqr_step the hat cell and values
struct SqrState { double *lq, *f0, *f1; int *fail, *ci; };

// the Bernstein coefficients of the density along cell j and the cell's mass: c(j) clamped into [-lim, lim], lim = sqrt(s(j))
// sqrt(s(j+1)) (Cauchy-Schwarz; a NaN passes through), q0 = s(j) + g, qm = c(j) + g, q1 = s(j+1) + g, A = (((q0 + qm) + q1) / 3) h_j
__device__ inline double sqr_cell(const double *Sc, const double *Cc, const double *t, double g, int j, double &q0, double &qm, double &q1)
{
    const double s0 = Sc[j], s1 = Sc[j + 1], lim = sqrt(s0) * sqrt(s1);
    double cc = Cc[j];
    cc = cc > lim ? lim : cc;
    cc = cc < -lim ? -lim : cc;
    q0 = s0 + g; qm = cc + g; q1 = s1 + g;
    return (((q0 + qm) + q1) / 3.0) * (t[j + 1] - t[j]);
}
__device__ inline double sqr_mass(const double *Sc, const double *Cc, const double *t, double g, int j, int nc)
{
    double q0, qm, q1;
    return j < nc ? sqr_cell(Sc, Cc, t, g, j, q0, qm, q1) : 0.0;
}

// the log term of a mode: the density at the hat values f0, f1 of the hat cell ci, with c(ci) clamped as in sqr_cell, over the total mass
__device__ inline double sqr_log_term(const double *Sc, const double *Cc, double g, int ci, double f0, double f1, double total)
{
    const double s0 = Sc[ci], s1 = Sc[ci + 1], lim = sqrt(s0) * sqrt(s1);
    double cc = Cc[ci];
    cc = cc > lim ? lim : cc;
    cc = cc < -lim ? -lim : cc;
    double dens = (((f0 * f0) * s0 + ((2.0 * f0) * f1) * cc) + (f1 * f1) * s1) + g;
    dens = dens > 0.0 ? dens : 0.0;
    return log(dens / total);
}

// The draw of one mode for one sample by one wave, from the sample's rows Sc and Cc of the two sheets, the mode's n nodes t, its
// defensive term g and the uniform uk: the cell masses with lanes along j, then k_sr_draw's search, clamps and placement
// (sm_wave_search, sr_mass_within, sr_place); a cell's mass is formed again in the search's second pass from the same numbers by the
// same expression.  A failed search sets fail and nothing else; otherwise cj is the drawn cell, xk the rounded coordinate, ci, f0, f1
// its hat cell and values, and the mode's log term is added to lq.  One text for k_sqr_pick and for ttx_pullback.h.
__device__ inline void sqr_pick_one(int n, const double *t, double g, const double *Sc, const double *Cc, double uk, int lane, bool &fail, double &lq, int &ci, int &cj,
                                    double &f0, double &f1, double &xk)
{
    const int nc = n - 1;
    const auto mass = [&](int j) { return sqr_mass(Sc, Cc, t, g, j, nc); };
    const SmFound f = sm_wave_search(nc, uk, lane, mass, mass);
    if (!f.ok) { fail = true; return; }
    cj = f.pos;
    double lam = 1.0;
    if (f.hit) {
        double q0, qm, q1;
        (void)sqr_cell(Sc, Cc, t, g, cj, q0, qm, q1);
        lam = sqr_invert(q0, qm, q1, sr_mass_within(f) / (t[cj + 1] - t[cj]));
    }
    xk = sr_place(t, n, cj, lam, ci, f0, f1);
    lq = lq + sqr_log_term(Sc, Cc, g, ci, f0, f1, f.total);
}
// the chain step of one sample by one wave: sr_chain_step with the hat cell range-checked where it is read (k_sqr_step, ttx_pullback.h)
__device__ inline void sqr_step_one(const double *G, int RM, size_t SS, int r0, int r1, int n, int ci, double f0, double f1, const double *x, double *z, int lane)
{
    const int top = n > 2 ? n - 2 : 0;
    ci = ci < 0 ? 0 : ci > top ? top : ci;
    sr_chain_step(G + (size_t)RM * ci, (size_t)RM, SS, r0, r1, n > 1, f0, f1, x, z, lane);
}

// One wave per sample, grid-stride, one launch per mode (0-based k), in the frame of k_sq_pick.  A held mode forms nothing: its
// coordinate goes to x and 0 to cell.  Otherwise the cell masses from the two sheets with lanes along j, then k_sr_draw's
// search, clamps and placement (sm_wave_search, sr_mass_within, sr_place); a cell's mass is formed again in the search's second pass
// from the same numbers by the same expression.  The hat cell and values of the rounded x_k go to work space, where k_sqr_step finds
// them.  first also checks the sample's uniforms and clears its state; last writes logq and, for a failed sample, the row of NaN in
// x and of zeros in cell.
__global__ __launch_bounds__(256) void k_sqr_pick(int n, int k, int d, SrMode M, const int *held, const double *nodes, const double *gk, const double *S, const double *Cs,
                                                  SqrState st, long long npts, const double *u, int first, int last, double *xo, int *cell, double *logq)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const double *t = nodes + M.noff;
    for (long long p = (long long)blockIdx.x * nw + wave; p < npts; p += (long long)gridDim.x * nw) {
        bool fail;
        double lq = 0.0;
        if (first) fail = sm_bad_u(u + (size_t)p * d, d, lane, [&](int i) { return held[i] != 0; }, (double *)nullptr);
        else { fail = st.fail[p] != 0; lq = st.lq[p]; }
        int ci = M.cell, cj = -1;
        double f0 = M.phi0, f1 = M.phi1, xk = M.xh;
        if (!fail && !M.held) sqr_pick_one(n, t, gk[0], S + (size_t)p * n, Cs + (size_t)p * n, u[(size_t)p * d + k], lane, fail, lq, ci, cj, f0, f1, xk);
        if (lane == 0) {
            st.fail[p] = fail ? 1 : 0; st.lq[p] = lq;
            if (!fail) {
                st.ci[p] = ci; st.f0[p] = f0; st.f1[p] = f1;
                xo[(size_t)p * d + k] = xk;
                if (cell) cell[(size_t)p * d + k] = cj + 1;
            }
            if (last && logq) logq[p] = fail ? __builtin_nan("") : lq;
        }
        if (last && fail)
            for (int i = lane; i < d; i += 64) { xo[(size_t)p * d + i] = __builtin_nan(""); if (cell) cell[(size_t)p * d + i] = 0; }
    }
}

// The way back (ttx_rosenblatt_sq_real), in k_sqr_pick's place and frame: one wave per point, grid-stride, one launch per mode.  The
// coordinate x_k is given; a held mode forms nothing and writes u_k = 0.0 and cell 0.  Otherwise the hat cell ci of x_k
// (sr_hat_cell; the wave's copy of x_k is made uniform first, so the search runs once on the scalar unit), its hat values by
// sr_place's expressions, the cell masses from the two sheets with lanes along j, one pass of running sums (sm_wave_before), the
// mass inside the cell (sqr_cdf) and the log term.  A coordinate that is NaN or outside [t_0, t_(n-1)], or a total that is 0, NaN or
// Inf, fails the point.  ci lies in 0 .. n - 2 whatever x_k holds and is clamped again before the sheets are read.  The hat cell
// and values go to work space, where k_sqr_step finds them.  first clears the point's state; last writes logq and, for a failed
// point, the row of NaN in u and of zeros in cell.
__global__ __launch_bounds__(256) void k_sqr_cdf(int n, int k, int d, SrMode M, const double *nodes, const double *gk, const double *S, const double *Cs, SqrState st,
                                                 long long npts, const double *x, int first, int last, double *uo, int *cell, double *logq)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const double *t = nodes + M.noff;
    const int nc = n - 1;
    for (long long p = (long long)blockIdx.x * nw + wave; p < npts; p += (long long)gridDim.x * nw) {
        bool fail = false;
        double lq = 0.0;
        if (!first) { fail = st.fail[p] != 0; lq = st.lq[p]; }
        int ci = M.cell, co = 0;
        double f0 = M.phi0, f1 = M.phi1, uk = 0.0;
        if (!fail && !M.held) {
            const double xk = lane_get(x[(size_t)p * d + k], 0);
            if (!(xk >= t[0] && xk <= t[n - 1])) fail = true;                   // NaN, or outside the box
            else {
                const double *Sc = S + (size_t)p * n, *Cc = Cs + (size_t)p * n;
                const double g = gk[0];
                ci = sr_hat_cell(t, n, xk);
                ci = ci < 0 ? 0 : ci > n - 2 ? n - 2 : ci;
                const double t0 = t[ci], t1 = t[ci + 1];
                f1 = (xk - t0) / (t1 - t0);
                f0 = 1.0 - f1;
                const SmBefore b = sm_wave_before(nc, ci, lane, [&](int j) { return sqr_mass(Sc, Cc, t, g, j, nc); });
                if (!(b.total > 0.0) || b.total == __builtin_inf()) fail = true;    // 0, NaN or Inf
                else {
                    double q0, qm, q1;
                    const double at = sqr_cell(Sc, Cc, t, g, ci, q0, qm, q1);
                    double in = (t1 - t0) * sqr_cdf(q0, qm, q1, f1);
                    in = in > 0.0 ? in : 0.0;
                    in = in < at ? in : at;
                    uk = (b.before + in) / b.total;
                    uk = uk > 0.0 ? uk : 0.0;
                    uk = uk < 1.0 ? uk : 1.0;
                    co = ci + 1;
                    lq = lq + sqr_log_term(Sc, Cc, g, ci, f0, f1, b.total);
                }
            }
        }
        if (lane == 0) {
            st.fail[p] = fail ? 1 : 0; st.lq[p] = lq;
            if (!fail) {
                st.ci[p] = ci; st.f0[p] = f0; st.f1[p] = f1;
                uo[(size_t)p * d + k] = uk;
                if (cell) cell[(size_t)p * d + k] = co;
            }
            if (last && logq) logq[p] = fail ? __builtin_nan("") : lq;
        }
        if (last && fail)
            for (int i = lane; i < d; i += 64) { uo[(size_t)p * d + i] = __builtin_nan(""); if (cell) cell[(size_t)p * d + i] = 0; }
    }
}

// The chain step of mode k, one wave per sample: z = (0.0 + f0 A0 x) + f1 A1 x (sr_chain_step) with the hat cell and values
// k_sqr_pick left in work space; the cell is range-checked again here where it is read.  A failed sample is skipped.  last writes val.
__global__ __launch_bounds__(256) void k_sqr_step(const double *G, int RM, size_t SS, int r0, int r1, int n, SqrState st, const double *Xo, double *Xn, int ldx,
                                                  long long npts, int last, double *val)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (long long p = (long long)blockIdx.x * nw + wave; p < npts; p += (long long)gridDim.x * nw) {
        const bool fail = st.fail[p] != 0;
        double *z = Xn + (size_t)p * ldx;
        if (!fail) sqr_step_one(G, RM, SS, r0, r1, n, st.ci[p], st.f0[p], st.f1[p], Xo + (size_t)p * ldx, z, lane);
        if (last && val && lane == 0) val[p] = fail ? 0.0 : z[0];
    }
}
#endif
