// ttx_sample_real.h -- real-valued samples drawn from the piecewise-linear interpolant of the resident train of grid values
// (ttx_sample_real / ttx_sample_real_dev): the inverse Rosenblatt transform of the interpolant, the conditional-distribution
// sampler of Dolgov, Anaya-Izquierdo, Fox and Scheichl (2020) on the nodal conditionals.
//
// The definition is in include/ttx.h.  Everything up to the head tables is ttx_sample's (ttx_sample.h): k_ct_modesum and
// k_ct_chains form the prefix vectors from the effective weights (trapezoid weights of a drawn mode, the hat row of a held one),
// k_sm_head the head tables with weights of 1.0.  Then
//   k_sr_draw   one wave per sample: per drawn mode the row p(i) = |sum_b H_k(i, b) x(b)| with lanes along i, the cell masses
//               A(j) = (0.5 (p(j) + p(j+1))) h_j with lanes along j, the search for the cell (sm_wave_search, ttx_sample.h), the
//               root of the quadratic inside the cell (sr_invert), the placement of x (sr_place), and the two-term chain step with the hat row of the rounded coordinate;
//               the chain ends exactly where k_bs_exact (ttx_basis.h) would: val is the interpolant at x
//   k_sr_count  the failed samples of a chunk (their rows of x start with a NaN), added to the call's counter by one workgroup
// The first part of this file is plain C++ a host compiler accepts (tests/sample_real_main.cpp runs it on the CPU).
// Open: a direct COS-basis sampler (root finding on a density that may go negative; for a signed train ttx_sample_sq_real draws from the squared interpolant), an MFMA
// path for the rows of p, extra per-mode weights, ranks above 128.
#pragma once
#include <math.h>
#include <stddef.h>
#include "ttx_basis.h"     // ttx_basis_entry: host and device
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TTX_SR_HD __host__ __device__ inline
#else
#define TTX_SR_HD static inline
#endif

// lambda in [0, 1] with p0 lambda + (p1 - p0) lambda^2 / 2 = sp: the position inside a cell whose density runs linearly from p0 to
// p1 (both >= 0) at which the mass per unit length sp = s / h is reached, 0 <= sp <= (p0 + p1) / 2.  The root is taken in the form
// 2 sp / (p0 + sqrt(p0^2 + 2 D sp)), which has no cancellation for either sign of D.  The three numbers are first scaled by the power
// of two that takes max(p0, p1) into [0.5, 1): lambda has no scale, the scaling is exact, and wherever the plain formula neither
// under- nor overflows (p0^2 does below 1e-154 and above 1e154) the bits are the same.  Anything that is not a number ends as 0.
TTX_SR_HD double sr_invert(double p0, double p1, double sp)
{
    const double m = p0 > p1 ? p0 : p1;
    if (!(m > 0.0) || m > 1.7976931348623157e308) return 0.0;
    int e;
    (void)frexp(m, &e);
    p0 = ldexp(p0, -e); p1 = ldexp(p1, -e); sp = ldexp(sp, -e);
    const double D = p1 - p0;
    double disc = p0 * p0 + (2.0 * D) * sp;
    disc = disc > 0.0 ? disc : 0.0;
    const double den = p0 + sqrt(disc);
    double l = den > 0.0 ? (2.0 * sp) / den : 0.0;
    l = l > 1.0 ? 1.0 : l;
    return l >= 0.0 ? l : 0.0;
}

// trapezoid weights of n strictly ascending nodes: om(0) = 0.5 (t_1 - t_0), om(i) = 0.5 (t_(i+1) - t_(i-1)), om(n-1) = 0.5 (t_(n-1) -
// t_(n-2)).  A single node carries the weight 1.0: such a mode is a point, held at its node.
TTX_SR_HD void sr_trapezoid(const double *t, int n, double *om)
{
    if (n == 1) { om[0] = 1.0; return; }
    om[0] = 0.5 * (t[1] - t[0]);
    for (int i = 1; i < n - 1; i++) om[i] = 0.5 * (t[i + 1] - t[i - 1]);
    om[n - 1] = 0.5 * (t[n - 1] - t[n - 2]);
}

// the cell of TTX_BASIS_LINEAR's rule for a coordinate x that is a number: 0 for x <= t_0, n - 2 for x >= t_(n-1), otherwise the last
// node with t_i <= x; always in 0 .. max(n - 2, 0).  The row's nonzero entries are those of the nodes i and i + 1.
TTX_SR_HD int sr_hat_cell(const double *t, int n, double x)
{
    int lo = 0, hi = n - 2;                     // invariant: the answer lies in lo .. hi
    while (lo < hi) { const int m = (lo + hi + 1) >> 1; if (t[m] <= x) lo = m; else hi = m - 1; }
    return lo > 0 ? lo : 0;
}

// one mode as k_sr_draw, k_sqr_pick and k_sqr_step take it.  held != 0: the mode is not drawn, its coordinate xh, cell and the two hat
// values were formed on the host (ttx_basis_entry, the function of ttx_basis_host).  noff: where the mode's nodes start in the call's
// node block
struct SrMode { int held, cell; double phi0, phi1, xh; size_t noff; };

// the record of a mode of n nodes t held at the coordinate x (a number): TTX_BASIS_LINEAR's cell and its two hat values, entry by entry
// from ttx_basis_entry (a mode of one node has the first only)
TTX_SR_HD SrMode sr_held_mode(const double *t, int n, double x, size_t noff)
{
    SrMode M{1, sr_hat_cell(t, n, x), 0.0, 0.0, x, noff};
    M.phi0 = ttx_basis_entry(2, 0, 0.0, 0.0, t, n, x, M.cell);                  // kind 2: TTX_BASIS_LINEAR
    M.phi1 = n > 1 ? ttx_basis_entry(2, 0, 0.0, 0.0, t, n, x, M.cell + 1) : 0.0;
    return M;
}

#if defined(__HIPCC__)
#include "ttx_sample.h"    // TTX_SM_LDSROW, sm_wave_search, k_sm_head

// z = (0.0 + f0 A0 x) + f1 A1 x for the slices A0 = G(:, i, :) and A1 = G(:, i + 1, :) (two; a mode of one node has the first term
// only).  Both products are k_ev_exact's: sums from 0.0 over ascending b, separate multiply and add, two rows per lane above rank 64
__device__ inline void sr_chain_step(const double *A, size_t RM, size_t SS, int q0, int q1, bool two, double f0, double f1, const double *x, double *z, int lane)
{
    const double *B = two ? A + RM : A;
    if (q0 <= 64) {
        if (lane < q0) {
            double s = 0.0, t = 0.0;
#pragma unroll 4
            for (int k = 0; k < q1; k++) { const double xk = x[k]; s = s + A[lane + SS * k] * xk; t = t + B[lane + SS * k] * xk; }
            double v = 0.0 + f0 * s;
            if (two) v = v + f1 * t;
            z[lane] = v;
        }
    } else {
        const bool hi = lane + 64 < q0;
        const int o = hi ? 64 : 0;
        double s0 = 0.0, s1 = 0.0, t0 = 0.0, t1 = 0.0;
#pragma unroll 2
        for (int k = 0; k < q1; k++) {
            const double xk = x[k];
            s0 = s0 + A[lane + SS * k] * xk; s1 = s1 + A[lane + o + SS * k] * xk;
            t0 = t0 + B[lane + SS * k] * xk; t1 = t1 + B[lane + o + SS * k] * xk;
        }
        double v0 = 0.0 + f0 * s0, v1 = 0.0 + f0 * s1;
        if (two) { v0 = v0 + f1 * t0; v1 = v1 + f1 * t1; }
        z[lane] = v0;
        if (hi) z[lane + 64] = v1;
    }
}

// the mass to invert inside the cell a search has hit: t minus the running sum before the cell, clamped into [0, the cell's mass]
__device__ inline double sr_mass_within(const SmFound &f)
{
    double s = f.t - f.before;
    s = s > 0.0 ? s : 0.0;
    return s < f.at ? s : f.at;
}

// x = t_cj + lam h_cj placed into the closed cell cj before the hat row is looked up; ci: TTX_BASIS_LINEAR's cell of the rounded x (it may
// be the next one, capped at n - 2), f0 and f1: the two hat values of x there
__device__ inline double sr_place(const double *t, int n, int cj, double lam, int &ci, double &f0, double &f1)
{
    const double tl = t[cj], tr = t[cj + 1];
    double xk = tl + lam * (tr - tl);
    xk = xk > tl ? xk : tl;
    xk = xk < tr ? xk : tr;
    ci = cj + ((cj + 1 <= n - 2 && xk >= tr) ? 1 : 0);
    const double t0 = t[ci], t1 = t[ci + 1];
    f1 = (xk - t0) / (t1 - t0);
    f0 = 1.0 - f1;
    return xk;
}

// One wave per sample, grid-stride, in the frame of k_sm_draw.  Dynamic LDS per wave: x[ldx], z[ldx], the sample's row of u [d], its
// coordinates [d], its cell row [d] and the row of p of the current mode [ldsrow]; nothing is shared between waves, so there is no
// workgroup barrier.  A mode longer than ldsrow keeps its row in grow (growlen doubles per wave of the grid).  The row is complete,
// behind a wave barrier, before the cells are formed: cell j reads p(j) and p(j+1).  A cell index comes from lane numbers alone,
// the hat cell is that index or the next, capped at n - 2: whatever cores and u hold, every read stays inside its table.
__global__ __launch_bounds__(256) void k_sr_draw(EvTrain T, const size_t *hoff, const SrMode *modes, const double *nodes, const double *H, int ldsrow, double *grow,
                                                 size_t growlen, long long npts, const double *u, double *xo, int *cell, double *logq, double *val)
{
    extern __shared__ __align__(16) double sr_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, d = T.d;
    const size_t per = 2 * (size_t)T.ldx + 2 * (size_t)d + (((size_t)d + 1) >> 1) + ldsrow;
    double *xb = sr_dyn + per * wave, *us = xb + 2 * T.ldx, *xs = us + d, *lrow = xs + d + (((size_t)d + 1) >> 1);
    int *id = (int *)(xs + d);
    double *wrow = grow ? grow + growlen * ((size_t)blockIdx.x * nw + wave) : nullptr;
    for (long long p = (long long)blockIdx.x * nw + wave; p < npts; p += (long long)gridDim.x * nw) {
        double *x = xb, *z = xb + T.ldx;
        __builtin_amdgcn_wave_barrier();
        bool fail = sm_bad_u(u + (size_t)p * d, d, lane, [&](int i) { return modes[i].held != 0; }, us);
        if (lane == 0) x[0] = 1.0;                                              // x_(d+1) = [1]
        double lq = 0.0;
        __builtin_amdgcn_wave_barrier();
        for (int k = d - 1; k >= 0 && !fail; k--) {
            const int q0 = T.r[k], q1 = T.r[k + 1], n = T.n[k];
            const SrMode M = modes[k];
            int ci = M.cell, cj = -1;
            double f0 = M.phi0, f1 = M.phi1, xk = M.xh;
            if (!M.held) {
                const double *Hk = H + hoff[k], *t = nodes + M.noff;
                double *row = n <= ldsrow ? lrow : wrow;
                const int nc = n - 1;                                           // cells; a drawn mode has n >= 2
                for (int i = lane; i < n; i += 64) {                            // the row of p
                    double m = 0.0;
#pragma unroll 4
                    for (int b = 0; b < q1; b++) m = m + Hk[(size_t)b * n + i] * x[b];
                    row[i] = fabs(m);
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const auto mass = [&](int j) { return j < nc ? (0.5 * (row[j] + row[j + 1])) * (t[j + 1] - t[j]) : 0.0; };   // the cell masses A(j)
                const SmFound f = sm_wave_search(nc, us[k], lane, mass, mass);
                if (!f.ok) { fail = true; break; }
                cj = f.pos;
                const double lam = f.hit ? sr_invert(row[cj], row[cj + 1], sr_mass_within(f) / (t[cj + 1] - t[cj])) : 1.0;
                xk = sr_place(t, n, cj, lam, ci, f0, f1);
                lq = lq + log((f0 * row[ci] + f1 * row[ci + 1]) / f.total);
            }
            if (lane == 0) { id[k] = cj + 1; xs[k] = xk; }
            sr_chain_step(T.core[k] + (size_t)T.RM * ci, (size_t)T.RM, T.SS, q0, q1, n > 1, f0, f1, x, z, lane);
            __builtin_amdgcn_wave_barrier();
            double *t_ = x; x = z; z = t_;
        }
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < d; i += 64) {
            xo[(size_t)p * d + i] = fail ? __builtin_nan("") : xs[i];
            if (cell) cell[(size_t)p * d + i] = fail ? 0 : id[i];
        }
        if (lane == 0) {
            if (logq) logq[p] = fail ? __builtin_nan("") : lq;
            if (val) val[p] = fail ? 0.0 : x[0];
        }
    }
}

// cnt[0] += samples of the chunk whose row of x starts with a NaN (the failed ones); one workgroup, launched chunk after chunk on one stream
__global__ __launch_bounds__(1024) void k_sr_count(long long npts, int d, const double *xo, long long *cnt)
{
    __shared__ long long part[1024];
    long long s = 0;
    for (long long p = threadIdx.x; p < npts; p += 1024) { const double v = xo[(size_t)p * d]; s += v != v; }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 512; o; o >>= 1) { if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) cnt[0] += part[0];
}
#endif
