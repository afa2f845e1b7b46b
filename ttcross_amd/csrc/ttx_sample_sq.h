// ttx_sample_sq.h -- samples drawn from the SQUARE of the resident tensor train (ttx_sample_sq / ttx_sample_sq_dev): the squared-
// density sampler (SIRT) of Cui and Dolgov (2022) on grid indices.  Every conditional is a sum of squares, so it is non-negative
// whatever the signs of the cores.
//
// The definition is in include/ttx.h.  Modes are drawn from the last to the first with dtt_ijk's chain as the state, as in
// ttx_sample.h.  Per call, one left-to-right pass (the head: ort_impl's loop with H_k kept instead of Q; the train is only read):
//   gemm               H_k = F_(k-1) times the unfolded core k (k_gemm_mfma)
//   k_sq_split         H_k into its table, i contiguous: (a, i, b) at i + n (a + l b), r_k padded to four with zeros; the rows sqrt(e_k(i)) H_k(a, i, :) for the QR
//   qr()               the R factor where the matrix has more rows than columns
//   k_sq_pow2          F_k = R (or the matrix itself) times the power of two that takes its largest entry into [0.5, 1); the
//                      running exponent and the defensive term g of the next mode in the scaled units
// and per chunk and per mode k = d .. 1:
//   k_sq_rows_mfma / _exact   s(c, i) = sum_a (sum_b H_k(a, i, b) x_c(b))^2 to the sheet [chunk][n_k]
//   k_sq_pick          one wave per sample: p = w (s + g), the scan and the search (ttx_sample.h's device functions); logq and
//                      the failure flag of a sample stay in work space between the launches
//   k_sq_step          one wave per sample: the chain step of the picked index (sm_chain_step); the states stay in work space
// then k_sm_count (ttx_sample.h) counts the failed samples.  No atomics and no sum whose order depends on the grid, the chunk or
// the other samples: a call repeats bit for bit.  Every index comes from lane numbers and counts, never from a value.
// The real-valued variant (squared interpolant, mass-matrix factors, a cubic CDF inversion per cell) is ttx_sample_sq_real.h; it
// reuses sq_head's tables.  Open: per-sample weights; ranks above 128.
// The first part of this file is plain C++ a host compiler accepts (tests/sample_sq_main.cpp runs it on the CPU).
#pragma once
#include <math.h>
#include <stddef.h>
#include <vector>

// the call's plan: the rows of the factors, where the tables start, the flops of the rows per sample
struct SqPlan {
    std::vector<int> l;                     // l[k], k = 0 .. d: the rows of F_k, l[0] = 1, l[k] = min(l[k-1] n_k, r_k)
    std::vector<size_t> hoff, foff, woff;   // 0-based mode k: H_(k+1) (l[k] x n_k x r_(k+1) padded to four) starts at hoff[k], F_k (l[k] x r_k) at
                                            // foff[k], the mode's weights at woff[k]; entry d: the totals
    double flops = 0.0;                     // 2 sum n_k l_(k-1) r_k over the drawn modes
    int rmax = 1, nmax = 1;
};
// n[0 .. d-1], r[0 .. d], fx[k] != 0: mode k is held
inline void sq_plan(int d, const int *n, const int *r, const int *fx, SqPlan &P)
{
    P.l.assign(d + 1, 1); P.hoff.assign(d + 1, 0); P.foff.assign(d + 1, 0); P.woff.assign(d + 1, 0);
    P.flops = 0.0; P.rmax = r[0] > 1 ? r[0] : 1; P.nmax = 1;
    for (int k = 1; k <= d; k++) {
        const int nk = n[k - 1], r1 = r[k], r1p = (r1 + 3) & ~3;
        const long long ln = (long long)P.l[k - 1] * nk;
        P.l[k] = (int)(ln < r1 ? ln : r1);
        P.hoff[k] = P.hoff[k - 1] + (size_t)P.l[k - 1] * nk * r1p;              // slabs of zeros up to a multiple of four
        P.foff[k] = P.foff[k - 1] + (size_t)P.l[k - 1] * r[k - 1];
        P.woff[k] = P.woff[k - 1] + (size_t)nk;
        if (!fx[k - 1]) P.flops += 2.0 * nk * P.l[k - 1] * r1;
        if (r1 > P.rmax) P.rmax = r1;
        if (nk > P.nmax) P.nmax = nk;
    }
}
// the first weight that is not a finite number >= 0 (its square root enters), -1 if there is none
inline long long sq_bad_weight(const double *w, size_t count)
{
    for (size_t j = 0; j < count; j++) if (!(w[j] >= 0.0) || !(w[j] <= 1.7976931348623157e308)) return (long long)j;
    return -1;
}
// eff: the effective weights of all modes (w, or ones for w = null; a held mode has the unit vector of its index fx[k], 1-based);
// gw[k], k = 0 .. d: gamma prod_(j < k) W_j with W_j the sum of a drawn mode's weights over ascending i from 0.0, 1 for a held one
inline void sq_effective(int d, const int *n, const int *fx, const double *w, double gamma, std::vector<double> &eff, std::vector<double> &gw)
{
    size_t total = 0;
    for (int k = 0; k < d; k++) total += (size_t)n[k];
    eff.assign(total, 1.0); gw.assign(d + 1, gamma);
    if (w) for (size_t j = 0; j < total; j++) eff[j] = w[j];
    size_t o = 0;
    for (int k = 0; k < d; k++) {
        double W = 1.0;
        if (fx[k]) { for (int i = 0; i < n[k]; i++) eff[o + i] = i == fx[k] - 1 ? 1.0 : 0.0; }
        else { W = 0.0; for (int i = 0; i < n[k]; i++) W = W + eff[o + i]; }
        gw[k + 1] = gw[k] * W;
        o += (size_t)n[k];
    }
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "ttx_sample.h"    // sm_chain_step, wave_scan, k_sm_count
#include "ttx_ttops.h"     // dbl4

// TTX_EVAL_AUTO forms the rows on the matrix cores from this many flops per call on (2 sum_k npts n_k l_(k-1) r_k).  Measured on the
// D_64 train (profiles/sample_sq_mi355x.txt): EXACT and MFMA tie from 1.9e8 to 1.9e9 flops per call (launch-bound), MFMA is 1.6 times
// faster at 1.9e10 and 8 times at 6.3e12: the two part between 1.9e9 and 1.9e10
#define TTX_SQ_AUTO_FLOPS 3.0e9
#define TTX_SQ_SHEET (1ll << 28)    // largest sheet chunk x max n_k (doubles, 2 GiB)

// F_0 = [1] with no exponent, the defensive term of the first mode
__global__ void k_sq_init(double *F0, double *g0, int *st, double gamma)
{
    if (threadIdx.x == 0) { F0[0] = 1.0; g0[0] = gamma; st[0] = 0; }
}
// the state of the empty suffix, x = [1], for C samples
__global__ __launch_bounds__(256) void k_sq_ones(double *X, int ldx, int C)
{
    for (size_t c = (size_t)blockIdx.x * 256 + threadIdx.x; c < (size_t)C; c += (size_t)gridDim.x * 256) X[c * ldx] = 1.0;
}

// C is the l x (n r1) product of the gemm, (a, i, b) at a + l (i + n b).  H: the same numbers with i contiguous, and r1p - r1 slabs
// of zeros behind them (r1p = r1 rounded up to four: k_sq_rows_mfma's last step reads them).  A (null for the last mode): the rows
// sqrt(e(i)) C(a, i, :) in C's own layout, the (l n) x r1 matrix the QR takes.  sp (null for the grid sampler): e holds the diagonal dg
// of a bidiagonal factor as it is and the rows are dg(i) C(a, i, :) + sp(i) C(a, i+1, :) (ttx_sample_sq_real.h); sp(n-1) is not read
__global__ __launch_bounds__(256) void k_sq_split(const double *C, int l, int n, int r1, int r1p, const double *e, const double *sp, double *H, double *A)
{
    const size_t M = (size_t)l * n * r1p, M1 = (size_t)l * n * r1;
    for (size_t q = (size_t)blockIdx.x * 256 + threadIdx.x; q < M; q += (size_t)gridDim.x * 256) {
        const int a = (int)(q % l), i = (int)((q / l) % n), b = (int)(q / ((size_t)l * n));
        const double v = q < M1 ? C[q] : 0.0;
        H[i + (size_t)n * (a + (size_t)l * b)] = v;
        if (A && q < M1) A[q] = !sp ? sqrt(e[i]) * v : i + 1 < n ? e[i] * v + sp[i] * C[q + l] : e[i] * v;
    }
}

// F = R 2^(-ex) with ex the exponent that takes max |R| into [0.5, 1) (0 where that maximum is 0 or not finite).  R is rows x cols
// with leading dimension ldr, F compact.  st[0] (an int, the exponent of all factors so far) += ex; *gout = gw 2^(-2 st[0]): the
// defensive term of the next mode in the units of F.  One workgroup.
__global__ __launch_bounds__(1024) void k_sq_pow2(int rows, int cols, const double *R, int ldr, double *F, int *st, double gw, double *gout)
{
    __shared__ double red[1024];
    const int M = rows * cols;
    double m = 0.0;
    bool bad = false;
    for (int q = threadIdx.x; q < M; q += 1024) { const double v = fabs(R[(q % rows) + (size_t)ldr * (q / rows)]); bad |= !(v <= 1.7976931348623157e308); m = v > m ? v : m; }
    red[threadIdx.x] = bad ? __builtin_inf() : m;
    __syncthreads();
    for (int o = 512; o; o >>= 1) { if ((int)threadIdx.x < o) { const double v = red[threadIdx.x + o]; if (v > red[threadIdx.x]) red[threadIdx.x] = v; } __syncthreads(); }
    m = red[0];
    int ex = 0;
    if (m > 0.0 && m <= 1.7976931348623157e308) (void)frexp(m, &ex);
    for (int q = threadIdx.x; q < M; q += 1024) F[q] = ldexp(R[(q % rows) + (size_t)ldr * (q / rows)], -ex);
    if (threadIdx.x == 0) {
        const long long tot = (long long)st[0] + ex;
        st[0] = (int)tot;
        const long long sh = -2 * tot;
        *gout = ldexp(gw, (int)(sh > 100000 ? 100000 : sh < -100000 ? -100000 : sh));
    }
}

// EXACT: one thread per pair (c, i), grid-stride.  m(a) = sum_b H(a, i, b) x_c(b) over ascending b from 0.0, s = sum_a m(a)^2 over
// ascending a from 0.0, separate multiplies and adds.
__global__ __launch_bounds__(256) void k_sq_rows_exact(const double *H, int l, int n, int r1, const double *X, int ldx, int C, double *S)
{
    const long long M = (long long)C * n;
    for (long long q = (long long)blockIdx.x * 256 + threadIdx.x; q < M; q += (long long)gridDim.x * 256) {
        const int c = (int)(q / n), i = (int)(q % n);
        const double *x = X + (size_t)c * ldx, *Hi = H + i;
        double s = 0.0;
        for (int a = 0; a < l; a++) {
            double m = 0.0;
#pragma unroll 4
            for (int b = 0; b < r1; b++) m = m + Hi[(size_t)n * (a + (size_t)l * b)] * x[b];
            s = s + m * m;
        }
        S[q] = s;
    }
}

// MFMA: a workgroup owns 64 samples, 16 per wave, and the index tiles t0 .. t0 + tper - 1 of 16 indices; nothing is shared between
// the waves.  A wave keeps its X (r1 x 16, zero-filled) in KS registers per lane.  Per tile and per row a of the factor it forms
// Y_a(i, c) = sum_b H(a, i, b) X(b, c) on v_mfma_f64_16x16x4_f64 with the tile's 16 indices as the rows of the A operand -- the
// table is i contiguous, so an operand load is four runs of 128 bytes -- squares its four accumulators and adds them over
// ascending a in registers: the sum over a needs no shuffle and no LDS.  Lane maps as k_tk_score_mfma's: A[row l & 15][k l >> 4],
// B[k l >> 4][col l & 15], result row (l >> 4) + 4 reg, column l & 15.  Steps b >= r1 read the table's slabs of zeros and samples
// >= C are zero-filled.  A lane whose index is >= n loads index 0 instead: a row of the A operand enters its own row of the result
// only, and the rows >= n are never stored.  The loads carry no per-step predicate: offsets are 32-bit (a table has at most
// 128 n 128 < 2^31 entries).
template <int KS>
__global__ __launch_bounds__(256) void k_sq_rows_mfma(const double *H, int l, int n, int r1, const double *X, int ldx, int C, int tper, double *S)
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
    const int nt = (n + 15) >> 4, t1 = min(nt, (int)(blockIdx.x + 1) * tper);
    const unsigned ln_ = (unsigned)l * (unsigned)n;
    for (int t = blockIdx.x * tper; t < t1; t++) {
        const int ia = 16 * t + col;                                            // the index this lane loads for the A operand
        const double *Hi = H + (ia < n ? ia : 0);
        dbl4 sq = dbl4{0.0, 0.0, 0.0, 0.0};
        for (int a = 0; a < l; a++) {
            const double *Ha = Hi + (size_t)n * a;
            dbl4 acc = dbl4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ks = 0; ks < KS; ks++)
                if (4 * ks < r1) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ha[(unsigned)(4 * ks + kq) * ln_], xb[ks], acc, 0, 0, 0);
#pragma unroll
            for (int reg = 0; reg < 4; reg++) sq[reg] = sq[reg] + acc[reg] * acc[reg];
        }
        if (cok) {
#pragma unroll
            for (int reg = 0; reg < 4; reg++) { const int i = 16 * t + kq + 4 * reg; if (i < n) S[(size_t)c * n + i] = sq[reg]; }
        }
    }
}

// what a sample carries from one k_sq_pick to the next
struct SqState { double *lq; int *fail; };

__device__ inline double sq_p(const double *w, const double *Sc, double g, int i, int n) { return i < n ? w[i] * (Sc[i] + g) : 0.0; }

// One wave per sample, grid-stride, one launch per mode (0-based k).  ifix >= 0: the mode is held at that index and no p is formed.
// Otherwise p(i) = w(i) (s(i) + g) from the sheet with lanes along i, the scan, the total, the search and the log term exactly
// as in k_sm_draw; p is formed again in the search from the same numbers by the same expression.  Both kernels keep the loops
// written out, the cell samplers share them as sm_wave_search (ttx_sample.h says why).  The index goes to the sample's
// row of ind, where k_sq_step finds it.  first also checks the sample's uniforms and clears its state; last writes logq and, for
// a failed sample, the index row of zeros.  A failed sample is skipped by every later launch.
__global__ __launch_bounds__(256) void k_sq_pick(int n, int k, int d, int ifix, const int *fixed, const double *w, const double *gk, const double *S, SqState st,
                                                 long long npts, const double *u, int first, int last, int *ind, double *logq)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (long long p = (long long)blockIdx.x * nw + wave; p < npts; p += (long long)gridDim.x * nw) {
        bool fail;
        double lq = 0.0;
        if (first) {
            bool badu = false;
            for (int i = lane; i < d; i += 64) { const double uu = u[(size_t)p * d + i]; badu |= !fixed[i] && !(uu >= 0.0); }   // NaN or negative
            fail = __ballot(badu) != 0;
        } else { fail = st.fail[p] != 0; lq = st.lq[p]; }
        int ik = ifix;
        if (!fail && ik < 0) {
            const double *Sc = S + (size_t)p * n;
            const double uk = u[(size_t)p * d + k], g = gk[0];
            double carry = 0.0, plast = 0.0;
            int lastp = -1;
            for (int i0 = 0; i0 < n; i0 += 64) {                                // the total c(n)
                const double pi = sq_p(w, Sc, g, i0 + lane, n);
                carry = __shfl(carry + wave_scan(pi, lane), 63);
                const unsigned long long pos = __ballot(pi > 0.0);
                if (pos) { const int hl = 63 - __builtin_clzll(pos); lastp = i0 + hl; plast = __shfl(pi, hl); }
            }
            const double total = carry;
            if (!(total > 0.0) || total == __builtin_inf() || lastp < 0) fail = true;       // 0, NaN or Inf
            else {
                const double t = uk * total;
                double psel = plast;
                ik = lastp;                                                     // u >= 1, or no i with t < c(i): the largest i with p > 0
                if (uk < 1.0) {
                    carry = 0.0;
                    for (int i0 = 0; i0 < n; i0 += 64) {
                        const int i = i0 + lane;
                        const double pi = sq_p(w, Sc, g, i, n), c = carry + wave_scan(pi, lane);
                        const unsigned long long hit = __ballot(i < n && pi > 0.0 && t < c);
                        if (hit) { const int fl = __builtin_ctzll(hit); ik = i0 + fl; psel = __shfl(pi, fl); break; }
                        carry = __shfl(c, 63);
                    }
                }
                lq = lq + log(psel / total);
            }
        }
        if (lane == 0) {
            st.fail[p] = fail ? 1 : 0; st.lq[p] = lq;
            if (!fail) ind[(size_t)p * d + k] = ik + 1;
            if (last && logq) logq[p] = fail ? __builtin_nan("") : lq;
        }
        if (last && fail) for (int i = lane; i < d; i += 64) ind[(size_t)p * d + i] = 0;
    }
}

// The chain step of mode k, one wave per sample: Xn = G(:, i, :) Xo in TTX_EVAL_EXACT's operation sequence (sm_chain_step; first: the
// copy of k_ev_exact) with i the index k_sq_pick left in the sample's row of ind, range-checked again here where it is read.  A
// failed sample is skipped.  last writes val.
__global__ __launch_bounds__(256) void k_sq_step(const double *G, int RM, size_t SS, int r0, int r1, int n, int k, int d, const int *ind, const int *failed,
                                                 const double *Xo, double *Xn, int ldx, long long npts, int first, int last, double *val)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (long long p = (long long)blockIdx.x * nw + wave; p < npts; p += (long long)gridDim.x * nw) {
        const bool fail = failed[p] != 0;
        double *z = Xn + (size_t)p * ldx;
        if (!fail) {
            int ik = ind[(size_t)p * d + k] - 1;
            ik = ik < 0 ? 0 : ik >= n ? n - 1 : ik;
            const double *A = G + (size_t)RM * ik;
            if (first) { for (int a = lane; a < r0; a += 64) z[a] = A[a]; }     // x_d = G_d(:, i_d, 1), a copy as in k_ev_exact
            else sm_chain_step(A, SS, r0, r1, Xo + (size_t)p * ldx, z, lane);
        }
        if (last && val && lane == 0) val[p] = fail ? 0.0 : z[0];
    }
}
#endif
