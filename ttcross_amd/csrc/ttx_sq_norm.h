// ttx_sq_norm.h -- the normaliser Z = <f, f>_M of the squared density of the resident train, its logarithm and its gradient with
// respect to the cores (ttx_sq_lognorm_grad), and the point kernel of the negative log-likelihood (ttx_sq_nll_batch).
//
// The definition is in include/ttx.h; tests/sq_norm_ref.py restates it in numpy.  M_k is symmetric tridiagonal, diagonal md, off-diagonal
// mo (null: a diagonal matrix).  V_k = U_k x_2 M_k is never stored: sqn_stencil forms an entry where it is read, terms i-1, i, i+1.
//   right chain, k = d .. 2   k_sqn_w   Y(b, i, a') = sum_b' PR_k(b, b') V_k(a', i, b')            ascending b' from 0.0
//                             k_sqn_p   p_i(a, a') = sum_b U_k(a, i, b) Y(b, i, a')                 ascending b from 0.0, every i on workgroups of its own
//                             k_sqn_pow2  PR_(k-1) = sum_i p_i, ascending i from 0.0, times the power of two that takes the largest
//                                       entry into [0.5, 1); every PR_k is kept
//   left chain, k = 1 .. d    k_sqn_w   W_k(a, i, b') = sum_a' PL_(k-1)(a, a') V_k(a', i, b')       ascending a' from 0.0; every W_k is kept,
//                             k_sqn_p   p_i(b, b') = sum_a U_k(a, i, b) W_k(a, i, b')               in the packed layout of g
//                             k_sqn_pow2  PL_k as above; PL_d is the mantissa of Z, the summed exponents its exponent
// A chain step is three short, wide launches; the two chains are sequential in k and launch-bound on the trains measured.
//   assembly, all cores in one launch: D_k(a, i, b) = sum_b' W_k(a, i, b') PR_k(b, b'), G_k = G0_k + s_k * D_k with the host's
//                             s_k = ldexp((2 * coef) / (z_mant + gvol 2^-z_exp), eL(k-1) + eR(k) - z_exp)
//     k_sqn_asm<false>  one thread per element, ascending b' from 0.0: the bits of the restatement
//     k_sqn_asm<true>   D_k^T = PR_k W_k^T on v_mfma_f64_16x16x4_f64.  A workgroup owns TTX_SQN_ROWS = 128 rows (a, i) of one core and all
//                       its columns b; a wave owns two row tiles of 16.  PR_k goes through LDS in chunks of TTX_SQN_KC = 16 columns b'
//                       (row stride TTX_SQN_LDA = 144 doubles: the rows of a half-wave's two k fall into different halves of the banks);
//                       W is read from memory once, 16 consecutive rows per k: 128-byte rows, as are the stores.  The product is formed
//                       transposed so that the result's lanes l & 15 run along the rows (a, i), the contiguous direction of g.
//                       A operand PR_k(16 m + (l & 15), k0 + 4 s + (l >> 4)), B operand W_k(row0 + (l & 15), k0 + 4 s + (l >> 4)); rows past
//                       r0 n, columns past r1 and steps past r1 are zero-filled operands whose results are never stored.
// The chains run the same kernels in both modes: their cost is the launches, not the products (profiles/sq_norm_mi355x.txt).  No
// floating-point atomics and no sum whose order depends on the grid: a call repeats bit for bit.  Every element of g is written once.
// Every index comes from the shapes.
#pragma once

#define TTX_SQN_ROWS 128            // rows (a, i) of a workgroup of k_sqn_asm<true>: 4 waves x 2 tiles of 16
#define TTX_SQN_KC 16               // columns b' of PR_k per staged chunk
#define TTX_SQN_LDA 144             // row stride of the staged chunk in LDS (doubles)

struct SqnCore {                    // one core of the assembly launch
    const double *W, *PR;           // W_k (packed, r0 n x r1) and PR_k (r1 x r1, compact)
    double *G;                      // the core's block of g
    long long first;                // <false>: first element of the launch it owns; <true>: first workgroup
    int r0, n, r1, pad;
    double s;                       // s_k
};

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "ttx_ttops.h"     // dbl4

// (U x_2 M)(., i, .) at the element whose fibre starts at u (index stride RM): from 0.0, the terms i-1, i, i+1, multiply and add separate
__device__ inline double sqn_stencil(const double *u, int RM, int i, int n, const double *md, const double *mo)
{
    double t = 0.0;
    if (mo && i > 0) t = t + mo[i - 1] * u[(size_t)RM * (i - 1)];
    t = t + md[i] * u[(size_t)RM * i];
    if (mo && i + 1 < n) t = t + mo[i] * u[(size_t)RM * (i + 1)];
    return t;
}

// O(q, i, p) = sum_q' P(q, q') V(q', i, p), ascending q' from 0.0.  The core's contracted rank index q has element stride sq and Q
// values, the other rank index p has stride sp; P is Q x Q compact, O compact at q + Q (i + n p).  One workgroup per (i, p), threads
// along q (Q <= 128); V(:, i, p) goes through LDS.
__global__ __launch_bounds__(128) void k_sqn_w(const double *U, int RM, size_t sq, size_t sp, int Q, int n, const double *md, const double *mo, const double *P, double *O)
{
    __shared__ double v[128];
    const int i = blockIdx.x % n, p = blockIdx.x / n, q = threadIdx.x;
    if (q < Q) v[q] = sqn_stencil(U + sq * (size_t)q + sp * (size_t)p, RM, i, n, md, mo);
    __syncthreads();
    if (q >= Q) return;
    double s = 0.0;
#pragma unroll 4
    for (int t = 0; t < Q; t++) s = s + P[q + (size_t)Q * t] * v[t];
    O[q + (size_t)Q * (i + (size_t)n * p)] = s;
}

// Part_i(p, p') = sum_q U(q, i, p) O(q, i, p'), ascending q from 0.0, for the index i = blockIdx.z; q, p, sq, sp and Q as in k_sqn_w, R
// the values of p.  Part_i is R x R compact at Part + i R R.  A workgroup owns 16 x 16 elements of one i and walks the sum in LDS tiles
// of 16 q: every index has workgroups of its own, so a step is as wide as the core is long.
__global__ __launch_bounds__(256) void k_sqn_p(const double *U, int RM, size_t sq, size_t sp, int Q, int R, const double *O, int n, double *Part)
{
    __shared__ double gs[16][17], ws[16][17];
    const int t = threadIdx.x, lo = t & 15, hi = t >> 4, b0 = 16 * blockIdx.x, c0 = 16 * blockIdx.y, i = blockIdx.z;
    double s = 0.0;
    for (int q0 = 0; q0 < Q; q0 += 16) {
        const int q = q0 + lo;
        if (q0) __syncthreads();
        gs[hi][lo] = (q < Q && b0 + hi < R) ? U[sq * (size_t)q + (size_t)RM * i + sp * (size_t)(b0 + hi)] : 0.0;
        ws[hi][lo] = (q < Q && c0 + hi < R) ? O[q + (size_t)Q * (i + (size_t)n * (c0 + hi))] : 0.0;
        __syncthreads();
        const int nq = min(16, Q - q0);
        for (int x = 0; x < nq; x++) s = s + gs[lo][x] * ws[hi][x];
    }
    if (b0 + lo < R && c0 + hi < R) Part[(size_t)i * R * R + (b0 + lo) + (size_t)R * (c0 + hi)] = s;
}

// P = sum_i Part_i, ascending i from 0.0, then P <- P 2^(-ex), ex the exponent that takes max |P| into [0.5, 1) (0 where that maximum
// is 0 or not finite: k_sq_pow2's rule); ecum[0] = ein[0] + ex, the exponent of all factors so far.  P has M entries.  One workgroup.
__global__ __launch_bounds__(1024) void k_sqn_pow2(int M, int n, const double *Part, double *P, const int *ein, int *ecum)
{
    __shared__ double red[1024];
    double m = 0.0;
    bool bad = false;
    for (int q = threadIdx.x; q < M; q += 1024) {
        double s = 0.0;
#pragma unroll 4
        for (int i = 0; i < n; i++) s = s + Part[(size_t)i * M + q];
        P[q] = s;
        const double v = fabs(s);
        bad |= !(v <= 1.7976931348623157e308);
        m = v > m ? v : m;
    }
    red[threadIdx.x] = bad ? __builtin_inf() : m;
    __syncthreads();
    for (int o = 512; o; o >>= 1) { if ((int)threadIdx.x < o) { const double v = red[threadIdx.x + o]; if (v > red[threadIdx.x]) red[threadIdx.x] = v; } __syncthreads(); }
    m = red[0];
    int ex = 0;
    if (m > 0.0 && m <= 1.7976931348623157e308) (void)frexp(m, &ex);
    for (int q = threadIdx.x; q < M; q += 1024) P[q] = ldexp(P[q], -ex);         // every thread scales the entries it wrote itself
    if (threadIdx.x == 0) ecum[0] = ein[0] + ex;
}
// the starts of the chains: P = [1], exponent 0
__global__ void k_sqn_init(double *PL0, double *PRd, int *eL0, int *eRd)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { PL0[0] = 1.0; PRd[0] = 1.0; eL0[0] = 0; eRd[0] = 0; }
}

// the workgroup's (the element's) core by bisection over SqnCore::first
__device__ inline int sqn_find(const SqnCore *cs, int d, long long x)
{
    int lo = 0, hi = d - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (cs[mid].first <= x) lo = mid; else hi = mid - 1; }
    return lo;
}

template <bool MFMA, int MR>
__global__ __launch_bounds__(256) void k_sqn_asm(const SqnCore *cs, int d, long long tot, int acc)
{
    if (!MFMA) {
        for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long long)gridDim.x * blockDim.x) {
            const SqnCore C = cs[sqn_find(cs, d, e)];
            const long long t = e - C.first, rows = (long long)C.r0 * C.n;
            const long long row = t % rows;
            const int b = (int)(t / rows);
            double s = 0.0;
#pragma unroll 4
            for (int q = 0; q < C.r1; q++) s = s + C.W[row + rows * q] * C.PR[b + (size_t)C.r1 * q];
            const double g0 = acc ? C.G[t] : 0.0;
            C.G[t] = g0 + C.s * s;
        }
    } else {
        __shared__ double As[TTX_SQN_KC * TTX_SQN_LDA];
        const SqnCore C = cs[sqn_find(cs, d, (long long)blockIdx.x)];
        const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, col = l & 15, kq = l >> 4;
        const long long rows = (long long)C.r0 * C.n, row0 = ((long long)blockIdx.x - C.first) * TTX_SQN_ROWS + 32 * wave;
        const int r1 = C.r1, rp = (r1 + 15) & ~15;
        dbl4 a[2][MR];
#pragma unroll
        for (int rt = 0; rt < 2; rt++)
#pragma unroll
            for (int m = 0; m < MR; m++) a[rt][m] = dbl4{0.0, 0.0, 0.0, 0.0};
        const long long rw[2] = {row0 + col, row0 + 16 + col};
        const bool ok[2] = {rw[0] < rows, rw[1] < rows};
        for (int k0 = 0; k0 < r1; k0 += TTX_SQN_KC) {
            if (k0) __syncthreads();
            for (int e = tid; e < TTX_SQN_KC * 128; e += 256) {
                const int kk = e >> 7, b = e & 127;
                As[kk * TTX_SQN_LDA + b] = (b < r1 && k0 + kk < r1) ? C.PR[b + (size_t)r1 * (k0 + kk)] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int st = 0; st < TTX_SQN_KC / 4; st++) {
                const int kk = 4 * st + kq, k = k0 + kk;
                const double w0 = (ok[0] && k < r1) ? C.W[rw[0] + rows * k] : 0.0, w1 = (ok[1] && k < r1) ? C.W[rw[1] + rows * k] : 0.0;
#pragma unroll
                for (int m = 0; m < MR; m++) {
                    if (16 * m < rp) {
                        const double pr = As[kk * TTX_SQN_LDA + 16 * m + col];
                        a[0][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(pr, w0, a[0][m], 0, 0, 0);
                        a[1][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(pr, w1, a[1][m], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int rt = 0; rt < 2; rt++) {
            if (!ok[rt]) continue;
#pragma unroll
            for (int m = 0; m < MR; m++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int b = 16 * m + kq + 4 * reg;
                    if (b < r1) {
                        double *g = C.G + rw[rt] + rows * b;
                        const double g0 = acc ? *g : 0.0;
                        *g = g0 + C.s * a[rt][m][reg];
                    }
                }
        }
    }
}

// the point kernel of ttx_sq_nll_batch: wv = w (null: 1.0), one = 1.0, den = val * val + gamma, c = -((2 * wv) * val) / den, lt = log(den)
__global__ __launch_bounds__(256) void k_sqn_points(long long npts, const double *val, const double *w, double gamma, double *c, double *lt, double *wv, double *one)
{
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npts; p += (long long)gridDim.x * blockDim.x) {
        const double v = val[p], ww = w ? w[p] : 1.0, den = v * v + gamma;
        c[p] = -((2.0 * ww) * v) / den;
        lt[p] = log(den);
        wv[p] = ww;
        one[p] = 1.0;
    }
}
#endif
