// ttx_sq_moments.h -- moments and one-mode reduced density matrices of the squared density of the resident train (ttx_sq_moments).
//
// The definition is in include/ttx.h; tests/sq_moments_ref.py restates it in numpy.  The chains of ttx_sq_lognorm_grad (ttx_sq_norm.h) give
// every PL_k, PR_k and their exponents.  New here:
//   carried matrices  C^(k)_j: a left chain matrix with A_k inserted at mode k, taken through the modes j = k+1 .. with M_j.  All carried
//                     matrices of a mode go through one launch per kernel, the batch index c on the grid:
//     k_sqm_w / k_sqm_p / k_sqm_pow2   the three kernels of a chain step with a batch index, the operation order of k_sqn_w / k_sqn_p /
//                     k_sqn_pow2 for every member, one exponent per member.  They also run the unbatched steps of this call (the
//                     insertion of A_k, the right matrices RA_(l-1), T of the band) with a batch of one.
//     k_sqm_w_mfma    W^(c) = C^(c) V on v_mfma_f64_16x16x4_f64: the stacked batch against the one V = U x_2 M, which is formed where it is
//                     read (sqn_stencil).  A wave owns a 16 x 16 tile of one member; the product is formed transposed, so that the result's
//                     lanes l & 15 run along q, the contiguous direction of W.
//     k_sqm_p_mfma    P^(c) = U^T W^(c), the sum over (q, i) in one accumulation; one wave per 16 x 16 tile of one member, no split of the
//                     sum over workgroups, so the order does not depend on the grid.  Lane group l >> 4 takes the four consecutive q
//                     4 (l >> 4) .. + 3 of a chunk of 16: both operands use the same assignment, which a sum in MFMA mode is free to do.
//                     Ragged tiles are zero-filled operands whose results are never stored.  k_sqm_pow2 follows with n = 1.
//   k_sqm_dot         the closing products of a bond, one workgroup per carried matrix, in ttx_cores_dot's association order for
//                     tot = r^2 <= 16384: segments of 256 consecutive elements, a lane per element, the lanes halved (t, t + 128) .. (0, 1),
//                     the segment sums added ascending from 0.0 (segments past tot are 0.0 and change nothing).
//   the band          T = PL_(k-1) U_k by k_sqm_w without a stencil, k_sqm_d0 (D0 = T PR_k^T, ascending b' from 0.0), k_sqm_band (for
//                     i' = i and i + 1 the bracket sum_a U(a, i, b) D0(a, i', b) per b, then ascending b from 0.0).
// No floating-point atomics and no sum whose order depends on the grid or on the batch: a call repeats bit for bit, and a carried
// matrix does not depend on which others share its launch.  Every index comes from the shapes; no kernel uses scratch memory.
#pragma once

#define TTX_SQM_TILE_COLS 64        // columns (i, p) of a workgroup of k_sqm_w_mfma: 4 waves x one tile of 16

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "ttx_sq_norm.h"   // sqn_stencil
#include "ttx_ttops.h"     // dbl4

// k_sqn_w with a batch index c = blockIdx.y: P and O of member c lie at c * pst and c * ost.  md null: V = U (no stencil)
__global__ __launch_bounds__(128) void k_sqm_w(const double *U, int RM, size_t sq, size_t sp, int Q, int n, const double *md, const double *mo, const double *P, size_t pst,
                                               double *O, size_t ost)
{
    __shared__ double v[128];
    const int i = blockIdx.x % n, p = blockIdx.x / n, q = threadIdx.x;
    P += pst * blockIdx.y; O += ost * blockIdx.y;
    if (q < Q) {
        const double *u = U + sq * (size_t)q + sp * (size_t)p;
        v[q] = md ? sqn_stencil(u, RM, i, n, md, mo) : u[(size_t)RM * i];
    }
    __syncthreads();
    if (q >= Q) return;
    double s = 0.0;
#pragma unroll 4
    for (int t = 0; t < Q; t++) s = s + P[q + (size_t)Q * t] * v[t];
    O[q + (size_t)Q * (i + (size_t)n * p)] = s;
}

// k_sqn_p with a batch index: blockIdx.z = i + n c; O of member c at c * ost, its partial matrices at c * n * R * R
__global__ __launch_bounds__(256) void k_sqm_p(const double *U, int RM, size_t sq, size_t sp, int Q, int R, const double *O, size_t ost, int n, double *Part)
{
    __shared__ double gs[16][17], ws[16][17];
    const int t = threadIdx.x, lo = t & 15, hi = t >> 4, b0 = 16 * blockIdx.x, c0 = 16 * blockIdx.y, i = blockIdx.z % n, c = blockIdx.z / n;
    O += ost * c; Part += (size_t)c * n * R * R;
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

// k_sqn_pow2 with a batch index c = blockIdx.x: Part at c * n * M, P at c * M, ein[c * est_in], ecum[c * est_out] (ein may be ecum).
// scale == 0: the sum alone, no power of two, no exponent written (a right matrix RA)
__global__ __launch_bounds__(1024) void k_sqm_pow2(int M, int n, const double *Part, double *P, const int *ein, int est_in, int *ecum, int est_out, int scale)
{
    __shared__ double red[1024];
    const int c = blockIdx.x;
    Part += (size_t)c * n * M; P += (size_t)c * M;
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
    if (!scale) return;
    red[threadIdx.x] = bad ? __builtin_inf() : m;
    __syncthreads();
    for (int o = 512; o; o >>= 1) { if ((int)threadIdx.x < o) { const double v = red[threadIdx.x + o]; if (v > red[threadIdx.x]) red[threadIdx.x] = v; } __syncthreads(); }
    m = red[0];
    int ex = 0;
    if (m > 0.0 && m <= 1.7976931348623157e308) (void)frexp(m, &ex);
    for (int q = threadIdx.x; q < M; q += 1024) P[q] = ldexp(P[q], -ex);
    if (threadIdx.x == 0) ecum[(size_t)c * est_out] = ein[(size_t)c * est_in] + ex;
}

// O_c(q, col) = sum_q' P_c(q, q') V(q', col), col = i + n p, on the matrix cores.  Grid: x column tiles of TTX_SQM_TILE_COLS, y row tiles of
// 16, z the member.  A operand V(k, col0 + (l & 15)), B operand P_c(q0 + (l & 15), k), k = k0 + (l >> 4): D(col, q), lanes along q.
__global__ __launch_bounds__(256) void k_sqm_w_mfma(const double *U, int RM, size_t sq, size_t sp, int Q, int n, int R, const double *md, const double *mo, const double *P, size_t pst,
                                                    double *O, size_t ost)
{
    const int l = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = l & 15, kq = l >> 4;
    const long long cols = (long long)n * R, col0 = (long long)TTX_SQM_TILE_COLS * blockIdx.x + 16 * wave, col = col0 + lo;
    const int q0 = 16 * blockIdx.y, q = q0 + lo;
    if (col0 >= cols) return;                                                   // a whole wave: no barrier follows
    P += pst * blockIdx.z; O += ost * blockIdx.z;
    const bool cok = col < cols, qok = q < Q;
    const int i = cok ? (int)(col % n) : 0, p = cok ? (int)(col / n) : 0;
    const double *u = U + sp * (size_t)p;
    dbl4 acc = dbl4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < Q; k0 += 4) {
        const int k = k0 + kq;
        const double a = (cok && k < Q) ? sqn_stencil(u + sq * (size_t)k, RM, i, n, md, mo) : 0.0;
        const double b = (qok && k < Q) ? P[q + (size_t)Q * k] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
    if (!qok) return;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const long long cc = col0 + kq + 4 * reg;
        if (cc < cols) O[q + (size_t)Q * (size_t)cc] = acc[reg];
    }
}

// P_c(p, p') = sum_(q, i) U(q, i, p) O_c(q, i, p') on the matrix cores, one accumulation per element.  A wave owns tile (tp, tp') of member
// c: blockIdx.x = 4 waves of consecutive tiles, blockIdx.y = c.  A operand O_c(k, p'0 + (l & 15)), B operand U(k, p0 + (l & 15)): D(p', p),
// lanes along p.  The q of a chunk of 16 are dealt 4 (l >> 4) + st to step st, the same for both operands.
__global__ __launch_bounds__(256) void k_sqm_p_mfma(const double *U, int RM, size_t sq, size_t sp, int Q, int R, const double *O, size_t ost, int n, double *Pout, size_t pst)
{
    const int l = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = l & 15, kq = l >> 4;
    const int nt = (R + 15) / 16, tile = 4 * blockIdx.x + wave;
    if (tile >= nt * nt) return;                                                // a whole wave: no barrier follows
    const int p0 = 16 * (tile % nt), c0 = 16 * (tile / nt), p = p0 + lo, pc = c0 + lo;
    O += ost * blockIdx.y; Pout += pst * blockIdx.y;
    const bool pok = p < R, cok = pc < R;
    const double *ub = U + sp * (size_t)(pok ? p : 0), *ob = O + (size_t)Q * n * (size_t)(cok ? pc : 0);
    dbl4 acc = dbl4{0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < n; i++) {
        const double *ui = ub + (size_t)RM * i, *oi = ob + (size_t)Q * i;
        for (int q0 = 0; q0 < Q; q0 += 16) {
#pragma unroll
            for (int st = 0; st < 4; st++) {
                const int q = q0 + 4 * kq + st;
                const double a = (cok && q < Q) ? oi[q] : 0.0;
                const double b = (pok && q < Q) ? ui[sq * (size_t)q] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
        }
    }
    if (!pok) return;
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int cc = c0 + kq + 4 * reg;
        if (cc < R) Pout[p + (size_t)R * cc] = acc[reg];
    }
}

// dots[c] = dot(A + c * ast, B) over tot <= 16384 elements in ttx_cores_dot's order; eout[c] = ein[c] (the member's exponent now; ein
// null: eout untouched).  One workgroup per member.
__global__ __launch_bounds__(256) void k_sqm_dot(int tot, const double *A, size_t ast, const double *B, const int *ein, double *dots, int *eout)
{
    __shared__ double sm[256];
    const int t = threadIdx.x, c = blockIdx.x;
    A += ast * c;
    double s = 0.0;
    for (int e0 = 0; e0 < tot; e0 += 256) {
        const int e = e0 + t;
        double v = 0.0;
        if (e < tot) v = v + A[e] * B[e];
        if (e0) __syncthreads();
        sm[t] = v;
        __syncthreads();
        for (int hlf = 128; hlf >= 1; hlf >>= 1) {
            if (t < hlf) sm[t] = sm[t] + sm[t + hlf];
            __syncthreads();
        }
        s = s + sm[0];
    }
    if (t == 0) { dots[c] = s; if (ein) eout[c] = ein[c]; }
}

// D0(row, b) = sum_b' T(row, b') PR(b, b'), ascending b' from 0.0; rows = r0 n, T compact rows x r1, PR r1 x r1 compact
__global__ __launch_bounds__(256) void k_sqm_d0(long long rows, int r1, const double *T, const double *PR, double *D0)
{
    const long long tot = rows * r1;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long long)gridDim.x * blockDim.x) {
        const long long row = e % rows;
        const int b = (int)(e / rows);
        double s = 0.0;
#pragma unroll 4
        for (int q = 0; q < r1; q++) s = s + T[row + rows * q] * PR[b + (size_t)r1 * q];
        D0[e] = s;
    }
}

// B(i, i') = sum_b [ sum_a U(a, i, b) D0(a, i', b) ] for i' = i (band[i]) and i' = i + 1 (band[n + i]; 0.0 at i = n - 1), the bracket ascending
// a from 0.0, then ascending b from 0.0.  blockIdx.x = i, blockIdx.y = i' - i; a thread per b (r1 <= 128).  U is the resident core (element
// strides 1, RM, SS), D0 compact r0 x n x r1.
__global__ __launch_bounds__(128) void k_sqm_band(const double *U, int RM, size_t SS, int r0, int n, int r1, const double *D0, double *band)
{
    __shared__ double br[128];
    const int i = blockIdx.x, ip = i + blockIdx.y, b = threadIdx.x;
    if (ip >= n) { if (b == 0) band[(size_t)n * blockIdx.y + i] = 0.0; return; }
    if (b < r1) {
        double s = 0.0;
#pragma unroll 4
        for (int a = 0; a < r0; a++) s = s + U[(size_t)a + (size_t)RM * i + SS * (size_t)b] * D0[a + (size_t)r0 * (ip + (size_t)n * b)];
        br[b] = s;
    }
    __syncthreads();
    if (b == 0) {
        double s = 0.0;
        for (int x = 0; x < r1; x++) s = s + br[x];
        band[(size_t)n * blockIdx.y + i] = s;
    }
}
#endif
