// ttx_roundsum.h -- a rounded sum of resident tensor trains without ever forming a core of rank sum_t r_t (ttx_lincomb_round):
// the "randomize-then-orthogonalize" rounding of Al Daas, Ballard, Cazeaux, Hallman, Miedlar, Pasha, Reid, Saibaba (SIAM J. Sci.
// Comput. 2023) for sums of trains.  No intermediate rank exceeds the sketch rank.
//
// The definition (include/ttx.h and tests/roundsum_ref.py restate it).  Modes k = 1 .. d, cores X_{t,k} (r_t(k-1), n_k, r_t(k)) of
// the m terms, S(k) = sum_t r_t(k), coefficients c_t, sketch rank L, seed.
//  1. Sketch ranks (host, rs_sketch_ranks): l(0) = l(d) = 1; l(k) = min(L, S(k), prod_{j<=k} n_j, prod_{j>k} n_j), a product no
//     longer multiplied once it is above 128; then left to right l(k) <= l(k-1) n_k, then right to left l(k-1) <= n_k l(k).
//  2. Sketch train Omega_k (l(k-1), n_k, l(k)), entry at flat column-major index x = a + l(k-1) (i + n_k b), uniform on (-1, 1):
//        z = seed + 0x9E3779B97F4A7C15 * ((k << 40) + x + 1)                       (uint64, wrapping; k = 1 .. d)
//        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31)
//        value = (bit 63 of z ? -1 : +1) * ((z >> 11) & (2^52 - 1)) * 2^-52
//     (the splitmix64 finaliser; the top 53 bits are a sign and a 52-bit magnitude, every step is exact in a double).
//  3. Right to left: W_t(d) = [1]; W_t(k-1) = sum_i X_{t,k}(:, i, :) W_t(k) Omega_k(:, i, :)^T, r_t(k-1) x l(k-1); the W_t(k) of all
//     terms are stacked in term order (S(k) rows).  After each step the whole stack is multiplied by 2^-e, (f, e) = frexp(max |W|)
//     (e = 0 for a stack of zeros or one that holds an Inf or a NaN): one power of two per bond, common to all terms -- a per-term scale would
//     change the sum of step 4, a common power of two changes no bit of any Q; without it long trains overflow.
//  4. Left to right: Y_t(1) = c_t X_{t,1}; the Y_t(k) side by side are Y(k), l(k-1) n_k rows (row a + l(k-1) i), S(k) columns.
//     For k = 1 .. d-1:  Z = Y(k) W(k);  Z = Q R by the engine's qr();  new core k = Q;  M = Q^T Y(k);  Y_t(k+1) = M_t x_1 X_{t,k+1}.
//     New core d = sum_t Y_t(d) in term order.  Y is plain double WITHOUT a running exponent, as in ttx_contract: a sum whose
//     elements leave the double range is not rescued.
//  5. tol >= 0: svd_impl(tol, rmax) on the new train; tol < 0: the left-orthogonal train of step 4 with ranks l(k).
//
// Kernels.  The operand cores are read in place in their padded layout (element (a, j, b) at a + RM j + SS b), never packed.
//   k_rs_omega    step 2 for all cores in one launch (grid.y = core)
//   k_rs_sketch   step 3 of one mode for all terms in one launch.  A workgroup of four waves takes 16 rows a of one term (the
//                 term by bisection over RsBlk::firstS).  Per index i: U (16 x l(k)) = X(a, i, :) W_t(k), the 16-column tiles dealt
//                 to the waves, through LDS (row stride 17) into the A-operand map; then out (16 x l(k-1)) += U Omega_k(:, i, :)^T,
//                 the tiles of out dealt to the waves (two per wave at most: l <= 128), accumulated over i in registers.
//   k_rs_scale    the power of two of step 3, one workgroup
//   k_rs_advance  Y_t(k+1) = M_t x_1 X_{t,k+1} of one mode for all terms in one launch: one wave per 16 x 16 tile of the
//                 l(k) x (n r_t(k+1)) result, written into the term's column block of Y(k+1).  With M = (c_1 .. c_m), 1 x m, it is
//                 step 4's Y_t(1) = c_t X_{t,1}: one product per element, nothing added to it but zeros.
//   k_rs_last     new core d = sum_t Y_t(d), ascending t, into the padded layout
// <true>: v_mfma_f64_16x16x4_f64, lane maps of k_gemm_mfma (ttx_ttops.h): A[row l & 15][k l >> 4], B[k l >> 4][col l & 15], C/D col =
// l & 15, row = (l >> 4) + 4 reg.  Operands beyond an edge are zero-filled and never read, so no rank or mode size needs to be a
// multiple of 16 or 4.  <false>: the same work split with plain loops, s = s + x * y over ascending index (TTX_EVAL_EXACT, the checker).
// Neither has atomics or a split of a sum across workgroups: a call repeats bit for bit.
// Z = Y W and M = Q^T Y run on k_gemm_mfma in both modes (Q^T by k_transpose).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include <vector>

// the sizes, the term table and step 1 are plain C++ a host compiler accepts (ttx_op_plan.h fills the table)

#define TTX_RS_MAXTERMS 256         // m
#define TTX_RS_MAXSUM 4096          // sum_t r_t(k) at any bond
#define TTX_RS_LDU 17               // row stride of U in LDS (doubles)
// TTX_EVAL_AUTO takes the matrix cores from this many flops per call on.  PROVISIONAL: the break-even has not been measured
// (profiles/roundsum_mi355x.txt has the commands that give it)
#define TTX_RS_AUTO_FLOPS 1.0e7

struct RsBlk {                      // one term at one mode k
    const double *x;                // core k of the term
    size_t SS;
    long long firstS, firstA;       // first workgroup of the term in the mode's sketch / advance launch
    int RM, r0, r1;                 // r_t(k-1), r_t(k)
    int o0, o1;                     // the term's first row in the stacked W(k-1) / W(k): its first column in Y(k-1) / Y(k)
    int pad;
};

// step 1 (host).  n[0 .. d-1], S[0 .. d] (S[0] = S[d] = m is not used), l[0 .. d]
inline void rs_sketch_ranks(int d, const int32_t *n, const long long *S, int L, int32_t *l)
{
    std::vector<long long> pl(d + 1, 1), pr(d + 1, 1);
    for (int k = 1; k <= d; k++) pl[k] = pl[k - 1] > 128 ? pl[k - 1] : pl[k - 1] * n[k - 1];
    for (int k = d - 1; k >= 0; k--) pr[k] = pr[k + 1] > 128 ? pr[k + 1] : pr[k + 1] * n[k];
    l[0] = l[d] = 1;
    for (int k = 1; k < d; k++) l[k] = (int32_t)std::min(std::min<long long>(L, S[k]), std::min(pl[k], pr[k]));
    for (int k = 1; k < d; k++) l[k] = (int32_t)std::min<long long>(l[k], (long long)l[k - 1] * n[k - 1]);
    for (int k = d - 1; k >= 1; k--) l[k] = (int32_t)std::min<long long>(l[k], (long long)n[k] * l[k + 1]);
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "ttx_ttops.h"     // dbl4, block_max_xor, tt_pow2_above

// step 2
__host__ __device__ inline double rs_uniform(unsigned long long seed, int k, unsigned long long x)
{
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (((unsigned long long)k << 40) + x + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z = z ^ (z >> 31);
    const double v = (double)(long long)((z >> 11) & 0xFFFFFFFFFFFFFull) * 2.220446049250313e-16;       // 2^-52, exact
    return (z >> 63) ? -v : v;
}
// off[k-1] .. off[k]: core k of Omega in out
__global__ __launch_bounds__(256) void k_rs_omega(unsigned long long seed, const size_t *off, double *out)
{
    const int k = blockIdx.y + 1;
    const size_t lo = off[k - 1], cnt = off[k] - lo;
    for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < cnt; x += (size_t)gridDim.x * blockDim.x) out[lo + x] = rs_uniform(seed, k, x);
}

template <bool SKETCH>
__device__ inline RsBlk rs_find(const RsBlk *blks, int m, long long *t)
{
    int lo = 0, hi = m - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((SKETCH ? blks[mid].firstS : blks[mid].firstA) <= (long long)blockIdx.x) lo = mid; else hi = mid - 1;
    }
    *t = (long long)blockIdx.x - (SKETCH ? blks[lo].firstS : blks[lo].firstA);
    return blks[lo];
}

// mode k: Wk = W(k) (S1 rows, l1 columns), Om = Omega_k (l0, n, l1), Wo = W(k-1) (S0 rows, l0 columns)
template <bool MFMA>
__global__ __launch_bounds__(256) void k_rs_sketch(const RsBlk *blks, int m, int n, int l0, int l1, const double *Om, const double *Wk, int S1, double *Wo, int S0)
{
    __shared__ double U[TTX_RS_LDU * 128];
    long long ab;
    const RsBlk B = rs_find<true>(blks, m, &ab);
    const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, c = l & 15, q4 = l >> 4;
    const int a0 = (int)ab * 16, a = a0 + c;
    const int nq = (l1 + 15) >> 4, np = (l0 + 15) >> 4;
    const double *wt = Wk + B.o1;
    if (MFMA) {
        dbl4 acc[2] = {dbl4{0.0, 0.0, 0.0, 0.0}, dbl4{0.0, 0.0, 0.0, 0.0}};
        for (int i = 0; i < n; i++) {
            const double *xi = B.x + a + (size_t)B.RM * i;
            for (int tq = wave; tq < nq; tq += 4) {
                const int qq = tq * 16 + c;
                dbl4 u = {0.0, 0.0, 0.0, 0.0};
                for (int b0 = 0; b0 < B.r1; b0 += 4) {
                    const int b = b0 + q4;
                    const double av = (a < B.r0 && b < B.r1) ? xi[B.SS * b] : 0.0;
                    const double bv = (b < B.r1 && qq < l1) ? wt[b + (size_t)S1 * qq] : 0.0;
                    u = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, u, 0, 0, 0);
                }
#pragma unroll
                for (int reg = 0; reg < 4; reg++) U[(q4 + 4 * reg) + TTX_RS_LDU * qq] = u[reg];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 2; j++) {
                const int tp = wave + 4 * j, p = tp * 16 + c;
                if (tp < np) {
                    const double *om = Om + p + (size_t)l0 * i;
                    for (int k0 = 0; k0 < 16 * nq; k0 += 4) {
                        const int qq = k0 + q4;
                        const double av = U[c + TTX_RS_LDU * qq];
                        const double bv = (p < l0 && qq < l1) ? om[(size_t)l0 * n * qq] : 0.0;
                        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[j], 0, 0, 0);
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int p = (wave + 4 * j) * 16 + c;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int ar = a0 + q4 + 4 * reg;
                if (p < l0 && ar < B.r0) Wo[B.o0 + ar + (size_t)S0 * p] = acc[j][reg];
            }
        }
    } else {
        const int g = tid >> 4;                                                  // lane (a, g): columns q = g + 16 j of U, p = g + 16 j of out
        double acc[8];
#pragma unroll
        for (int j = 0; j < 8; j++) acc[j] = 0.0;
        for (int i = 0; i < n; i++) {
            const double *xi = B.x + a + (size_t)B.RM * i;
            for (int qq = g; qq < l1; qq += 16) {
                double s = 0.0;
                if (a < B.r0) for (int b = 0; b < B.r1; b++) s = s + xi[B.SS * b] * wt[b + (size_t)S1 * qq];
                U[c + TTX_RS_LDU * qq] = s;
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int p = g + 16 * j;
                if (p < l0) {
                    const double *om = Om + p + (size_t)l0 * i;
                    double s = acc[j];
                    for (int qq = 0; qq < l1; qq++) s = s + U[c + TTX_RS_LDU * qq] * om[(size_t)l0 * n * qq];
                    acc[j] = s;
                }
            }
            __syncthreads();
        }
        if (a < B.r0) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int p = g + 16 * j;
                if (p < l0) Wo[B.o0 + a + (size_t)S0 * p] = acc[j];
            }
        }
    }
}

// W (cnt doubles) *= 2^-e, (f, e) = frexp(max |W|); e = 0 for zeros and for a stack with an Inf or a NaN in it (a NaN counts as not finite)
__global__ __launch_bounds__(1024) void k_rs_scale(size_t cnt, double *W)
{
    __shared__ double red[16];
    double mx = 0.0;
    for (size_t x = threadIdx.x; x < cnt; x += blockDim.x) { const double v = fabs(W[x]); mx = v != v ? INFINITY : fmax(mx, v); }   // fmax would drop a NaN
    const int e = tt_pow2_above(block_max_xor(mx, red));
    if (e == 0) return;
    const double s = ldexp(1.0, -e);
    for (size_t x = threadIdx.x; x < cnt; x += blockDim.x) W[x] *= s;
}

// mode k (blks of core k): M (lr rows, column o0 + b of term t, leading dimension ldm) -> Yn (lr n rows, leading dimension ldy);
// a workgroup takes the tile of 16 rows pt and four tiles of 16 columns j = i + n c of one term, ntp = tiles of rows
template <bool MFMA>
__global__ __launch_bounds__(256) void k_rs_advance(const RsBlk *blks, int m, int n, int lr, int ntp, const double *M, int ldm, double *Yn, size_t ldy)
{
    long long t;
    const RsBlk B = rs_find<false>(blks, m, &t);
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, c = l & 15, q4 = l >> 4;
    const int pt = (int)(t % ntp);
    const long long ncol = (long long)n * B.r1, jt = ((t / ntp) * 4 + wave) * 16;
    if (jt >= ncol) return;
    const long long j = jt + c;
    const bool jok = j < ncol;
    const int cc = jok ? (int)(j / n) : 0, i = jok ? (int)(j - (long long)cc * n) : 0;
    const double *xj = B.x + (size_t)B.RM * i + B.SS * cc;
    const double *mt = M + (size_t)ldm * B.o0;
    double *o = Yn + (size_t)lr * i + ldy * (size_t)(B.o1 + cc);
    if (MFMA) {
        const int p = pt * 16 + c;
        dbl4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int b0 = 0; b0 < B.r0; b0 += 4) {
            const int b = b0 + q4;
            const double av = (p < lr && b < B.r0) ? mt[p + (size_t)ldm * b] : 0.0;
            const double bv = (jok && b < B.r0) ? xj[b] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = pt * 16 + q4 + 4 * reg;
            if (jok && row < lr) o[row] = acc[reg];
        }
    } else if (jok) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int b = 0; b < B.r0; b++) {
            const double xv = xj[b];
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int row = pt * 16 + q4 + 4 * reg;
                if (row < lr) s[reg] = s[reg] + mt[row + (size_t)ldm * b] * xv;
            }
        }
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = pt * 16 + q4 + 4 * reg;
            if (row < lr) o[row] = s[reg];
        }
    }
}

// new core d (lr, n, 1) = sum over the m columns of Y(d) (lr n rows), ascending t
__global__ __launch_bounds__(256) void k_rs_last(int lr, int n, int m, const double *Y, size_t ldy, double *core, int RM)
{
    for (int x = blockIdx.x * blockDim.x + threadIdx.x; x < lr * n; x += gridDim.x * blockDim.x) {
        double s = 0.0;
        for (int t = 0; t < m; t++) s = s + Y[x + ldy * t];
        core[(x % lr) + (size_t)RM * (x / lr)] = s;
    }
}
#endif
