// ttx_contract.h -- chosen modes of the resident tensor train contracted with rank-1 weights (ttx_contract / ttx_marginals).
//
// A contracted mode k turns its core into the matrix M_k = sum_i w_k(i) G_k(:, i, :)  (r(k-1) x r(k)); a maximal run of contracted
// modes between two kept modes becomes the ordered product of its M_k, which is multiplied into the kept core on its right (the
// run after the last kept mode into the last kept core from the right).  Element (a, j, b) of a core lies at a + RM j + SS b.
// The number of launches does not depend on d:
//   k_ct_modesum  all M_k in one launch; work = (core, tile of the (a, b) plane); lanes along a, the contiguous direction
//   k_ct_runs     one workgroup per run; leading / trailing runs are vector chains, interior runs matrix chains on
//                 v_mfma_f64_16x16x4_f64 (lane maps of k_gemm_mfma, ttx_ttops.h)
//   k_ct_absorb   new core = P G (t): one wave per (kept core, slab b, 16 columns j) reading the padded slabs directly
//   k_ct_chains   ttx_marginals: prefix vectors l_k = l_(k-1) M_k and suffix vectors s_k = M_k s_(k+1), one workgroup each
//   k_ct_marg     ttx_marginals: block k (i) = l_(k-1) G_k(:, i, :) s_(k+1), one wave per (k, i)
// Plain fp64, no running exponent (as k_quad_*): a train whose partial products leave the double range over- or underflows.
// Every sum has a fixed order (no atomics, no dependence on the order in which workgroups finish): results repeat bit for bit.
#pragma once
#include <stddef.h>

// the tables are plain C++ a host compiler accepts (ttx_op_plan.h fills them)
struct CtCore {                     // one source core (0-based mode k)
    const double *src;
    size_t moff, woff;              // offset of M_k (compact, leading dimension r0) in the M buffer; of the mode's weights / outputs
    int r0, n, r1, ta;              // ta: lanes along a in a tile of k_ct_modesum (power of two <= 64)
};
struct CtTile { int c, a0, b0, pad; };
struct CtRun {                      // modes k0 .. k0 + cnt - 1 (0-based), all contracted
    int k0, cnt, kind, wmax;        // kind 0 leading (before the first kept mode), 1 trailing, 2 interior; wmax = max r(k+1) in the run
    size_t poff, soff;              // result in the P buffer (interior: r(k0) x r(k0+cnt), leading dimension r(k0)); global ping-pong space
};
struct CtKeep {                     // one kept core: dst (q0 x n x q1) = P (q0 x r0; null: identity) . src (r0 x n x r1) . t (r1; null: identity)
    const double *src, *P, *t;
    double *dst;
    long long first;                // first work item of this core
    int r0, n, r1, q0, ncol, pad;   // ncol = column tiles of 16
};

#define TTX_CT_WCH 1024             // weights staged per pass of k_ct_modesum (one pass for modes up to this size)
#define TTX_CT_LDS 8192             // doubles of LDS k_ct_runs owns (64 KB)

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "ttx_ttops.h"     // dbl4

// M_k(a, b) = sum_j w_k(j) G_k(a, j, b) for every contracted core: 256 threads = ta lanes along a x 256 / ta columns b.
// Four partial sums per element (j mod 4) keep four loads in flight; they are added in a fixed order.
__global__ __launch_bounds__(256) void k_ct_modesum(const CtCore *cores, const CtTile *tiles, int RM, size_t SS, const double *w, double *M)
{
    __shared__ double ws[TTX_CT_WCH];
    const CtTile t = tiles[blockIdx.x];
    const CtCore c = cores[t.c];
    const int a = t.a0 + ((int)threadIdx.x & (c.ta - 1)), b = t.b0 + (int)threadIdx.x / c.ta;
    const bool ok = a < c.r0 && b < c.r1;                                       // padded rows and columns are never read
    const double *p = c.src + a + SS * b, *wk = w + c.woff;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int j0 = 0; j0 < c.n; j0 += TTX_CT_WCH) {
        const int m = min(TTX_CT_WCH, c.n - j0);
        if (j0) __syncthreads();
        for (int j = threadIdx.x; j < m; j += 256) ws[j] = wk[j0 + j];
        __syncthreads();
        if (ok) {
            const double *q = p + (size_t)RM * j0;
            int j = 0;
#pragma unroll 2
            for (; j + 4 <= m; j += 4) {
                const double x0 = q[(size_t)RM * j], x1 = q[(size_t)RM * (j + 1)], x2 = q[(size_t)RM * (j + 2)], x3 = q[(size_t)RM * (j + 3)];
                s0 = s0 + ws[j] * x0; s1 = s1 + ws[j + 1] * x1; s2 = s2 + ws[j + 2] * x2; s3 = s3 + ws[j + 3] * x3;
            }
            for (; j < m; j++) s0 = s0 + ws[j] * q[(size_t)RM * j];
        }
    }
    if (ok) M[c.moff + a + (size_t)c.r0 * b] = (s0 + s1) + (s2 + s3);
}

// vo = v M (M r0 x r1, leading dimension r0): one wave per column, lanes along a, butterfly sum.  The caller synchronises.
__device__ inline void ct_vecmat(const double *v, const double *M, int r0, int r1, double *vo)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int b = wave; b < r1; b += nw) {
        double s = 0.0;
        for (int a = lane; a < r0; a += 64) s = s + v[a] * M[a + (size_t)r0 * b];
        s = wave_sum_xor(s);
        if (lane == 0) vo[b] = s;
    }
}
// uo = M u (ranks up to 128, 1024 threads): thread (a, g) sums the columns b = g mod 8; the 8 partial sums are added in g order.
// part: 1024 doubles of LDS.  The caller synchronises afterwards.
__device__ inline void ct_matvec(const double *M, const double *u, int r0, int r1, double *uo, double *part)
{
    const int a = threadIdx.x & 127, g = threadIdx.x >> 7, ng = blockDim.x >> 7;
    double s = 0.0;
    if (a < r0) for (int b = g; b < r1; b += ng) s = s + M[a + (size_t)r0 * b] * u[b];
    part[g * 128 + a] = s;
    __syncthreads();
    if ((int)threadIdx.x < r0) {
        double t = part[threadIdx.x];
        for (int q = 1; q < ng; q++) t = t + part[q * 128 + threadIdx.x];
        uo[threadIdx.x] = t;
    }
}
// C (m x n, ldc) = A (m x k, lda) B (k x n, ldb) by the waves of one workgroup, a 16 x 16 tile each; A[row l&15][k l>>4],
// B[k l>>4][col l&15], C: col = l&15, row = (l>>4) + 4 reg.  Rows, columns and k steps outside the matrices are zero-filled, never read.
__device__ inline void ct_gemm(int m, int n, int k, const double *A, int lda, const double *B, int ldb, double *C, int ldc)
{
    const int l = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, kq = l >> 4;
    const int tmn = (m + 15) >> 4, tnn = (n + 15) >> 4;
    for (int t = wave; t < tmn * tnn; t += nw) {
        const int tm = (t % tmn) * 16, tn = (t / tmn) * 16, ar = tm + (l & 15), bc = tn + (l & 15);
        dbl4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < k; k0 += 4) {
            const int kk = k0 + kq;
            const double a = (ar < m && kk < k) ? A[ar + (size_t)lda * kk] : 0.0;
            const double b = (bc < n && kk < k) ? B[kk + (size_t)ldb * bc] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = tm + kq + 4 * reg;
            if (row < m && bc < n) C[row + (size_t)ldc * bc] = acc[reg];
        }
    }
}

// the products of all runs, one workgroup (16 waves) per run.  An interior run keeps its running product in two LDS images while
// they fit (2 r(k0) wmax doubles <= 64 KB: up to rank 64), in global scratch above that.
__global__ __launch_bounds__(1024) void k_ct_runs(const CtRun *runs, const int *r, const size_t *moff, const double *M, double *Pb, double *scr)
{
    __shared__ __align__(16) double lds[TTX_CT_LDS];
    const CtRun R = runs[blockIdx.x];
    const int tid = threadIdx.x, k0 = R.k0, last = R.k0 + R.cnt - 1;
    if (R.kind == 0) {                                                          // r(k0) = 1: v = M_k0, then v = v M_k
        double *va = lds, *vb = lds + 128;
        if (tid < r[k0 + 1]) va[tid] = M[moff[k0] + tid];
        __syncthreads();
        for (int k = k0 + 1; k <= last; k++) {
            ct_vecmat(va, M + moff[k], r[k], r[k + 1], vb);
            __syncthreads();
            double *x = va; va = vb; vb = x;
        }
        if (tid < r[last + 1]) Pb[R.poff + tid] = va[tid];
    } else if (R.kind == 1) {                                                   // r(last + 1) = 1: u = M_last, then u = M_k u
        double *ua = lds, *ub = lds + 128, *part = lds + 256;
        if (tid < r[last]) ua[tid] = M[moff[last] + tid];
        __syncthreads();
        for (int k = last - 1; k >= k0; k--) {
            ct_matvec(M + moff[k], ua, r[k], r[k + 1], ub, part);
            __syncthreads();
            double *x = ua; ua = ub; ub = x;
        }
        if (tid < r[k0]) Pb[R.poff + tid] = ua[tid];
    } else {
        const int m = r[k0];
        const size_t img = (size_t)m * R.wmax;
        double *b0 = 2 * img <= TTX_CT_LDS ? lds : scr + R.soff, *b1 = b0 + img;
        const double *cur = M + moff[k0];
        for (int k = k0 + 1; k <= last; k++) {
            ct_gemm(m, r[k + 1], r[k], cur, m, M + moff[k], r[k], b0, m);
            __syncthreads();
            cur = b0;
            double *x = b0; b0 = b1; b1 = x;
        }
        for (int e = tid; e < m * r[last + 1]; e += blockDim.x) Pb[R.poff + e] = cur[e];
    }
}

// new cores: one wave per (kept core, slab b, 16 columns j).  With a trailing vector t the wave first folds the slabs,
// H(:, j) = sum_b G(:, j, b) t(b) (b ascending from 0), into LDS; with a left factor P the product runs on the matrix cores,
// B read from the padded slab (or H) directly; with neither the item is a strided copy.
__global__ __launch_bounds__(64) void k_ct_absorb(const CtKeep *keeps, int nkeep, int RMs, size_t SSs, int RMd, size_t SSd)
{
    __shared__ double H[128 * 16];
    int lo = 0, hi = nkeep - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (keeps[mid].first <= (long long)blockIdx.x) lo = mid; else hi = mid - 1; }
    const CtKeep K = keeps[lo];
    const int it = (int)((long long)blockIdx.x - K.first), jt = it % K.ncol, b = it / K.ncol, j0 = jt * 16, nj = min(16, K.n - j0);
    const int l = threadIdx.x;
    const double *G = K.src + (size_t)RMs * j0 + SSs * b;                       // b = 0 with a trailing vector
    double *D = K.dst + (size_t)RMd * j0 + SSd * b;
    if (K.t) {
        for (int jj = 0; jj < nj; jj++)
            for (int a = l; a < K.r0; a += 64) {
                double s = 0.0;
#pragma unroll 4
                for (int bb = 0; bb < K.r1; bb++) s = s + G[a + (size_t)RMs * jj + SSs * bb] * K.t[bb];
                H[a + 128 * jj] = s;
            }
        __syncthreads();
    }
    if (!K.P) {
        for (int jj = 0; jj < nj; jj++)
            for (int a = l; a < K.r0; a += 64) D[a + (size_t)RMd * jj] = K.t ? H[a + 128 * jj] : G[a + (size_t)RMs * jj];
        return;
    }
    const int col = l & 15, kq = l >> 4;
    for (int tm = 0; tm < K.q0; tm += 16) {
        const int ar = tm + col;
        dbl4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < K.r0; k0 += 4) {
            const int kk = k0 + kq;
            const double a = (ar < K.q0 && kk < K.r0) ? K.P[ar + (size_t)K.q0 * kk] : 0.0;
            const double bv = (col < nj && kk < K.r0) ? (K.t ? H[kk + 128 * col] : G[kk + (size_t)RMs * col]) : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = tm + kq + 4 * reg;
            if (row < K.q0 && col < nj) D[row + (size_t)RMd * col] = acc[reg];
        }
    }
}

// ttx_marginals: workgroup 0 forms l_0 = [1], l_k = l_(k-1) M_k (k = 1 .. d-1), workgroup 1 s_(d+1) = [1], s_k = M_k s_(k+1)
// (k = d .. 2); vector k of either family lies at k ldv (1-based k as in the formulas)
__global__ __launch_bounds__(1024) void k_ct_chains(int d, const int *r, const size_t *moff, const double *M, double *L, double *S, int ldv)
{
    __shared__ double part[1024];
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0) L[0] = 1.0;
        __syncthreads();
        for (int k = 1; k < d; k++) {
            ct_vecmat(L + (size_t)(k - 1) * ldv, M + moff[k - 1], r[k - 1], r[k], L + (size_t)k * ldv);
            __syncthreads();
        }
    } else {
        if (threadIdx.x == 0) S[(size_t)(d + 1) * ldv] = 1.0;
        __syncthreads();
        for (int k = d; k >= 2; k--) {
            ct_matvec(M + moff[k - 1], S + (size_t)(k + 1) * ldv, r[k - 1], r[k], S + (size_t)k * ldv, part);
            __syncthreads();
        }
    }
}
// out[woff(k) + i] = l_(k-1) G_k(:, i, :) s_(k+1): one wave per (k, i); lane a sums over b (ascending) its rows a, a + 64, the
// lanes are added by a butterfly
__global__ __launch_bounds__(256) void k_ct_marg(int d, const CtCore *cores, long long nitem, int RM, size_t SS, const double *L, const double *S, int ldv, double *out)
{
    const int lane = threadIdx.x & 63;
    const long long item = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (item >= nitem) return;
    int lo = 0, hi = d - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if ((long long)cores[mid].woff <= item) lo = mid; else hi = mid - 1; }
    const CtCore c = cores[lo];
    const int i = (int)(item - (long long)c.woff);
    const double *lv = L + (size_t)lo * ldv, *sv = S + (size_t)(lo + 2) * ldv, *G = c.src + (size_t)RM * i;
    double acc = 0.0;
    for (int a = lane; a < c.r0; a += 64) {
        const double la = lv[a];
#pragma unroll 4
        for (int b = 0; b < c.r1; b++) acc = acc + (la * G[a + SS * b]) * sv[b];
    }
    acc = wave_sum_xor(acc);
    if (lane == 0) out[item] = acc;
}
#endif
