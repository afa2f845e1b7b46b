// ttx_modeapply.h -- matrices applied to chosen modes of the resident tensor train (ttx_mode_apply: the n-mode product).
//
// An applied mode k replaces its index i = 0 .. n-1 by j = 0 .. m-1 through A_k (m x n, column-major, A_k(j, i) at j + m i):
//   G'_k(a, j, b) = sum_i A_k(j, i) G_k(a, i, b);   per slab b:  Out_b (r0 x m, ld RM') = G_b (r0 x n, ld RM) . A_k^T
// Element (a, j, b) of a core lies at a + RM j + SS b; the source and the new train have layouts of their own.
// The number of launches does not depend on d:
//   k_ma_copy   every untouched core, element by element into the new layout (bit-identical; no multiply touches it)
//   k_ma_apply  every applied core in one launch, <false> the scalar loop (TTX_EVAL_EXACT), <true> on v_mfma_f64_16x16x4_f64
// Work of k_ma_apply.  A unit is 16 rows a of one slab b; a workgroup of four waves takes four consecutive units of one core and
// one panel of TTX_MA_JP = 64 columns j (the core table MaCore gives the first workgroup of every core; a workgroup finds its
// core by bisection).  Over the K direction (i) it walks chunks of TTX_MA_KC = 32: the A_k panel of the chunk (64 x 32, zero
// beyond m and n) is staged in LDS once for all four waves -- A_k itself may be far larger than LDS, n goes up to 32000 -- and
// every wave reads its G elements from HBM once per panel: once in all when m <= 64.  Panels of one unit group are neighbours
// in the grid, so with m > 64 the re-reads meet L2.
// Lanes: l & 15 runs along a, the contiguous direction, for loads and stores alike (128-byte rows); l >> 4 along i (loads, the
// MFMA's k) and along j (stores).  The product is formed transposed, Out^T = A G^T, so that the result's lane map (col = l & 15,
// row = (l >> 4) + 4 reg; lane maps of k_gemm_mfma, ttx_ttops.h, and ct_gemm, ttx_contract.h) has a on the contiguous lanes:
//   A operand  A_k(j0 + 16 t + (l & 15), i0 + 4 s + (l >> 4))   from LDS (row stride 80 doubles: the two i rows of a half-wave
//                                                                fall into different halves of the 64 banks)
//   B operand  G(a0 + (l & 15), i0 + 4 s + (l >> 4), b)          from HBM, one load feeds the four MFMAs of the panel
// Rows a >= r0, columns j >= m and steps i >= n are zero-filled and never read; padded rows of the destination are never written.
// Low ranks: a unit always spans 16 rows, so r0 < 16 (the first core, low-rank bonds) leaves matrix rows and lanes idle -- 15
// of 16 at r0 = 1.  Such cores are small (r0 n r1 elements against the r^2 n of an interior core), they do not show in a call's time.
// EXACT: the same units, panels and staging; lane (a, q = l >> 4) owns the 16 columns j = j0 + q + 4 t and runs
//   s = 0.0; for i = 0 .. n-1: s = s + A_k(j, i) * G_k(a, i, b)       (ascending i, separate multiply and add: -ffp-contract=off)
// Neither kernel has atomics or a split of K across workgroups: an element depends on its own row of A_k and its own fibre of G_k
// alone, not on the tiling of other cores or the grid, and a call repeats bit for bit.
#pragma once

// the sizes and the core table are plain C++ a host compiler accepts (ttx_op_plan.h fills the table)
#define TTX_MA_JP 64                // columns j of a workgroup's panel
#define TTX_MA_KC 32                // steps i per staged chunk of A_k
#define TTX_MA_LDA 80               // row stride of the staged chunk in LDS (doubles)
#define TTX_MA_UNITS 4              // units (16 rows a x one slab b) per workgroup: one per wave
// TTX_EVAL_AUTO takes the matrix cores from this many flops per call (2 sum r0 r1 n m) on.  PROVISIONAL: the break-even has not
// been measured yet; profiles/modeapply_mi355x.txt has the runs that give it
#define TTX_MA_AUTO_FLOPS 1.0e7

struct MaCore {                     // one core of a launch (applied: k_ma_apply, untouched: k_ma_copy)
    const double *src, *A;          // A: this mode's block of the matrices (null in the copy table)
    double *dst;
    long long first;                // first workgroup of this core
    int r0, n, r1, m;               // m: columns of the result (n for a copy)
    int nab, npan, ngrp, pad;       // blocks of 16 rows a, panels of 64 columns j, groups of four units
};

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "ttx_ttops.h"     // dbl4

// the workgroup's core by bisection over MaCore::first, and its place in it: group of units and panel
__device__ inline const MaCore *ma_find(const MaCore *cores, int ncore, int *grp, int *pan)
{
    int lo = 0, hi = ncore - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (cores[mid].first <= (long long)blockIdx.x) lo = mid; else hi = mid - 1; }
    const long long t = (long long)blockIdx.x - cores[lo].first;
    *pan = (int)(t % cores[lo].npan); *grp = (int)(t / cores[lo].npan);
    return cores + lo;
}

// the MFMA steps of one staged chunk for a panel of NT tiles of 16 columns: FULL, all TTX_MA_KC / 4 steps unrolled, the loads
// ahead of the products; otherwise the steps of a last, shorter chunk one by one
template <int NT, bool FULL>
__device__ inline void ma_steps(const double *As, const double *gi, int RMs, bool ok, int kc, int col, int q, dbl4 (&acc)[4])
{
    if (FULL) {
        double gv[TTX_MA_KC / 4];
#pragma unroll
        for (int st = 0; st < TTX_MA_KC / 4; st++) gv[st] = ok ? gi[(size_t)RMs * (4 * st + q)] : 0.0;
#pragma unroll
        for (int st = 0; st < TTX_MA_KC / 4; st++)
#pragma unroll
            for (int t = 0; t < NT; t++)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(As[(4 * st + q) * TTX_MA_LDA + 16 * t + col], gv[st], acc[t], 0, 0, 0);
    } else {
#pragma unroll 1
        for (int st = 0; 4 * st < kc; st++) {
            const int ii = 4 * st + q;
            const double gv = (ok && ii < kc) ? gi[(size_t)RMs * ii] : 0.0;
#pragma unroll
            for (int t = 0; t < NT; t++)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(As[ii * TTX_MA_LDA + 16 * t + col], gv, acc[t], 0, 0, 0);
        }
    }
}

template <bool MFMA>
__global__ __launch_bounds__(256) void k_ma_apply(const MaCore *cores, int ncore, int RMs, size_t SSs, int RMd, size_t SSd)
{
    __shared__ double As[TTX_MA_KC * TTX_MA_LDA];
    int grp, pan;
    const MaCore c = *ma_find(cores, ncore, &grp, &pan);
    const int tid = threadIdx.x, l = tid & 63, col = l & 15, q = l >> 4;
    const int u = grp * TTX_MA_UNITS + (tid >> 6);                              // this wave's unit
    const int ab = u % c.nab, b = u / c.nab, a = ab * 16 + col;
    const bool live = b < c.r1, ok = live && a < c.r0;                          // a wave without a unit still stages and waits
    const int j0 = pan * TTX_MA_JP, jn = min(TTX_MA_JP, c.m - j0);              // 1 <= jn <= 64
    const double *g = c.src + a + SSs * (size_t)(live ? b : 0);
    dbl4 acc[4];
    double s[16];
    if (MFMA) { for (int t = 0; t < 4; t++) acc[t] = dbl4{0.0, 0.0, 0.0, 0.0}; }
    else { for (int t = 0; t < 16; t++) s[t] = 0.0; }
    const int nt = MFMA ? (jn + 15) >> 4 : (jn + 3) >> 2;
    for (int i0 = 0; i0 < c.n; i0 += TTX_MA_KC) {
        const int kc = min(TTX_MA_KC, c.n - i0);
        if (i0) __syncthreads();
        for (int e = tid; e < TTX_MA_KC * TTX_MA_JP; e += 256) {
            const int ii = e / TTX_MA_JP, jj = e % TTX_MA_JP;
            As[ii * TTX_MA_LDA + jj] = (ii < kc && jj < jn) ? c.A[(size_t)(j0 + jj) + (size_t)c.m * (i0 + ii)] : 0.0;
        }
        __syncthreads();
        if (!live) continue;
        const double *gi = g + (size_t)RMs * i0;
        if (MFMA) {
            const bool full = kc == TTX_MA_KC;
            switch (nt) {                                                       // uniform: straight-line code for every panel width
            case 1: full ? ma_steps<1, true>(As, gi, RMs, ok, kc, col, q, acc) : ma_steps<1, false>(As, gi, RMs, ok, kc, col, q, acc); break;
            case 2: full ? ma_steps<2, true>(As, gi, RMs, ok, kc, col, q, acc) : ma_steps<2, false>(As, gi, RMs, ok, kc, col, q, acc); break;
            case 3: full ? ma_steps<3, true>(As, gi, RMs, ok, kc, col, q, acc) : ma_steps<3, false>(As, gi, RMs, ok, kc, col, q, acc); break;
            default: full ? ma_steps<4, true>(As, gi, RMs, ok, kc, col, q, acc) : ma_steps<4, false>(As, gi, RMs, ok, kc, col, q, acc); break;
            }
        } else if (ok) {
#pragma unroll 2
            for (int ii = 0; ii < kc; ii++) {
                const double gv = gi[(size_t)RMs * ii];
#pragma unroll
                for (int t = 0; t < 16; t++)
                    if (t < nt) s[t] = s[t] + As[ii * TTX_MA_LDA + q + 4 * t] * gv;
            }
        }
    }
    if (!ok) return;
    double *o = c.dst + a + SSd * (size_t)b;
    if (MFMA) {
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int jj = 16 * t + q + 4 * reg;
                if (jj < jn) o[(size_t)RMd * (j0 + jj)] = acc[t][reg];
            }
    } else {
#pragma unroll
        for (int t = 0; t < 16; t++) {
            const int jj = q + 4 * t;
            if (jj < jn) o[(size_t)RMd * (j0 + jj)] = s[t];
        }
    }
}

// untouched cores into the new layout: the units and panels of k_ma_apply, lane (a, q) copies the columns j = j0 + q + 4 t
__global__ __launch_bounds__(256) void k_ma_copy(const MaCore *cores, int ncore, int RMs, size_t SSs, int RMd, size_t SSd)
{
    int grp, pan;
    const MaCore c = *ma_find(cores, ncore, &grp, &pan);
    const int l = threadIdx.x & 63, col = l & 15, q = l >> 4;
    const int u = grp * TTX_MA_UNITS + ((int)threadIdx.x >> 6);
    const int ab = u % c.nab, b = u / c.nab, a = ab * 16 + col;
    if (b >= c.r1 || a >= c.r0) return;
    const int j0 = pan * TTX_MA_JP, jn = min(TTX_MA_JP, c.m - j0);
    const double *g = c.src + a + SSs * (size_t)b;
    double *o = c.dst + a + SSd * (size_t)b;
    for (int jj = q; jj < jn; jj += 4) o[(size_t)RMd * (j0 + jj)] = g[(size_t)RMs * (j0 + jj)];
}
#endif
