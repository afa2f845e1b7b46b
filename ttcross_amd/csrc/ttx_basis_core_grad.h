// ttx_basis_core_grad.h -- the gradient with respect to the cores of the resident tensor train in a function basis at a BATCH of real
// points (ttx_basis_core_grad_batch / ttx_basis_core_grad_tab and their _dev forms), and the update U_i <- U_i + alpha_i G_i
// (ttx_cores_axpy).  f is linear in every core, so with the caller's weights c[p] (the derivative of their loss with respect to
// f(x_p))
//     G_i(a, j, k) = G0_i(a, j, k) + sum_p ((c[p] * L_i(p, a)) * (phi_(i, j)(p) * X_i(p, k))),
// L_i the train left of core i and X_i the train right of it at point p.
//
// The definition of include/ttx.h.  Backward, mode i = d .. 1, from X_d = (1): the chain of ttx_basis.h with every X_i kept.  Forward,
// mode i = 1 .. d, from L_1 = (1): the forward step of ttx_basis_grad.h.  The terms of G_i are added one by one over ascending p onto
// G0 (0.0, or the buffer on entry); multiply and add are separate (-ffp-contract=off) and the three multiplies are bracketed as written.
// Per chunk: the backward chain runs on the value chain's own kernels (k_bs_exact, k_bs_gemm) with their Z pointed into the state store
// SC_GST, X_i's block (i = 1 .. d-1) at (i - 1) ldx chunk doubles, row p of it at ldx p -- so val is ttx_basis_batch's bit for bit by
// construction; then, mode by mode, the accumulation of G_i from L_i and X_i and the advance of L through mode i (k_bg_exact_fwd,
// k_bg_gemm<MR, true> with a null D: their grad_i prologue is skipped).  L alternates between SC_XA and SC_XB.
//   exact (k_cg_exact): one thread per element (a, j, k), adjacent threads adjacent in a; it walks the chunk's points in ascending
//          order from the buffer's value: the order of the definition, whatever the chunk and the grid
//   MFMA  (k_cg_gemm<MR>): G_i as the GEMM (c o L_i)^T (phi_i (.) X_i) over the points, four per v_mfma_f64_16x16x4_f64.  Rows a in MR
//          tiles of 16; columns the flattened (j, k) at j + n k -- the packed block's own order -- in tiles of 16, CT = cg_ct(MR) per
//          wave, 64 CT per workgroup.  The points of a chunk are split into segments of CgStep::seg points (the plan's, from the shapes
//          and the points per chunk alone), one workgroup per column group and segment; a workgroup's partial block goes to its slot of SC_CGP
//          and k_cg_reduce adds the slots onto G_i in ascending order.  No floating-point atomics anywhere: a call repeats bit for bit.
//   k_cores_axpy: every core in one launch, in the engine's own layout (a + RM j + SS k), every element written at most once.
#pragma once
#if defined(__HIPCC__)
#include "ttx_basis_grad.h"

// G[e] <- G[e] + sum over p < c, ascending.  L = null: mode 1, L = (1); X = null: mode d, X = (1).  Rows of L and X at ldx p.
__global__ __launch_bounds__(256) void k_cg_exact(int r0, int n, int r1, long long c, const double *w, const double *phi, size_t ldphi,
                                                  const double *L, const double *X, int ldx, double *G)
{
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)r0 * n * r1) return;
    const int a = (int)(e % r0);
    const long long jk = e / r0;
    const int j = (int)(jk % n), k = (int)(jk / n);
    double g = G[e];
#pragma unroll 4
    for (long long p = 0; p < c; p++) {
        const double l = L ? L[(size_t)p * ldx + a] : 1.0, x = X ? X[(size_t)p * ldx + k] : 1.0;
        g = g + (w[p] * l) * (phi[(size_t)p * ldphi + j] * x);
    }
    G[e] = g;
}

// ---- MFMA -------------------------------------------------------------------------------------------------------------------------
// A workgroup (4 waves) owns 64 CT columns col = j + n k of the block, all 16 MR >= r0 rows of them and the points [seg y, seg (y + 1))
// of the chunk.  It walks its points in blocks of TTX_CG_PB = 16, fetched into registers one block ahead; of a block it stages in LDS
//   cl (pp, a) = c[p] * L(p, a)       at cg_lda(MR) pp + a    (the a operand: the product is rounded once, on its way into LDS)
//   pw (pp, w) = phi(p, (c0 + w) % n) at cg_ldw(MR) pp + w    (the table entries of the workgroup's columns, w = col - c0)
//   xs (pp, k) = X(p, k)              at cg_ldq(r1) pp + k
// zero for points past the segment and rows past r0; nothing is read out of range.  An MFMA step takes the four points pp = 4 s + kq:
// lane (col = l & 15, kq = l >> 4) gives a = cl(pp, 16 m + col) and b = pw(pp, w) * xs(pp, k(w)), formed in registers; a column past
// n r1 gives b = 0.0 itself (never 0 * something).  The operand layout is k_bs_gemm's: the accumulator register reg of lane (col, kq)
// holds row 16 m + kq + 4 reg of column col.  The partial block of segment y goes to P + y size, packed: (a, col) at a + r0 col.
template <int MR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(cg_waves(MR)))) void k_cg_gemm(int r0, int n, int r1, int c, int seg, const double *w, const double *phi, size_t ldphi,
                                                 const double *L, const double *X, int ldx, double *P)
{
    constexpr int CT = cg_ct(MR), W = 64 * CT, PB = TTX_CG_PB, RP = 16 * MR, lda = cg_lda(MR), ldw = cg_ldw(MR);
    extern __shared__ __align__(16) double cg_dyn[];
    const int ldq = cg_ldq(r1), rp = (r0 + 15) & ~15;
    double *cl = cg_dyn, *pw = cl + PB * lda, *xs = pw + PB * ldw;
    const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, col = l & 15, kq = l >> 4;
    const long long ncol = (long long)n * r1, c0 = (long long)blockIdx.x * W;
    const size_t size = (size_t)r0 * n * r1;
    const int p0 = blockIdx.y * seg, p1 = p0 + seg < c ? p0 + seg : c;

    // this lane's columns: offset in the window, k of the column, inside the block or not
    int ww[CT], wk[CT];
    bool ok[CT];
    dbl4 acc[CT][MR];
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        ww[ct] = (wave * CT + ct) * 16 + col;
        ok[ct] = c0 + ww[ct] < ncol;
        wk[ct] = ok[ct] ? (int)((c0 + ww[ct]) / n) : 0;
#pragma unroll
        for (int m = 0; m < MR; m++) acc[ct][m] = dbl4{0.0, 0.0, 0.0, 0.0};
    }
    // this thread's share of the staging: the window entry tid % W of the points tid / W + (256 / W) t, its table column
    const int sw = tid & (W - 1), spw = tid / W;
    const bool swok = c0 + sw < ncol;
    const int sj = swok ? (int)((c0 + sw) % n) : 0;
    const int sk = tid & 127, spk = tid >> 7;                                    // xs: entry k = tid % 128 of the points tid / 128 + 2 t

    // the rows of a block on their way into LDS: fetched into registers one block ahead, so that the global loads of the next block
    // are in flight during the MFMAs of this one
    constexpr int NCL = (PB * RP + 255) / 256, NPW = PB * W / 256, NXS = PB / 2;
    double vc[NCL], vp[NPW], vx[NXS];
    auto fetch = [&](int pb) {
#pragma unroll
        for (int t = 0; t < NCL; t++) {
            const int e = tid + 256 * t, pp = e / RP, a = e % RP, p = pb + pp;
            vc[t] = (e < PB * RP && p < p1 && a < r0) ? w[p] * (L ? L[(size_t)p * ldx + a] : 1.0) : 0.0;
        }
#pragma unroll
        for (int t = 0; t < NPW; t++) {
            const int p = pb + spw + (256 / W) * t;
            vp[t] = (p < p1 && swok) ? phi[(size_t)p * ldphi + sj] : 0.0;
        }
#pragma unroll
        for (int t = 0; t < NXS; t++) {
            const int p = pb + spk + 2 * t;
            vx[t] = (sk < r1 && p < p1) ? (X ? X[(size_t)p * ldx + sk] : 1.0) : 0.0;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int t = 0; t < NCL; t++) { const int e = tid + 256 * t; if (e < PB * RP) cl[(e / RP) * lda + e % RP] = vc[t]; }
#pragma unroll
        for (int t = 0; t < NPW; t++) pw[(spw + (256 / W) * t) * ldw + sw] = vp[t];
#pragma unroll
        for (int t = 0; t < NXS; t++) if (sk < r1) xs[(spk + 2 * t) * ldq + sk] = vx[t];
    };

    if (p0 < p1) fetch(p0);
    for (int pb = p0; pb < p1; pb += PB) {
        __syncthreads();                         // nobody reads the previous block any more
        stash();
        __syncthreads();
        if (pb + PB < p1) fetch(pb + PB);
#pragma unroll
        for (int s = 0; s < PB / 4; s++) {
            const int pp = 4 * s + kq;
            double b[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ct++) { const double v = pw[pp * ldw + ww[ct]] * xs[pp * ldq + wk[ct]]; b[ct] = ok[ct] ? v : 0.0; }
#pragma unroll
            for (int m = 0; m < MR; m++) {
                if (16 * m < rp) {
                    const double a = cl[pp * lda + 16 * m + col];
#pragma unroll
                    for (int ct = 0; ct < CT; ct++) acc[ct][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[ct], acc[ct][m], 0, 0, 0);
                }
            }
        }
    }
    double *Pb = P + (size_t)blockIdx.y * size;
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        if (!ok[ct]) continue;
        double *gp = Pb + (size_t)r0 * (size_t)(c0 + ww[ct]);
#pragma unroll
        for (int m = 0; m < MR; m++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) { const int row = 16 * m + kq + 4 * reg; if (row < r0) gp[row] = acc[ct][m][reg]; }
    }
}

// G[e] <- (.. ((G[e] + P_0[e]) + P_1[e]) ..) + P_(ns-1)[e]: the partial blocks of a chunk, in ascending order of their segments
__global__ __launch_bounds__(256) void k_cg_reduce(long long size, int ns, const double *P, double *G)
{
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < size; e += (long long)gridDim.x * blockDim.x) {
        double g = G[e];
        for (int s = 0; s < ns; s++) g = g + P[(size_t)s * (size_t)size + e];
        G[e] = g;
    }
}

// ---- U_i <- U_i + alpha_i G_i ----------------------------------------------------------------------------------------------------
// one core of the update: where it lies in the train, where its block starts in the packed gradient, the first element of the launch it owns
struct CaCore { double *U; long long goff, first; int r0, n, r1; double alpha; };
// element t of core i, (a, j, k) = (t % r0, t / r0 % n, t / (r0 n)): U(a + RM j + SS k) <- U + alpha * g[goff + t], multiply and add
// separate.  alpha == 0.0: the core is neither read nor written and its G_i is not read
__global__ __launch_bounds__(256) void k_cores_axpy(const CaCore *cs, int d, long long tot, int RM, size_t SS, const double *g)
{
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long long)gridDim.x * blockDim.x) {
        int lo = 0, hi = d - 1;                                                  // the last core with first <= e
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (cs[mid].first <= e) lo = mid; else hi = mid - 1; }
        const CaCore C = cs[lo];
        if (C.alpha == 0.0) continue;
        const long long t = e - C.first;
        const int a = (int)(t % C.r0);
        const long long jk = t / C.r0;
        double *u = C.U + a + (size_t)RM * (size_t)(jk % C.n) + SS * (size_t)(jk / C.n);
        *u = *u + C.alpha * g[C.goff + t];
    }
}
#endif
