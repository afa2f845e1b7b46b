// ttx_basis_grad.h -- value and gradient of the resident tensor train in a function basis at a BATCH of real points
// (ttx_basis_grad_batch / ttx_basis_grad_tab and their _dev forms):  grad_m f(x_p) = the chain of ttx_basis.h with mode m's table
// phi replaced by its derivative table dphi.  All d partial derivatives come from one backward and one forward pass, about three
// value chains, instead of d of them.
//
// The definition of include/ttx.h.  Backward, mode i = d .. 1, from x = (1): t_j(a) = sum_k U_i(a, j, k) x(k) (from 0.0 over ascending
// k), z(a) = sum_j phi_j t_j(a), e(a) = sum_j dphi_j t_j(a) (both from 0.0 over ascending j); D_i = e, x = z; val = z(1) after mode 1:
// the operation sequence of ttx_basis_batch.  Forward, mode i = 1 .. d, from l = (1): grad_i = sum_a l(a) D_i(a) (from 0.0 over
// ascending a), s_j(k) = sum_a l(a) U_i(a, j, k) (from 0.0 over ascending a), l(k) = sum_j phi_j s_j(k) (from 0.0 over ascending j);
// the last l is not formed.  Multiply and add are separate (-ffp-contract=off).
// One launch per mode, pass and chunk.  The states x and l of a chunk live in SC_XA / SC_XB as in ttx_basis.h; the rows D_i of all
// modes of a chunk live in the state store SC_GST, mode i's block at soff(i) chunk doubles, row p of it at r(i-1) p:
// S = sum_i r(i-1) doubles per point, which is what bounds the chunk (bg_plan, ttx_op_plan.h).
//   table    (k_bg_table): phi and dphi of one mode for one chunk in one launch, entry by entry from ttx_basis_entry and
//            ttx_basis_dentry -- the functions ttx_basis_host and ttx_basis_host_d run on the host
//   exact    (k_bg_exact_back, k_bg_exact_fwd): one wave per point in the frame of k_bs_exact, the operation order of the definition
//   MFMA     (k_bg_gemm<MR, FWD>): the design of k_bs_gemm.  Backward: a second operand b' = dphi_j x_k and a second accumulator set
//            take the same a fragment, so one pass over the core feeds z and e; the z accumulators see the MFMA sequence of
//            k_bs_gemm, so val equals ttx_basis_batch's bit for bit.  Forward: the transposed step l_new(k) = sum_(j, a) U(a, j, k)
//            [phi_j l(a)]: the rows are k, the contraction runs over (j, a), the panels are staged along a, which is contiguous in
//            memory.  grad_i = l . D_i is formed first, per lane group over its own a = 4 kk + kq ascending, then (p_0 + p_1) +
//            (p_2 + p_3) across the four groups.  A point's results depend on its own table rows and on this fixed order only.
#pragma once
#if defined(__HIPCC__)
#include "ttx_basis.h"

// tab[j + n p] = phi_j(x[ldx p]) and, where dtab is not null, dtab[j + n p] = dphi_j(x[ldx p]) for p < c: one thread per entry
__global__ __launch_bounds__(256) void k_bg_table(BsMode M, long long c, const double *x, int ldx, double *tab, double *dtab)
{
    const long long tot = c * M.n;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long long)gridDim.x * blockDim.x) {
        const long long p = e / M.n;
        const double xp = x[(size_t)p * ldx];
        const int j = (int)(e - p * M.n);
        tab[e] = ttx_basis_entry(M.kind, M.flags, M.a, M.w, M.nodes, M.n, xp, j);
        if (dtab) dtab[e] = ttx_basis_dentry(M.kind, M.flags, M.a, M.w, M.nodes, M.n, xp, j);
    }
}

// ---- exact: one wave per point, grid-stride --------------------------------------------------------------------------------------
// backward step of mode i: k_bs_exact with a second accumulator e for the derivative table; D (row p at D + q0 p) takes e.
// dynamic LDS per wave: x[ldx].  X = null: the first step (mode d), x = (1).  last: mode 1 (r0 = 1): z goes to out[p] where out is
// not null, no state is written.
__global__ __launch_bounds__(256) void k_bg_exact_back(EvTrain T, int i, long long c, const double *phi, const double *dphi, size_t ldphi,
                                                       const double *X, double *Z, double *D, double *out, int last)
{
    extern __shared__ __align__(16) double bg_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int q0 = T.r[i], q1 = T.r[i + 1], n = T.n[i], RM = T.RM;
    const size_t SS = T.SS;
    const double *A = T.core[i];
    double *x = bg_dyn + (size_t)T.ldx * wave;
    for (long long p = (long long)blockIdx.x * nw + wave; p < c; p += (long long)gridDim.x * nw) {
        __builtin_amdgcn_wave_barrier();
        if (X) { for (int t = lane; t < q1; t += 64) x[t] = X[(size_t)p * T.ldx + t]; }
        else if (lane == 0) x[0] = 1.0;
        __builtin_amdgcn_wave_barrier();
        const double *ph = phi + (size_t)p * ldphi, *dh = dphi + (size_t)p * ldphi;
        double *Dp = D + (size_t)p * q0;
        if (q0 <= 64) {
            if (lane < q0) {
                double z = 0.0, e = 0.0;
                for (int j = 0; j < n; j++) {
                    const double *Aj = A + (size_t)RM * j + lane;
                    double t = 0.0;
#pragma unroll 8
                    for (int k = 0; k < q1; k++) t = t + Aj[SS * k] * x[k];
                    z = z + ph[j] * t;
                    e = e + dh[j] * t;
                }
                Dp[lane] = e;
                if (last) { if (out && lane == 0) out[p] = z; } else Z[(size_t)p * T.ldx + lane] = z;
            }
        } else {                                                                // ranks above 64: two rows per lane
            const bool two = lane + 64 < q0;
            double z0 = 0.0, z1 = 0.0, e0 = 0.0, e1 = 0.0;
            for (int j = 0; j < n; j++) {
                const double *Aj = A + (size_t)RM * j + lane, *Bj = two ? Aj + 64 : Aj;
                double t0 = 0.0, t1 = 0.0;
#pragma unroll 4
                for (int k = 0; k < q1; k++) { const double xk = x[k]; t0 = t0 + Aj[SS * k] * xk; t1 = t1 + Bj[SS * k] * xk; }
                const double pj = ph[j], dj = dh[j];
                z0 = z0 + pj * t0; z1 = z1 + pj * t1;
                e0 = e0 + dj * t0; e1 = e1 + dj * t1;
            }
            Z[(size_t)p * T.ldx + lane] = z0; Dp[lane] = e0;
            if (two) { Z[(size_t)p * T.ldx + lane + 64] = z1; Dp[lane + 64] = e1; }
        }
    }
}

// forward step of mode i.  dynamic LDS per wave: l[ldx], D_i's row [ldx].  Lin = null: mode 1, l = (1).  grad_i goes to
// grad[i + d p] (D = null: no grad_i is formed, the advance alone: ttx_basis_core_grad.h); last (mode d): no new state.  Lane k (and k + 64) owns l_new(k) and walks a ascending, contiguous in memory.
__global__ __launch_bounds__(256) void k_bg_exact_fwd(EvTrain T, int i, long long c, const double *phi, size_t ldphi, const double *Lin, double *Lout,
                                                      const double *D, double *grad, int d, int last)
{
    extern __shared__ __align__(16) double bg_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int q0 = T.r[i], q1 = T.r[i + 1], n = T.n[i], RM = T.RM;
    const size_t SS = T.SS;
    const double *A = T.core[i];
    double *l = bg_dyn + (size_t)2 * T.ldx * wave, *dd = l + T.ldx;
    for (long long p = (long long)blockIdx.x * nw + wave; p < c; p += (long long)gridDim.x * nw) {
        __builtin_amdgcn_wave_barrier();
        if (Lin) { for (int t = lane; t < q0; t += 64) l[t] = Lin[(size_t)p * T.ldx + t]; }
        else if (lane == 0) l[0] = 1.0;
        if (D) for (int t = lane; t < q0; t += 64) dd[t] = D[(size_t)p * q0 + t];
        __builtin_amdgcn_wave_barrier();
        if (D && lane == 0) {
            double g = 0.0;
            for (int a = 0; a < q0; a++) g = g + l[a] * dd[a];
            grad[(size_t)p * d + i] = g;
        }
        if (last) continue;
        const double *ph = phi + (size_t)p * ldphi;
        for (int k = lane; k < q1; k += 64) {
            const double *Ak = A + SS * k;
            double z = 0.0;
            for (int j = 0; j < n; j++) {
                const double *Aj = Ak + (size_t)RM * j;
                double s = 0.0;
#pragma unroll 8
                for (int a = 0; a < q0; a++) s = s + l[a] * Aj[a];
                z = z + ph[j] * s;
            }
            Lout[(size_t)p * T.ldx + k] = z;
        }
    }
}

// ---- MFMA -------------------------------------------------------------------------------------------------------------------------
// The frame of k_bs_gemm (ttx_basis.h): a workgroup of 4 waves owns TP = 64 CT points, every wave CT column tiles of 16; the core is
// walked slice by slice and, inside a slice, in panels of TTX_BS_KPAN = 16 contraction indices, staged in LDS, double-buffered, one
// barrier per panel.  MR = row tiles = panels: 16 MR >= max(r0, r1).
//   FWD = false (backward step): rows a < r0, contraction k < r1; the panel image is (a, kc) at a + lda kc as in k_bs_gemm.  Two
//         operands per MFMA pair, b = phi_j x_k and b' = dphi_j x_k, two accumulator sets (z and e) from one a fragment: CT = bg_ct(MR).
//   FWD = true (forward step): rows k < r1, contraction a < r0; the panel image is (k, ac) at TTX_BG_LDT k + ac, read from global
//         memory along a.  One operand b = phi_j l(a), one accumulator set: CT = bs_ct(MR).  Before the GEMM the kernel forms grad_i (not where D is null).
// The figures per MR (registers, LDS, occupancy; no scratch at any MR) are in profiles/basis_grad_mi355x.txt.
// Where both accumulator sets fit into 256 registers the allocator is held to two waves per SIMD (bg_waves, ttx_op_plan.h).
template <int MR, bool FWD>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(bg_waves(MR, FWD)))) void k_bg_gemm(EvTrain T, int i, int c, const double *phi, const double *dphi, size_t ldphi, const double *X, double *Z,
                                                 double *D, double *out, double *grad, int d, int last)
{
    constexpr int CT = FWD ? bs_ct(MR) : bg_ct(MR), TP = 64 * CT;
    extern __shared__ __align__(16) double bg_dyn[];
    const int q0 = T.r[i], q1 = T.r[i + 1], n = T.n[i], RM = T.RM, ldx = T.ldx;
    const size_t SS = T.SS;
    const int R = FWD ? q1 : q0, K = FWD ? q0 : q1;                             // output rows, contraction length
    const int lda = ev_lda(R), rp = (R + 15) & ~15, kp = (K + 3) & ~3, npan = (K + TTX_BS_KPAN - 1) / TTX_BS_KPAN;
    const int pan = FWD ? TTX_BG_LDT * rp : lda * TTX_BS_KPAN;
    const size_t pstr = FWD ? (size_t)TTX_BS_KPAN : SS * TTX_BS_KPAN;           // from one panel to the next in global memory
    const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, col = l & 15, kq = l >> 4;
    const double *A = T.core[i];

    // this thread's share of a panel: elements e = tid + 256 s of the rp x 16 image; backward: row = e % rp, kc = e / rp; forward: kc = e % 16, row = e / 16
    int sl[MR], skc[MR];                        // LDS offset (-1: none), contraction index inside the panel
    long long sg[MR];                           // global offset of the element in panel 0 of slice 0, -1: a padded row
#pragma unroll
    for (int s = 0; s < MR; s++) {
        const int e = tid + 256 * s;
        const int row = FWD ? e / TTX_BS_KPAN : e % rp, kc = FWD ? e % TTX_BS_KPAN : e / rp;
        sl[s] = e < rp * TTX_BS_KPAN ? (FWD ? TTX_BG_LDT * row + kc : row + lda * kc) : -1;
        skc[s] = kc;
        sg[s] = row < R ? (FWD ? (long long)SS * row + kc : (long long)row + (long long)SS * kc) : -1;
    }
    double sv[MR];
    auto fetch = [&](int j, int pn) {
#pragma unroll
        for (int s = 0; s < MR; s++)
            sv[s] = (sl[s] >= 0 && sg[s] >= 0 && TTX_BS_KPAN * pn + skc[s] < K) ? A[(size_t)RM * j + pstr * pn + sg[s]] : 0.0;
    };
    auto stash = [&](double *B) {
#pragma unroll
        for (int s = 0; s < MR; s++) if (sl[s] >= 0) B[sl[s]] = sv[s];
    };

    // the points of this lane's columns, their table rows and their states
    int pt[CT];
    const double *ph[CT], *dh[CT];
    double x[CT][4 * MR];
    dbl4 acc[CT][MR], ace[FWD ? 1 : CT][FWD ? 1 : MR];
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        const long long p = (long long)blockIdx.x * TP + (wave * CT + ct) * 16 + col;
        pt[ct] = p < c ? (int)p : -1;
        ph[ct] = phi + (size_t)(p < c ? p : 0) * ldphi;
        dh[ct] = FWD ? nullptr : dphi + (size_t)(p < c ? p : 0) * ldphi;
#pragma unroll
        for (int kk = 0; kk < 4 * MR; kk++) {
            const int k = 4 * kk + kq;
            x[ct][kk] = (pt[ct] >= 0 && k < K) ? (X ? X[(size_t)pt[ct] * ldx + k] : 1.0) : 0.0;       // X = null: the state is (1), K = 1
        }
#pragma unroll
        for (int m = 0; m < MR; m++) {
            acc[ct][m] = dbl4{0.0, 0.0, 0.0, 0.0};
            if constexpr (!FWD) ace[ct][m] = dbl4{0.0, 0.0, 0.0, 0.0};
        }
    }

    if constexpr (FWD) {
        // grad_i = l . D_i: every lane group sums its own a = 4 kk + kq ascending, the four groups are paired (0 + 1) + (2 + 3)
#pragma unroll
        for (int ct = 0; D && ct < CT; ct++) {
            const double *Dp = D + (size_t)(pt[ct] >= 0 ? pt[ct] : 0) * q0;
            double g = 0.0;
#pragma unroll
            for (int kk = 0; kk < 4 * MR; kk++) {
                const int k = 4 * kk + kq;
                if (4 * kk < kp) g = g + x[ct][kk] * ((pt[ct] >= 0 && k < K) ? Dp[k] : 0.0);
            }
            g = g + __shfl_xor(g, 16, 64);
            g = g + __shfl_xor(g, 32, 64);
            if (pt[ct] >= 0 && kq == 0) grad[(size_t)pt[ct] * d + i] = g;
        }
        if (last) return;                       // mode d: the last l is not formed
    }

    fetch(0, 0);
    stash(bg_dyn);
    int cur = 0;
    double pn_[CT], dn_[CT];                     // phi_j (and dphi_j) of the columns, loaded one slice ahead
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        pn_[ct] = pt[ct] >= 0 ? ph[ct][0] : 0.0;
        dn_[ct] = (!FWD && pt[ct] >= 0) ? dh[ct][0] : 0.0;
    }
    for (int j = 0; j < n; j++) {
        double pj[CT], dj[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ct++) {
            pj[ct] = pn_[ct]; dj[ct] = dn_[ct];
            if (j + 1 < n) {
                pn_[ct] = pt[ct] >= 0 ? ph[ct][j + 1] : 0.0;
                if constexpr (!FWD) dn_[ct] = pt[ct] >= 0 ? dh[ct][j + 1] : 0.0;
            }
        }
#pragma unroll
        for (int pn = 0; pn < MR; pn++) {
            if (pn < npan) {
                __syncthreads();                 // the panel in buffer cur is complete; nobody reads the other buffer any more
                const int npn = pn + 1 < npan ? pn + 1 : 0, nj = pn + 1 < npan ? j : j + 1;
                const bool more = nj < n;
                if (more) fetch(nj, npn);
                const double *B = bg_dyn + cur * pan;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (4 * (4 * pn + q) < kp) {
                        double b[CT], bd[CT];
#pragma unroll
                        for (int ct = 0; ct < CT; ct++) {
                            b[ct] = pj[ct] * x[ct][4 * pn + q];
                            if constexpr (!FWD) bd[ct] = dj[ct] * x[ct][4 * pn + q];
                        }
#pragma unroll
                        for (int m = 0; m < MR; m++) {
                            if (16 * m < rp) {
                                const double a = FWD ? B[TTX_BG_LDT * (16 * m + col) + 4 * q + kq] : B[16 * m + col + lda * (4 * q + kq)];
#pragma unroll
                                for (int ct = 0; ct < CT; ct++) {
                                    acc[ct][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[ct], acc[ct][m], 0, 0, 0);
                                    if constexpr (!FWD) ace[ct][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bd[ct], ace[ct][m], 0, 0, 0);
                                }
                            }
                        }
                    }
                }
                if (more) stash(bg_dyn + (cur ^ 1) * pan);
                cur ^= 1;
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        if (pt[ct] < 0) continue;
        if constexpr (!FWD) {
            double *dp = D + (size_t)pt[ct] * q0;
            if (last) {                                                          // mode 1: r0 = 1, row 0 is lane group 0, register 0
                if (kq == 0) { if (out) out[pt[ct]] = acc[ct][0][0]; dp[0] = ace[ct][0][0]; }
                continue;
            }
#pragma unroll
            for (int m = 0; m < MR; m++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) { const int row = 16 * m + kq + 4 * reg; if (row < q0) dp[row] = ace[ct][m][reg]; }
        }
        double *zp = Z + (size_t)pt[ct] * ldx;
#pragma unroll
        for (int m = 0; m < MR; m++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) { const int row = 16 * m + kq + 4 * reg; if (row < R) zp[row] = acc[ct][m][reg]; }
    }
}
#endif
