// ttx_basis.h -- the resident tensor train in a function basis at a BATCH of real points (ttx_basis_batch / ttx_basis_tab and
// their _dev forms, ttx_basis_host):  f(x_p) = sum_i T(i_1 .. i_d) prod_m phi_(m, i_m)(x_(p, m)).
//
// The chain of include/ttx.h, from the last mode to the first: x = (1); for mode i = d .. 1: t_j(a) = sum_k U_i(a, j, k) x(k) (from
// 0.0 over ascending k), z(a) = sum_j phi_j t_j(a) (from 0.0 over ascending j), x = z; the value is z(1) after mode 1.  Every
// multiply and add is separate (the library is built with -ffp-contract=off).  One launch per mode and chunk; the state of a chunk
// lives between the launches in two buffers of chunk x ldx doubles (SC_XA / SC_XB of the engine), element (p, a) at a + ldx p.
//   table (k_bs_table): phi of one mode for one chunk, chunk x n_i doubles, entry by entry from ttx_basis_entry -- the function
//          ttx_basis_host runs on the host, so the device tables equal the host tables bit for bit
//   exact (k_bs_exact): one wave per point in the frame of k_ev_exact: the state of the step in per-wave LDS, one row per lane, two
//          above rank 64, the operation order of the definition
//   MFMA  (k_bs_gemm<MR>): one step is the GEMM Z = U_(r0 x (n r1)) B with B = the row-wise Kronecker product phi_j(p) x_k(p), formed
//          in registers; v_mfma_f64_16x16x4_f64.  A point's value depends on its own column and on the fixed order (j ascending, k
//          ascending in quads) only: never on its neighbours, the tile, the chunk or npts.
// Open: a two-term path for TTX_BASIS_LINEAR (version one sums its table densely), complex tables, ranks > 128.
// The gradient (derivative tables, ttx_basis_dentry below) is ttx_basis_grad.h.
#pragma once
#include "ttx_coscoeff.h"   // ttx_cos, TTX_TRIG_MAX, TTX_COSCOEFF_PI, TTX_CC_HD: host and device

// w of a TTX_BASIS_COS mode
TTX_CC_HD double ttx_basis_cos_w(double a, double b) { return TTX_COSCOEFF_PI / (b - a); }

// phi_j(x) of one mode: the tables of include/ttx.h, entry by entry.  COS: w = ttx_basis_cos_w(a, b), nodes unused; LINEAR: a, w unused
TTX_CC_HD double ttx_basis_entry(int kind, int flags, double a, double w, const double *nodes, int n, double x, int j)
{
    if (kind == 1) {                                    // TTX_BASIS_COS
        const double y = (x - a) * w;
        const double arg = (double)j * y;
        const double aa = arg < 0.0 ? -arg : arg;
        if (!(aa <= TTX_TRIG_MAX)) return __builtin_nan("");
        const double c = ttx_cos(arg);
        return (j == 0 && (flags & 1)) ? c * 0.5 : c;
    }
    // TTX_BASIS_LINEAR: hat functions on strictly ascending nodes; i = the last node with t_i <= x, so t_i <= x < t_(i+1)
    if (x != x) return __builtin_nan("");
    if (n == 1) return 1.0;
    if (x <= nodes[0]) return j == 0 ? 1.0 : 0.0;
    if (x >= nodes[n - 1]) return j == n - 1 ? 1.0 : 0.0;
    if (j >= 1 && nodes[j - 1] <= x && x < nodes[j]) return (x - nodes[j - 1]) / (nodes[j] - nodes[j - 1]);           // i = j - 1: lambda
    if (j <= n - 2 && nodes[j] <= x && x < nodes[j + 1]) return 1.0 - (x - nodes[j]) / (nodes[j + 1] - nodes[j]);   // i = j: 1 - lambda
    return 0.0;
}

// dphi_j / dx of one mode, the derivative tables of include/ttx.h (ttx_basis_grad_batch, ttx_basis_host_d), the arguments of
// ttx_basis_entry.  COS: the y, arg and NaN rule of ttx_basis_entry; TTX_BASIS_HALVE_FIRST touches j = 0 only, which is 0.0 anyway.
// LINEAR: the derivative of the branch ttx_basis_entry takes, so at an interior node the right-hand derivative
TTX_CC_HD double ttx_basis_dentry(int kind, int flags, double a, double w, const double *nodes, int n, double x, int j)
{
    (void)flags;
    if (kind == 1) {                                    // TTX_BASIS_COS
        const double y = (x - a) * w;
        const double arg = (double)j * y;
        const double aa = arg < 0.0 ? -arg : arg;
        if (!(aa <= TTX_TRIG_MAX)) return __builtin_nan("");
        if (j == 0) return 0.0;
        return -(((double)j * w) * ttx_sin(arg));
    }
    if (x != x) return __builtin_nan("");
    if (n == 1 || x <= nodes[0] || x >= nodes[n - 1]) return 0.0;
    if (j >= 1 && nodes[j - 1] <= x && x < nodes[j]) return 1.0 / (nodes[j] - nodes[j - 1]);           // i = j - 1: d lambda
    if (j <= n - 2 && nodes[j] <= x && x < nodes[j + 1]) return -(1.0 / (nodes[j + 1] - nodes[j]));   // i = j: d (1 - lambda)
    return 0.0;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "ttx_eval.h"      // EvTrain
#include "ttx_op_plan.h"   // TTX_BS_KPAN, bs_ct, ev_lda

// one mode's basis as the table kernel takes it
struct BsMode { int kind, flags, n; double a, w; const double *nodes; };

// tab[j + n p] = phi_j(x[ldx p]) for p < c: one thread per entry, grid-stride
__global__ __launch_bounds__(256) void k_bs_table(BsMode M, long long c, const double *x, int ldx, double *tab)
{
    const long long tot = c * M.n;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long long)gridDim.x * blockDim.x) {
        const long long p = e / M.n;
        tab[e] = ttx_basis_entry(M.kind, M.flags, M.a, M.w, M.nodes, M.n, x[(size_t)p * ldx], (int)(e - p * M.n));
    }
}

// ---- exact: one wave per point, grid-stride --------------------------------------------------------------------------------------
// dynamic LDS per wave: x[ldx].  X = null: the first step of the chain (mode d), x = (1).  out != null: the last step (mode 1, r0 = 1),
// the value goes to out[p]; otherwise the new state goes to Z.  phi: the table of this mode, row p at phi + ldphi p.
__global__ __launch_bounds__(256) void k_bs_exact(EvTrain T, int i, long long c, const double *phi, size_t ldphi, const double *X, double *Z, double *out)
{
    extern __shared__ __align__(16) double bs_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int q0 = T.r[i], q1 = T.r[i + 1], n = T.n[i], RM = T.RM;
    const size_t SS = T.SS;
    const double *A = T.core[i];
    double *x = bs_dyn + (size_t)T.ldx * wave;
    for (long long p = (long long)blockIdx.x * nw + wave; p < c; p += (long long)gridDim.x * nw) {
        __builtin_amdgcn_wave_barrier();
        if (X) { for (int t = lane; t < q1; t += 64) x[t] = X[(size_t)p * T.ldx + t]; }
        else if (lane == 0) x[0] = 1.0;
        __builtin_amdgcn_wave_barrier();
        const double *ph = phi + (size_t)p * ldphi;
        if (q0 <= 64) {
            if (lane < q0) {
                double z = 0.0;
                for (int j = 0; j < n; j++) {
                    const double *Aj = A + (size_t)RM * j + lane;
                    double t = 0.0;
#pragma unroll 8
                    for (int k = 0; k < q1; k++) t = t + Aj[SS * k] * x[k];
                    z = z + ph[j] * t;
                }
                if (out) { if (lane == 0) out[p] = z; } else Z[(size_t)p * T.ldx + lane] = z;
            }
        } else {                                                                // ranks above 64: two rows per lane
            const bool two = lane + 64 < q0;
            double z0 = 0.0, z1 = 0.0;
            for (int j = 0; j < n; j++) {
                const double *Aj = A + (size_t)RM * j + lane, *Bj = two ? Aj + 64 : Aj;
                double t0 = 0.0, t1 = 0.0;
#pragma unroll 4
                for (int k = 0; k < q1; k++) { const double xk = x[k]; t0 = t0 + Aj[SS * k] * xk; t1 = t1 + Bj[SS * k] * xk; }
                const double pj = ph[j];
                z0 = z0 + pj * t0; z1 = z1 + pj * t1;
            }
            Z[(size_t)p * T.ldx + lane] = z0;
            if (two) Z[(size_t)p * T.ldx + lane + 64] = z1;
        }
    }
}

// ---- MFMA -------------------------------------------------------------------------------------------------------------------------
// A workgroup (4 waves) owns a tile of TP = 64 CT points: every wave CT column tiles of 16, CT chosen so that a lane's registers --
// the state x_k(pt) of its columns (4 MR doubles per column tile) and all accumulator tiles (MR dbl4 per column tile) -- leave room
// for two waves per SIMD up to MR = 6 (no scratch at any MR; the figures per MR are in profiles/basis_mi355x.txt): MR <= 2: CT = 4
// (TP = 256 = TTX_EV_TP), MR <= 4: CT = 2, else CT = 1.  MR = row tiles = k panels: 16 MR >= max(r0, r1).
// The core is walked slice by slice (j = 0 .. n-1) and, inside a slice, in panels of TTX_BS_KPAN = 16 columns k; a panel (r0 rounded
// up to 16 rows x 16 columns, zero-padded, leading dimension ev_lda(r0)) is staged in LDS, double-buffered: the global loads of the
// next panel are issued before the MFMAs of the current one and stored to the other buffer after them, one barrier per panel.
// Every MFMA takes a = U(16 m + col, j, k) from LDS and b = phi_j(pt) * x_k(pt), formed in registers; the accumulators run over all
// j and k of the mode, the new state is written once.  Lanes of padded points carry b = 0 and store nothing.
// TTX_BS_KPAN, bs_ct and bs_gemm_lds are in ttx_op_plan.h, shared with the call's plan

template <int MR>
__global__ __launch_bounds__(256) void k_bs_gemm(EvTrain T, int i, int c, const double *phi, size_t ldphi, const double *X, double *Z, double *out)
{
    constexpr int CT = bs_ct(MR), TP = 64 * CT;
    extern __shared__ __align__(16) double bs_dyn[];
    const int q0 = T.r[i], q1 = T.r[i + 1], n = T.n[i], RM = T.RM, ldx = T.ldx;
    const size_t SS = T.SS;
    const int lda = ev_lda(q0), rp = (q0 + 15) & ~15, kp = (q1 + 3) & ~3, npan = (q1 + TTX_BS_KPAN - 1) / TTX_BS_KPAN, pan = lda * TTX_BS_KPAN;
    const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, col = l & 15, kq = l >> 4;
    const double *A = T.core[i];

    // this thread's share of a panel: elements e = tid + 256 s of the rp x 16 image, row a = e % rp, column kc = e / rp
    int sl[MR], skc[MR];                        // LDS offset (-1: none), panel column
    long long sg[MR];                           // global offset of (a, j = 0, k = kc), -1: a padded row
#pragma unroll
    for (int s = 0; s < MR; s++) {
        const int e = tid + 256 * s, a = e % rp, kc = e / rp;
        sl[s] = e < rp * TTX_BS_KPAN ? a + lda * kc : -1;
        skc[s] = kc;
        sg[s] = a < q0 ? (long long)a + (long long)SS * kc : -1;
    }
    double sv[MR];
    auto fetch = [&](int j, int pn) {
#pragma unroll
        for (int s = 0; s < MR; s++)
            sv[s] = (sl[s] >= 0 && sg[s] >= 0 && TTX_BS_KPAN * pn + skc[s] < q1) ? A[(size_t)RM * j + (size_t)SS * (TTX_BS_KPAN * pn) + sg[s]] : 0.0;
    };
    auto stash = [&](double *B) {
#pragma unroll
        for (int s = 0; s < MR; s++) if (sl[s] >= 0) B[sl[s]] = sv[s];
    };

    // the points of this lane's columns, their table rows and their states
    int pt[CT];
    const double *ph[CT];
    double x[CT][4 * MR];
    dbl4 acc[CT][MR];
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        const long long p = (long long)blockIdx.x * TP + (wave * CT + ct) * 16 + col;
        pt[ct] = p < c ? (int)p : -1;
        ph[ct] = phi + (size_t)(p < c ? p : 0) * ldphi;
#pragma unroll
        for (int kk = 0; kk < 4 * MR; kk++) {
            const int k = 4 * kk + kq;
            x[ct][kk] = (pt[ct] >= 0 && k < q1) ? (X ? X[(size_t)pt[ct] * ldx + k] : 1.0) : 0.0;     // X = null: x = (1), q1 = 1
        }
#pragma unroll
        for (int m = 0; m < MR; m++) acc[ct][m] = dbl4{0.0, 0.0, 0.0, 0.0};
    }

    fetch(0, 0);
    stash(bs_dyn);
    int cur = 0;
    double pn_[CT];                              // phi_j of the columns, loaded one slice ahead
#pragma unroll
    for (int ct = 0; ct < CT; ct++) pn_[ct] = pt[ct] >= 0 ? ph[ct][0] : 0.0;
    for (int j = 0; j < n; j++) {
        double pj[CT];
#pragma unroll
        for (int ct = 0; ct < CT; ct++) { pj[ct] = pn_[ct]; if (j + 1 < n) pn_[ct] = pt[ct] >= 0 ? ph[ct][j + 1] : 0.0; }
#pragma unroll
        for (int pn = 0; pn < MR; pn++) {
            if (pn < npan) {
                __syncthreads();                 // the panel in buffer cur is complete; nobody reads the other buffer any more
                const int npn = pn + 1 < npan ? pn + 1 : 0, nj = pn + 1 < npan ? j : j + 1;
                const bool more = nj < n;
                if (more) fetch(nj, npn);
                const double *B = bs_dyn + cur * pan;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (4 * (4 * pn + q) < kp) {
                        double b[CT];
#pragma unroll
                        for (int ct = 0; ct < CT; ct++) b[ct] = pj[ct] * x[ct][4 * pn + q];
#pragma unroll
                        for (int m = 0; m < MR; m++) {
                            if (16 * m < rp) {
                                const double a = B[16 * m + col + lda * (4 * q + kq)];
#pragma unroll
                                for (int ct = 0; ct < CT; ct++) acc[ct][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[ct], acc[ct][m], 0, 0, 0);
                            }
                        }
                    }
                }
                if (more) stash(bs_dyn + (cur ^ 1) * pan);
                cur ^= 1;
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        if (pt[ct] < 0) continue;
        if (out) { if (kq == 0) out[pt[ct]] = acc[ct][0][0]; continue; }         // mode 1: r0 = 1, row 0 is lane group 0, register 0
        double *zp = Z + (size_t)pt[ct] * ldx;
#pragma unroll
        for (int m = 0; m < MR; m++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) { const int row = 16 * m + kq + 4 * reg; if (row < q0) zp[row] = acc[ct][m][reg]; }
    }
}
#endif
