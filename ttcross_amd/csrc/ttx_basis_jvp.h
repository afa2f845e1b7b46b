// ttx_basis_jvp.h -- the derivative of the resident tensor train in a function basis along a direction V in core space, at a BATCH of
// real points (ttx_basis_jvp_batch / ttx_basis_jvp_tab and their _dev forms): the other half of ttx_basis_core_grad.h.  That call is
// J^T c, points to cores; this one is J V, cores to points:
//     dval_p = sum_i f_(U_i <- V_i)(x_p),
// and with both a Gauss-Newton step is solved matrix-free (ttx_fit_plan.h).  Also here: the vector operations on packed core-space
// buffers that such a solver, or a caller's own optimiser, runs on the device (ttx_cores_dot, ttx_cores_axpby_dev).
//
// The definition of include/ttx.h.  Backward, mode i = d .. 1, from X = (1), Y = (0.0):
//     t_j(a) = sum_k U_i(a, j, k) X(k),  s_j(a) = sum_k U_i(a, j, k) Y(k),  v_j(a) = sum_k V_i(a, j, k) X(k)   (each from 0.0, ascending k)
//     z(a) = sum_j phi_j t_j(a),         y(a) = sum_j phi_j (s_j(a) + v_j(a))                                  (each from 0.0, ascending j)
// X <- z, Y <- y; val = z(1), dval = y(1) after mode 1.  Multiply and add are separate (-ffp-contract=off).  The z half is the
// operation sequence of ttx_basis.h, so val is ttx_basis_batch's bit for bit.  No state is kept: the chunk is the value call's.
// V is read IN PLACE from the packed buffer (block i at its offset, (a, j, k) at a + r0 (j + n k)) -- never copied into a second train.
// The two states of a chunk lie side by side in SC_XA / SC_XB: X's rows first, Y's rows ystr doubles behind them.
//   exact (k_jv_exact): k_bs_exact with the second state and the second core: one wave per point, the order of the definition
//   MFMA  (k_jv_gemm<MR>): the frame of k_bg_gemm<MR, false>.  Per panel two a images in LDS (U_i from the engine's layout, V_i from the
//          packed block, through a second address rule of the panel fetch), two b operands in registers (phi_j x_k and phi_j y_k),
//          two accumulator sets: z += U b_x; y += U b_y; y += V b_x -- three v_mfma_f64_16x16x4_f64 per tile and k-group.  The z
//          accumulators see k_bs_gemm's MFMA sequence.  A point's results depend on its own table rows and this fixed order only.
//   k_vec_dot: the fixed-order dot product of include/ttx.h (ttx_cores_dot); k_vec_axpby: y <- (alpha * x) + (beta * y);
//   k_fit_residual, k_fit_weigh: the solver's point vectors.
#pragma once
#if defined(__HIPCC__)
#include "ttx_basis_grad.h"

// ---- exact: one wave per point, grid-stride --------------------------------------------------------------------------------------
// dynamic LDS per wave: x[ldx], y[ldx].  X = null: the first step (mode d), X = (1), Y = (0.0).  The states: row p of X at X + ldx p, of Y at
// X + ystr + ldx p; the new ones to Z likewise.  last: mode 1 (r0 = 1): z goes to out[p] where out is not null, y to dout[p].
// V: block i of the packed direction.
__global__ __launch_bounds__(256) void k_jv_exact(EvTrain T, int i, long long c, const double *phi, size_t ldphi, const double *V, const double *X, double *Z,
                                                  size_t ystr, double *out, double *dout, int last)
{
    extern __shared__ __align__(16) double jv_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int q0 = T.r[i], q1 = T.r[i + 1], n = T.n[i], RM = T.RM;
    const size_t SS = T.SS, vs = (size_t)q0 * n;                                // V's stride in k
    const double *A = T.core[i];
    double *x = jv_dyn + (size_t)2 * T.ldx * wave, *y = x + T.ldx;
    for (long long p = (long long)blockIdx.x * nw + wave; p < c; p += (long long)gridDim.x * nw) {
        __builtin_amdgcn_wave_barrier();
        if (X) { for (int t = lane; t < q1; t += 64) { x[t] = X[(size_t)p * T.ldx + t]; y[t] = X[ystr + (size_t)p * T.ldx + t]; } }
        else if (lane == 0) { x[0] = 1.0; y[0] = 0.0; }
        __builtin_amdgcn_wave_barrier();
        const double *ph = phi + (size_t)p * ldphi;
        if (q0 <= 64) {
            if (lane < q0) {
                double z = 0.0, e = 0.0;
                for (int j = 0; j < n; j++) {
                    const double *Aj = A + (size_t)RM * j + lane, *Vj = V + (size_t)q0 * j + lane;
                    double t = 0.0, s = 0.0, v = 0.0;
#pragma unroll 4
                    for (int k = 0; k < q1; k++) {
                        const double u = Aj[SS * k], xk = x[k];
                        t = t + u * xk; s = s + u * y[k]; v = v + Vj[vs * k] * xk;
                    }
                    z = z + ph[j] * t;
                    e = e + ph[j] * (s + v);
                }
                if (last) { if (lane == 0) { if (out) out[p] = z; dout[p] = e; } }
                else { Z[(size_t)p * T.ldx + lane] = z; Z[ystr + (size_t)p * T.ldx + lane] = e; }
            }
        } else {                                                                // ranks above 64: two rows per lane
            const bool two = lane + 64 < q0;
            double z0 = 0.0, z1 = 0.0, e0 = 0.0, e1 = 0.0;
            for (int j = 0; j < n; j++) {
                const double *Aj = A + (size_t)RM * j + lane, *Bj = two ? Aj + 64 : Aj;
                const double *Vj = V + (size_t)q0 * j + lane, *Wj = two ? Vj + 64 : Vj;
                double t0 = 0.0, t1 = 0.0, s0 = 0.0, s1 = 0.0, v0 = 0.0, v1 = 0.0;
#pragma unroll 2
                for (int k = 0; k < q1; k++) {
                    const double xk = x[k], yk = y[k], u0 = Aj[SS * k], u1 = Bj[SS * k];
                    t0 = t0 + u0 * xk; t1 = t1 + u1 * xk;
                    s0 = s0 + u0 * yk; s1 = s1 + u1 * yk;
                    v0 = v0 + Vj[vs * k] * xk; v1 = v1 + Wj[vs * k] * xk;
                }
                const double pj = ph[j];
                z0 = z0 + pj * t0; z1 = z1 + pj * t1;
                e0 = e0 + pj * (s0 + v0); e1 = e1 + pj * (s1 + v1);
            }
            Z[(size_t)p * T.ldx + lane] = z0; Z[ystr + (size_t)p * T.ldx + lane] = e0;
            if (two) { Z[(size_t)p * T.ldx + lane + 64] = z1; Z[ystr + (size_t)p * T.ldx + lane + 64] = e1; }
        }
    }
}

// ---- MFMA -------------------------------------------------------------------------------------------------------------------------
// The frame of k_bs_gemm / k_bg_gemm<MR, false>: a workgroup of 4 waves owns TP = 64 CT points, CT = jv_ct(MR) column tiles of 16 per
// wave; the core is walked slice by slice and, inside a slice, in panels of TTX_BS_KPAN = 16 columns k, staged in LDS, double-buffered,
// one barrier per panel.  A buffer holds two images of rp x 16 (leading dimension ev_lda of the workgroup's rows): U's, then V's.  A lane holds the two
// states of its columns (8 MR doubles per column tile) and two accumulator sets (2 MR dbl4 per column tile): jv_ct and jv_waves
// (ttx_op_plan.h) are chosen so that no tier has scratch (profiles/basis_fit_mi355x.txt); above MR = 5 all rows of a column tile
// spill, so a workgroup there takes jv_mh(MR) = 3 or 4 row tiles and the grid's y counts the row groups: the same MFMAs, the states read twice.
// Lanes of padded points carry b = 0 and store nothing.
template <int MR>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(jv_waves(MR)))) void k_jv_gemm(EvTrain T, int i, int c, const double *phi, size_t ldphi, const double *V, const double *X, double *Z,
                                                 size_t ystr, double *out, double *dout, int last)
{
    constexpr int CT = jv_ct(MR), TP = 64 * CT, MH = jv_mh(MR);
    extern __shared__ __align__(16) double jv_dyn[];
    const int q0 = T.r[i], q1 = T.r[i + 1], n = T.n[i], RM = T.RM, ldx = T.ldx;
    const size_t SS = T.SS, vs = (size_t)q0 * n;
    // the rows of this workgroup: MH row tiles from rb (blockIdx.y: the upper tiers split their rows over two workgroups)
    const int rb = 16 * MH * blockIdx.y, rows = q0 - rb < 16 * MH ? q0 - rb : 16 * MH;
    if (rows <= 0) return;                       // the whole workgroup: nothing of this mode's output lies here
    const int lda = ev_lda(rows), rp = (rows + 15) & ~15, kp = (q1 + 3) & ~3, npan = (q1 + TTX_BS_KPAN - 1) / TTX_BS_KPAN, pan = lda * TTX_BS_KPAN;
    const int tid = threadIdx.x, wave = tid >> 6, l = tid & 63, col = l & 15, kq = l >> 4;
    const double *A = T.core[i];

    // this thread's share of a panel: elements e = tid + 256 s of the rp x 16 image, row a = e % rp, column kc = e / rp; the same
    // element of both images, U's through the engine's layout (a + RM j + SS k), V's through the packed block's (a + r0 (j + n k))
    int sl[MH], skc[MH];                        // LDS offset (-1: none), panel column
    long long sg[MH], sh[MH];                   // global offset of (a, j = 0, k = kc) in U and in V, -1: a padded row
#pragma unroll
    for (int s = 0; s < MH; s++) {
        const int e = tid + 256 * s, a = e % rp, kc = e / rp;
        sl[s] = e < rp * TTX_BS_KPAN ? a + lda * kc : -1;
        skc[s] = kc;
        sg[s] = a < rows ? (long long)(rb + a) + (long long)SS * kc : -1;
        sh[s] = a < rows ? (long long)(rb + a) + (long long)vs * kc : -1;
    }
    double su[MH], sv[MH];
    auto fetch = [&](int j, int pn) {
#pragma unroll
        for (int s = 0; s < MH; s++) {
            const bool in = sl[s] >= 0 && sg[s] >= 0 && TTX_BS_KPAN * pn + skc[s] < q1;
            su[s] = in ? A[(size_t)RM * j + (size_t)SS * (TTX_BS_KPAN * pn) + sg[s]] : 0.0;
            sv[s] = in ? V[(size_t)q0 * j + vs * (size_t)(TTX_BS_KPAN * pn) + sh[s]] : 0.0;
        }
    };
    auto stash = [&](double *B) {
#pragma unroll
        for (int s = 0; s < MH; s++) if (sl[s] >= 0) { B[sl[s]] = su[s]; B[pan + sl[s]] = sv[s]; }
    };

    // the points of this lane's columns, their table rows and their two states
    int pt[CT];
    const double *ph[CT];
    double x[CT][4 * MR], y[CT][4 * MR];
    dbl4 acc[CT][MH], acy[CT][MH];
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        const long long p = (long long)blockIdx.x * TP + (wave * CT + ct) * 16 + col;
        pt[ct] = p < c ? (int)p : -1;
        ph[ct] = phi + (size_t)(p < c ? p : 0) * ldphi;
#pragma unroll
        for (int kk = 0; kk < 4 * MR; kk++) {
            const int k = 4 * kk + kq;
            const bool in = pt[ct] >= 0 && k < q1;
            x[ct][kk] = in ? (X ? X[(size_t)pt[ct] * ldx + k] : 1.0) : 0.0;      // X = null: X = (1), Y = (0.0), q1 = 1
            y[ct][kk] = (in && X) ? X[ystr + (size_t)pt[ct] * ldx + k] : 0.0;
        }
#pragma unroll
        for (int m = 0; m < MH; m++) { acc[ct][m] = dbl4{0.0, 0.0, 0.0, 0.0}; acy[ct][m] = dbl4{0.0, 0.0, 0.0, 0.0}; }
    }

    fetch(0, 0);
    stash(jv_dyn);
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
                __syncthreads();                 // the panels in buffer cur are complete; nobody reads the other buffer any more
                const int npn = pn + 1 < npan ? pn + 1 : 0, nj = pn + 1 < npan ? j : j + 1;
                const bool more = nj < n;
                if (more) fetch(nj, npn);
                const double *B = jv_dyn + cur * 2 * pan;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (4 * (4 * pn + q) < kp) {
                        double b[CT], by[CT];
#pragma unroll
                        for (int ct = 0; ct < CT; ct++) { b[ct] = pj[ct] * x[ct][4 * pn + q]; by[ct] = pj[ct] * y[ct][4 * pn + q]; }
#pragma unroll
                        for (int m = 0; m < MH; m++) {
                            if (16 * m < rp) {
                                const int o = 16 * m + col + lda * (4 * q + kq);
                                const double a = B[o], av = B[pan + o];
#pragma unroll
                                for (int ct = 0; ct < CT; ct++) {
                                    acc[ct][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[ct], acc[ct][m], 0, 0, 0);
                                    acy[ct][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, by[ct], acy[ct][m], 0, 0, 0);
                                    acy[ct][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[ct], acy[ct][m], 0, 0, 0);
                                }
                            }
                        }
                    }
                }
                if (more) stash(jv_dyn + (cur ^ 1) * 2 * pan);
                cur ^= 1;
            }
        }
    }
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        if (pt[ct] < 0) continue;
        if (last) {                                                              // mode 1: r0 = 1, row 0 is lane group 0, register 0
            if (kq == 0) { if (out) out[pt[ct]] = acc[ct][0][0]; dout[pt[ct]] = acy[ct][0][0]; }
            continue;
        }
        double *zp = Z + (size_t)pt[ct] * ldx + rb, *yp = zp + ystr;
#pragma unroll
        for (int m = 0; m < MH; m++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const int row = 16 * m + kq + 4 * reg;
                if (row < rows) { zp[row] = acc[ct][m][reg]; yp[row] = acy[ct][m][reg]; }
            }
    }
}

// ---- vector operations on packed buffers -----------------------------------------------------------------------------------------
// the fixed-order dot product of include/ttx.h: workgroup s owns segment s, the elements [L s, min(L (s + 1), tot)), L a multiple of 256;
// lane t adds its products a_e * b_e, e = t mod 256, in ascending order from 0.0; the 256 lane sums are halved (t, t + 128), (t, t + 64)
// .. (0, 1); part[s] takes the segment's sum (0.0 for an empty segment).  The host adds the TTX_DOT_SEGS sums in ascending order.
__global__ __launch_bounds__(256) void k_vec_dot(long long tot, long long L, const double *a, const double *b, double *part)
{
    __shared__ double sm[256];
    const int t = threadIdx.x;
    const long long e0 = L * blockIdx.x, e1 = e0 + L < tot ? e0 + L : tot;
    double s = 0.0;
    for (long long e = e0 + t; e < e1; e += 256) s = s + a[e] * b[e];
    sm[t] = s;
    __syncthreads();
    for (int hlf = 128; hlf >= 1; hlf >>= 1) {
        if (t < hlf) sm[t] = sm[t] + sm[t + hlf];
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = sm[0];
}
// y_e <- (alpha * x_e) + (beta * y_e): two multiplies and one add, no special cases
__global__ __launch_bounds__(256) void k_vec_axpby(long long tot, double alpha, const double *x, double beta, double *y)
{
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (long long)gridDim.x * blockDim.x) y[e] = (alpha * x[e]) + (beta * y[e]);
}
// the solver's point vectors: res_p = val_p - y_p and c_p = w_p * res_p (w = null: c_p = res_p)
__global__ __launch_bounds__(256) void k_fit_residual(long long n, const double *val, const double *y, const double *w, double *res, double *c)
{
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        const double r = val[e] - y[e];
        res[e] = r;
        c[e] = w ? w[e] * r : r;
    }
}
// c_p = w_p * q_p
__global__ __launch_bounds__(256) void k_fit_weigh(long long n, const double *w, const double *q, double *c)
{
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) c[e] = w[e] * q[e];
}
#endif
