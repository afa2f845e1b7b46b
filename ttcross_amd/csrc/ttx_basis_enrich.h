// ttx_basis_enrich.h -- grow the ranks of the resident train from data: gradient enrichment (ttx_basis_enrich_batch / _tab and their
// _dev forms).  To every bond i = 1 .. d-1 the call appends up to k_i directions of the two-site gradient
//     G2_i = sum_p c_p (L_i (x) phi_i)(phi_(i+1) (x) X_(i+1))^T
// that lie outside the range of core i's left unfolding; the new rows of core i+1 are zeros, so the function stays and the next fit step
// can move into the new directions.  G2_i (r n x n r) is never formed: it is sketched from the right with a random Omega_i,
//     z_q(p) = sum_j phi_(i+1, j)(p) (sum_b Omega_i(q, j, b) X_(i+1)(p, b)),    Y_i(a, j, q) = sum_p ((c[p] * L_i(p, a)) * (phi_(i, j)(p) * z_q(p))),
// the backward step of the value chain with Omega_i in place of core i+1, then G_i's formula of ttx_basis_core_grad.h with z for X_i.
//
// The definition is include/ttx.h's; tests/enrich_ref.py restates it.  Per chunk: the backward chain of ttx_basis_core_grad.h with every
// state kept (the value chain's own kernels), then forward over the bonds: z of the bond into the chunk's z block of the state store, Y_i
// accumulated from L_i and z, L advanced through mode i.  Every row of a state -- X, L and z -- has the stride EnPlan::ldx, the largest
// of the ranks and the k_i rounded up to four, so that the accumulation is ttx_basis_core_grad.h's own launch with z as its right operand
// and r1 = k_i: k_cg_exact in exact mode (the order of the definition, whatever the chunk and the grid), k_cg_gemm<MR> and k_cg_reduce in
// MFMA mode (segment partials added in ascending order, no atomics).  New here:
//   k_en_z_exact     one wave per point, lane q: t_j = sum_b Omega(q, j, b) X(b) from 0.0 over ascending b, z_q = sum_j phi_j t_j from 0.0
//                    over ascending j -- the restatement's order
//   k_en_z_gemm<QT>  z as the GEMM [phi (.) X] Omega^T on v_mfma_f64_16x16x4_f64: rows the points, the contraction index j + n b in steps
//                    of four, columns q in QT tiles of 16.  The a operand phi(p, j) * X(p, b) is formed in registers as the chain step does;
//                    the b operand is generated in registers from the hash and feeds en_pt(QT) point tiles
//   Omega is never stored: both kernels call rs_uniform(seed, i, q + k_i (j + n b)), ttx_lincomb_round's step-2 formula with the bond in
//   the mode field
//   k_en_stat        per bond and segment of ttx_cores_dot's rule: the segment's sum of squares and its largest |Y| (+Inf for a NaN)
//   k_en_pack        [U_i^L | 2^-e Y_i] into the QR's input, U read in place in the padded layout
//   k_en_assemble    all new cores in one launch: the U block copied, the Q block beside it, zeros written explicitly below
#pragma once
#include <stddef.h>

// one new core as k_en_assemble sees it (the plan fills the shapes, the engine the pointers)
struct EnCore {
    const double *U;                // core i of the source, padded layout
    const double *Q;                // the bond's new directions, r0 n x (R1 - r1) column-major; not read where R1 == r1
    double *dst;                    // core i of the new engine, padded layout
    long long first;                // the first element of the launch the core owns
    int r0, n, r1, R0, R1;          // source ranks; new ranks
};

#if defined(__HIPCC__)
#include "ttx_basis_core_grad.h"
#include "ttx_roundsum.h"           // rs_uniform

// Z[ldx p + q] = z_q(p) for p < c, q < k.  X = null: the last bond, X_d = (1), r1 = 1.
__global__ __launch_bounds__(256) void k_en_z_exact(unsigned long long seed, int bond, int k, int n, int r1, long long c, const double *phi, size_t ldphi,
                                                    const double *X, int ldx, double *Z)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (long long p = (long long)blockIdx.x * nw + wave; p < c; p += (long long)gridDim.x * nw) {
        const double *ph = phi + (size_t)p * ldphi, *x = X ? X + (size_t)p * ldx : nullptr;
        for (int q = lane; q < k; q += 64) {
            double z = 0.0;
            for (int j = 0; j < n; j++) {
                double t = 0.0;
                for (int b = 0; b < r1; b++)
                    t = t + rs_uniform(seed, bond, (unsigned long long)q + (unsigned long long)k * ((unsigned long long)j + (unsigned long long)n * b)) * (x ? x[b] : 1.0);
                z = z + ph[j] * t;
            }
            Z[(size_t)p * ldx + q] = z;
        }
    }
}

// A workgroup (4 waves) owns 64 PT points, wave w the PT tiles of 16 from point 64 PT blockIdx.x + 16 PT w on.  An MFMA step takes the
// four contraction indices K = 4 s + kq, K = j + n b: lane (row = l & 15, kq = l >> 4) gives a = phi(p, j) * X(p, b) of its point in
// every tile and b = Omega(q = 16 t + (l & 15), j, b) of every column tile; an index past n r1, a point past c and a column past k
// give 0.0 itself (never 0 * something).  Accumulator register reg of lane (col, kq) holds point kq + 4 reg of the tile, column col.
template <int QT>
__global__ __launch_bounds__(256) void k_en_z_gemm(unsigned long long seed, int bond, int k, int n, int r1, int c, const double *phi, size_t ldphi,
                                                   const double *X, int ldx, double *Z)
{
    constexpr int PT = en_pt(QT);
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, col = l & 15, kq = l >> 4;
    const int pw = (blockIdx.x * 4 + wave) * 16 * PT;
    const int K = n * r1;
    dbl4 acc[PT][QT];
    const double *pp[PT], *px[PT];
    bool pok[PT];
#pragma unroll
    for (int t = 0; t < PT; t++) {
        const int p = pw + 16 * t + col;
        pok[t] = p < c;
        pp[t] = phi + (size_t)(pok[t] ? p : 0) * ldphi;
        px[t] = X ? X + (size_t)(pok[t] ? p : 0) * ldx : nullptr;
#pragma unroll
        for (int q = 0; q < QT; q++) acc[t][q] = dbl4{0.0, 0.0, 0.0, 0.0};
    }
    int j = kq % n, b = kq / n;                                                  // of K = 4 s + kq, walked without a division per step
    for (int K0 = 0; K0 < K; K0 += 4) {
        const bool kok = K0 + kq < K;
        double bv[QT];
#pragma unroll
        for (int q = 0; q < QT; q++) {
            const int qq = 16 * q + col;
            bv[q] = (kok && qq < k) ? rs_uniform(seed, bond, (unsigned long long)qq + (unsigned long long)k * (unsigned long long)(K0 + kq)) : 0.0;
        }
#pragma unroll
        for (int t = 0; t < PT; t++) {
            const double av = (kok && pok[t]) ? pp[t][j] * (px[t] ? px[t][b] : 1.0) : 0.0;
#pragma unroll
            for (int q = 0; q < QT; q++)
                if (16 * q < k) acc[t][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv[q], acc[t][q], 0, 0, 0);
        }
        j += 4;
        while (j >= n) { j -= n; b++; }
    }
#pragma unroll
    for (int t = 0; t < PT; t++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int p = pw + 16 * t + kq + 4 * reg;
            if (p >= c) continue;
#pragma unroll
            for (int q = 0; q < QT; q++) { const int qq = 16 * q + col; if (qq < k) Z[(size_t)p * ldx + qq] = acc[t][q][reg]; }
        }
}

// Workgroup (s, bond y): segment s of ttx_cores_dot's rule over Y_y (off[y] .. off[y + 1]): part[256 y + s] = the segment's sum of
// squares in k_vec_dot's order, mx[256 y + s] = its largest |Y|, +Inf where an entry is a NaN.  The host folds the 256 of a bond.
__global__ __launch_bounds__(256) void k_en_stat(const size_t *off, const double *Y, double *part, double *mx)
{
    __shared__ double sm[256];
    __shared__ double red[4];
    const int t = threadIdx.x;
    const double *y = Y + off[blockIdx.y];
    const long long tot = (long long)(off[blockIdx.y + 1] - off[blockIdx.y]), L = 256 * ((tot + 65535) / 65536);       // dot_seg(tot)
    const long long e0 = L * blockIdx.x, e1 = e0 + L < tot ? e0 + L : tot;
    double s = 0.0, m = 0.0;
    for (long long e = e0 + t; e < e1; e += 256) {
        const double v = y[e], a = fabs(v);
        s = s + v * v;
        m = a != a ? INFINITY : fmax(m, a);                                      // fmax would drop a NaN
    }
    sm[t] = s;
    __syncthreads();
    for (int hlf = 128; hlf >= 1; hlf >>= 1) {
        if (t < hlf) sm[t] = sm[t] + sm[t + hlf];
        __syncthreads();
    }
    m = block_max_xor(m, red);
    if (t == 0) { part[256 * blockIdx.y + blockIdx.x] = sm[0]; mx[256 * blockIdx.y + blockIdx.x] = m; }
}

// A (rows = r0 n, r1 + k columns, column-major) = [U^L | 2^-e Y]: U(a, j, b) at a + RM j + SS b, Y packed
__global__ __launch_bounds__(256) void k_en_pack(const double *U, int RM, size_t SS, int r0, int n, int r1, int k, const double *Y, int e, double *A)
{
    const long long rows = (long long)r0 * n, tot = rows * (r1 + k);
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < tot; x += (long long)gridDim.x * blockDim.x) {
        const long long row = x % rows, cl = x / rows;
        A[x] = cl < r1 ? U[(row % r0) + (size_t)RM * (size_t)(row / r0) + SS * (size_t)cl] : ldexp(Y[row + rows * (cl - r1)], -e);
    }
}

// element t of new core i, (a, j, b) = (t % R0, t / R0 % n, t / (R0 n)): the source's where a < r0 and b < r1, Q(a, j, b - r1) where
// a < r0 and b >= r1, 0.0 in the rows from r0 on.  Every element of the new cores is written once.
__global__ __launch_bounds__(256) void k_en_assemble(const EnCore *cs, int d, long long tot, int sRM, size_t sSS, int dRM, size_t dSS)
{
    for (long long x = (long long)blockIdx.x * blockDim.x + threadIdx.x; x < tot; x += (long long)gridDim.x * blockDim.x) {
        int lo = 0, hi = d - 1;                                                  // the last core with first <= x
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (cs[mid].first <= x) lo = mid; else hi = mid - 1; }
        const EnCore C = cs[lo];
        const long long t = x - C.first;
        const int a = (int)(t % C.R0);
        const long long jb = t / C.R0;
        const int j = (int)(jb % C.n), b = (int)(jb / C.n);
        double v = 0.0;
        if (a < C.r0) v = b < C.r1 ? C.U[a + (size_t)sRM * j + sSS * b] : C.Q[a + (size_t)C.r0 * ((size_t)j + (size_t)C.n * (size_t)(b - C.r1))];
        C.dst[a + (size_t)dRM * j + dSS * b] = v;
    }
}
#endif
