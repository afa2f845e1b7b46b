// ttx_quadfin.h -- the quadrature of the train (per sweep and at the end) and the finalisation dtt_lua.
#pragma once
#include "ttx_addr.h"

// ------------------------------------------------------------------------------------------------
// quadrature (lib/dmrgg.f90:975-993 per sweep, :1261-1415 dtt_quad) and finalisation dtt_lua (:1169-1258)
// ------------------------------------------------------------------------------------------------
// mode 0: T = sum_j w_j arg(:,j,:) on raw fibers, then L(p-1)^-1 T U(p)^-1 (ttqq + dtt_lua);
// mode 1: T = sum_j w_j arg(:,j,:) on finalised cores (w == NULL: plain sum)
__global__ __launch_bounds__(256) void k_quad_build(DevProb P, int mode, const double *wq)
{
    if (P.ctl[2]) return;
    extern __shared__ double T[];   // RM*RM
    const int g = blockIdx.y, tid = threadIdx.x, RM = P.RM;
    GroupState &gs = P.gs[g];
    const int first = gs.first, p = first + blockIdx.x;
    const bool lastgroup = (gs.gglobal == P.nprocs - 1);
    if (p > gs.last && !(lastgroup && p == P.d)) return;
    const int *r = P.r + (size_t)g * (P.d + 2);
    const int r0 = r[p - 1], r1 = r[p], n = P.n[p];
    const double *A = core_ptr(P, P.arg, g, p, first);
    const double *w = wq ? wq + (size_t)p * P.NM : nullptr;
    for (int x = tid; x < r0 * r1; x += blockDim.x) {
        int i = x % r0, k = x / r0;
        const double *a = A + i + P.SS * k;
        double y = 0.0;
        if (w) {
#pragma unroll 8
            for (int j = 0; j < n; j++) y = y + w[j] * a[(size_t)RM * j];        // dgemv 'n', :988 / :1327
        } else {
#pragma unroll 8
            for (int j = 0; j < n; j++) y = y + a[(size_t)RM * j];               // :1331
        }
        T[i + RM * k] = y;
    }
    __syncthreads();
    if (mode == 0) {
        const double *gL = inv_ptr(P, g, p - 1, first);
        if (tid < r1) {                               // d2_luar(n*r1 -> r1 columns, r0, inv(p-1)) :1250
            double *c = T + RM * tid;
            for (int t = 1; t < r0; t++) {
                double tmp = 0.0;
                for (int s = 0; s < t; s++) tmp = tmp + c[s] * gL[t * t + s];
                c[t] = c[t] + (-1.0) * tmp;
            }
        }
        __syncthreads();
        if (p <= gs.last && tid < r0) {               // d2_lual(r0 rows, r1, inv(p)) :1251
            const double *gU = inv_ptr(P, g, p, first);
            for (int t = 0; t < r1; t++) {
                double y = T[tid + RM * t];
                for (int s = 0; s < t; s++) y = y + (-gU[t * t + t + s]) * T[tid + RM * s];
                T[tid + RM * t] = (1.0 / gU[(t + 1) * (t + 1) - 1]) * y;
            }
        }
        __syncthreads();
    }
    double *out = P.Tq + ((size_t)g * P.NC + (p - first)) * (size_t)RM * RM;
    for (int x = tid; x < r0 * r1; x += blockDim.x) out[(x % r0) + RM * (x / r0)] = T[(x % r0) + RM * (x / r0)];
}

// chain product of the group's T matrices (dgemm 'n','n' order, :1340); one block per group
__global__ __launch_bounds__(256) void k_quad_chain(DevProb P)
{
    if (P.ctl[2]) return;
    extern __shared__ double sh[];  // 2*RM*RM
    const int g = blockIdx.x, tid = threadIdx.x, RM = P.RM;
    GroupState &gs = P.gs[g];
    const int first = gs.first;
    const bool lastgroup = (gs.gglobal == P.nprocs - 1);
    const int lastc = lastgroup ? P.d : gs.last;
    const int *r = P.r + (size_t)g * (P.d + 2);
    const int mym = r[first - 1];
    // the two chain matrices: LDS, or the group's global scratch when 2 RM^2 doubles exceed it (same block: barriers order the accesses)
    double *prev = P.qscr ? P.qscr + (size_t)g * 2 * RM * RM : sh, *next = prev + RM * RM;
    const double *T0 = P.Tq + ((size_t)g * P.NC) * (size_t)RM * RM;
    for (int x = tid; x < mym * r[first]; x += blockDim.x) prev[(x % mym) + RM * (x / mym)] = T0[(x % mym) + RM * (x / mym)];
    __syncthreads();
    for (int p = first + 1; p <= lastc; p++) {
        const double *Tc = P.Tq + ((size_t)g * P.NC + (p - first)) * (size_t)RM * RM;
        const int r0 = r[p - 1], r1 = r[p];
        for (int x = tid; x < mym * r1; x += blockDim.x) {
            int i = x % mym, j = x / mym;
            double c = 0.0;
#pragma unroll 8
            for (int l = 0; l < r0; l++) c = c + Tc[l + RM * j] * prev[i + RM * l];
            next[i + RM * j] = c;
        }
        __syncthreads();
        double *t = prev; prev = next; next = t;
    }
    const int myn = r[lastc];
    const int gg = gs.gglobal;
    double *out = P.qsend + (size_t)gg * RM * RM;
    for (int x = tid; x < mym * myn; x += blockDim.x) out[(x % mym) + RM * (x / mym)] = prev[(x % mym) + RM * (x / mym)];
    if (tid == 0) {
        double *dm = P.qsend + (size_t)P.nprocs * RM * RM;
        dm[2 * gg] = (double)mym; dm[2 * gg + 1] = (double)myn;
        if (P.nprocs == 1) gs.val = prev[0];
    }
}

// dtt_lua on the raw fibers: luar pass then lual pass (two launches: the second needs the whole core)
// lds != 0: the block's 256 columns (rows) and the packed LU live in LDS while the substitution runs -- same operations
// in the same order, but the O(r^2) walk no longer goes through global memory (90 -> ~25 us per launch at r = 20..32)
__global__ __launch_bounds__(256) void k_fin_luar(DevProb P, int lds)
{
    extern __shared__ double fsh[];
    const int g = blockIdx.y, RM = P.RM;
    GroupState &gs = P.gs[g];
    const int first = gs.first, p = first + blockIdx.x;
    const bool lastgroup = (gs.gglobal == P.nprocs - 1);
    if (p > gs.last && !(lastgroup && p == P.d)) return;
    const int *r = P.r + (size_t)g * (P.d + 2);
    const int r0 = r[p - 1], r1 = r[p], n = P.n[p];
    double *A = core_ptr(P, P.arg, g, p, first);
    const double *gL = inv_ptr(P, g, p - 1, first);
    if (lds) {
        double *sg = fsh, *sc = fsh + (size_t)RM * RM;               // LU | columns as [t][thread]
        const int tid = threadIdx.x;
        // the columns of a core are spread over the workgroups along grid.z (T = blockDim.x columns each): every column is independent
        const int T = blockDim.x;
        if ((int)(blockIdx.z * T) >= n * r1) return;
        for (int x = tid; x < r0 * r0; x += T) sg[x] = gL[x];
        for (int x0 = blockIdx.z * T; x0 < n * r1; x0 += gridDim.z * T) {
            const int x = x0 + tid;
            const bool on = x < n * r1;
            double *c = on ? A + (size_t)RM * (x % n) + P.SS * (x / n) : A;
            __syncthreads();
            if (on) for (int t = 0; t < r0; t++) sc[t * T + tid] = c[t];
            __syncthreads();                                         // (also: sg complete before the first use)
            if (on) {
                for (int t = 1; t < r0; t++) {
                    double tmp = 0.0;
#pragma unroll 8
                    for (int s = 0; s < t; s++) tmp = tmp + sc[s * T + tid] * sg[t * t + s];
                    sc[t * T + tid] = sc[t * T + tid] + (-1.0) * tmp;
                }
                for (int t = 1; t < r0; t++) c[t] = sc[t * T + tid];
            }
        }
        return;
    }
    for (int x = blockIdx.z * blockDim.x + threadIdx.x; x < n * r1; x += gridDim.z * blockDim.x) {       // one column (j,k) per thread, :1250
        double *c = A + (size_t)RM * (x % n) + P.SS * (x / n);
        for (int t = 1; t < r0; t++) {
            double tmp = 0.0;
            for (int s = 0; s < t; s++) tmp = tmp + c[s] * gL[t * t + s];
            c[t] = c[t] + (-1.0) * tmp;
        }
    }
}
__global__ __launch_bounds__(256) void k_fin_lual(DevProb P, int lds)
{
    extern __shared__ double fsh[];
    const int g = blockIdx.y, RM = P.RM;
    GroupState &gs = P.gs[g];
    const int first = gs.first, p = first + blockIdx.x;
    if (p > gs.last) return;
    const int *r = P.r + (size_t)g * (P.d + 2);
    const int r0 = r[p - 1], r1 = r[p], n = P.n[p];
    double *A = core_ptr(P, P.arg, g, p, first);
    const double *gU = inv_ptr(P, g, p, first);
    if (lds) {
        double *sg = fsh, *sc = fsh + (size_t)RM * RM;
        const int tid = threadIdx.x;
        const int T = blockDim.x;
        if ((int)(blockIdx.z * T) >= r0 * n) return;
        for (int x = tid; x < r1 * r1; x += T) sg[x] = gU[x];
        for (int x0 = blockIdx.z * T; x0 < r0 * n; x0 += gridDim.z * T) {
            const int x = x0 + tid;
            const bool on = x < r0 * n;
            double *c = on ? A + (x % r0) + (size_t)RM * (x / r0) : A;
            __syncthreads();
            if (on) for (int t = 0; t < r1; t++) sc[t * T + tid] = c[P.SS * t];
            __syncthreads();
            if (on) {
                for (int t = 0; t < r1; t++) {
                    double y = sc[t * T + tid];
#pragma unroll 8
                    for (int s = 0; s < t; s++) y = y + (-sg[t * t + t + s]) * sc[s * T + tid];
                    sc[t * T + tid] = (1.0 / sg[(t + 1) * (t + 1) - 1]) * y;
                }
                for (int t = 0; t < r1; t++) c[P.SS * t] = sc[t * T + tid];
            }
        }
        return;
    }
    for (int x = blockIdx.z * blockDim.x + threadIdx.x; x < r0 * n; x += gridDim.z * blockDim.x) {       // one row (i,j) per thread, :1251
        double *c = A + (x % r0) + (size_t)RM * (x / r0);
        for (int t = 0; t < r1; t++) {
            double y = c[P.SS * t];
            for (int s = 0; s < t; s++) y = y + (-gU[t * t + t + s]) * c[P.SS * s];
            c[P.SS * t] = (1.0 / gU[(t + 1) * (t + 1) - 1]) * y;
        }
    }
}

// binary-tree product of the partial quadrature matrices of ALL groups (lib/dmrgg.f90:1355-1405); single
// block, run redundantly by every GPU on the all-reduced P.qall so that every rank holds the same value
// lds != 0 (CreatePlan::lds_qtree): the matrices live in LDS, in two regions of ng matrices -- a product reads its two factors from
// the region each of them is in and writes the other region of the left one, so the products of a level need no copy back and no
// barrier between them.  Every entry is the same sum c = c + B(l,j) A(i,l) in the same l order as below: the bits stay.  What is
// gone are the loads of the dependent sums out of L2 (56 of the 57 us of this kernel at C_16) and two of three barriers per product.
__global__ __launch_bounds__(256) void k_quad_tree(DevProb P, int lds)
{
    if (P.ctl[2]) return;
    const int tid = threadIdx.x, RM = P.RM, ng = P.nprocs;
    __shared__ int mym[256], myn[256];
    const double *part = P.qall, *dims = P.qall + (size_t)ng * RM * RM;
    double *work = P.qwork;
    for (int g = tid; g < ng; g += blockDim.x) { mym[g] = (int)dims[2 * g]; myn[g] = (int)dims[2 * g + 1]; }
    __syncthreads();
    if (lds) {
        extern __shared__ double qsh[];
        __shared__ int wh[256];                         // the region group g's matrix is in
        const size_t MS = (size_t)RM * RM, REG = (size_t)ng * MS;
        for (int g = tid; g < ng; g += blockDim.x) wh[g] = 0;
        for (int g = 0; g < ng; g++)
            for (int x = tid; x < mym[g] * myn[g]; x += blockDim.x) qsh[(size_t)g * MS + (x % mym[g]) + RM * (x / mym[g])] = part[(size_t)g * MS + (x % mym[g]) + RM * (x / mym[g])];
        __syncthreads();
        for (int q = 1; q < ng; q *= 2) {
            for (int me = 0; me + q < ng; me += 2 * q) {
                const int her = me + q;
                const double *Aa = qsh + (size_t)wh[me] * REG + (size_t)me * MS, *Bb = qsh + (size_t)wh[her] * REG + (size_t)her * MS;
                double *dst = qsh + (size_t)(wh[me] ^ 1) * REG + (size_t)me * MS;
                const int mm = mym[me], kk = myn[me], nn = myn[her];
                for (int x = tid; x < mm * nn; x += blockDim.x) {
                    int i = x % mm, j = x / mm;
                    double c = 0.0;
                    for (int l = 0; l < kk; l++) c = c + Bb[l + RM * j] * Aa[i + RM * l];     // dgemm 'n','n', :1381
                    dst[i + RM * j] = c;
                }
            }
            __syncthreads();
            if (tid == 0) for (int me = 0; me + q < ng; me += 2 * q) { myn[me] = myn[me + q]; wh[me] ^= 1; }
            __syncthreads();
        }
        if (tid == 0) { const double v = qsh[(size_t)wh[0] * REG]; for (int g = 0; g < P.G; g++) P.gs[g].val = v; }
        return;
    }
    for (int g = 0; g < ng; g++)
        for (int x = tid; x < mym[g] * myn[g]; x += blockDim.x) work[(size_t)g * RM * RM + (x % mym[g]) + RM * (x / mym[g])] = part[(size_t)g * RM * RM + (x % mym[g]) + RM * (x / mym[g])];
    __syncthreads();
    double *tmp = work + (size_t)ng * RM * RM;
    for (int q = 1; q < ng; q *= 2) {
        for (int me = 0; me + q < ng; me += 2 * q) {
            const int her = me + q;
            const double *Aa = work + (size_t)me * RM * RM, *Bb = work + (size_t)her * RM * RM;
            const int mm = mym[me], kk = myn[me], nn = myn[her];
            for (int x = tid; x < mm * nn; x += blockDim.x) {
                int i = x % mm, j = x / mm;
                double c = 0.0;
                for (int l = 0; l < kk; l++) c = c + Bb[l + RM * j] * Aa[i + RM * l];     // dgemm 'n','n', :1381
                tmp[i + RM * j] = c;
            }
            __syncthreads();
            double *dst = work + (size_t)me * RM * RM;
            for (int x = tid; x < mm * nn; x += blockDim.x) dst[(x % mm) + RM * (x / mm)] = tmp[(x % mm) + RM * (x / mm)];
            __syncthreads();
            if (tid == 0) myn[me] = nn;
            __syncthreads();
        }
    }
    if (tid == 0) for (int g = 0; g < P.G; g++) P.gs[g].val = work[0];
}
