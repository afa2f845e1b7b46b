// ttx_eval.h -- the resident tensor train at a BATCH of multi-indices (ttx_ijk_batch / ttx_ijk_batch_dev / ttx_value_batch).
//
// dtt_ijk (lib/tt.f90:630-652) is a chain of d mat-vecs: x = U_d(:, i_d, 1); for i = d-1 .. 1: x = U_i(:, i_i, :) x; value x(1).
// Two device paths over the finalised cores (element (a, j, k) of core i at a + RM j + SS k):
//   exact (k_ev_exact): one wave per point, the operation sequence of oracle/ttx_oracle_tt.c:ttxo_tt_ijk and of the chain inside
//          k_accchk -- sums from 0.0 over ascending k, separate multiply and add -- so the values are those of the oracle bit for bit
//   MFMA  (k_ev_init / k_ev_hist / k_ev_scan / k_ev_scatter / k_ev_gemm / k_ev_final): per mode the points are counting-sorted by
//          their index at that mode; all points of one index multiply the same slice U_i(:, j, :), a GEMM on the fp64 matrix cores.
//          A point's value depends on its own column and the fixed k order of v_mfma_f64_16x16x4_f64 only, never on its neighbours.
#pragma once
#include <hip/hip_runtime.h>
#include "ttx_ttops.h"     // the dbl4 vector type only
#include "ttx_op_plan.h"   // TTX_EV_TP, TTX_EV_LDSHIST, ev_lda, ev_gemm_lds: shared with the call's plan

// the train as the evaluation kernels see it: one device block [d core pointers][r(0:d)][n(1:d)], rebuilt per call (ort / svd move ranks)
struct EvTrain {
    int d, RM, ldx;                 // cores, row stride of a slab, doubles per point state (max rank rounded up to 4)
    size_t SS;                      // stride of the third core index
    const double *const *core;      // [d], 0-based mode
    const int *r;                   // [d+1]
    const int *n;                   // [d]
};

// ---- exact: one wave per point, grid-stride --------------------------------------------------------------------------------------
// dynamic LDS per wave: x[ldx], z[ldx], the point's index row [d]; nothing is shared between waves, so no workgroup barrier.
// flag (may be null): points whose flag is set get 0.0 (dtt_value of a negative coordinate) and read no core.
__global__ __launch_bounds__(256) void k_ev_exact(EvTrain T, long long npts, const int *ind, const int *flag, double *out)
{
    extern __shared__ __align__(16) double ev_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, d = T.d;
    const size_t per = 2 * (size_t)T.ldx + (((size_t)d + 1) >> 1);
    double *x = ev_dyn + per * wave, *z = x + T.ldx;
    int *id = (int *)(x + 2 * T.ldx);
    for (long long p = (long long)blockIdx.x * nw + wave; p < npts; p += (long long)gridDim.x * nw) {
        if (flag && flag[p]) { if (lane == 0) out[p] = 0.0; continue; }
        __builtin_amdgcn_wave_barrier();
        bool bad = false;
        for (int i = lane; i < d; i += 64) { const int v = ind[(size_t)p * d + i]; id[i] = v; bad |= (v <= 0 || v > T.n[i]); }
        if (__ballot(bad)) { if (lane == 0) out[p] = -3.0; continue; }          // lib/tt.f90:638
        __builtin_amdgcn_wave_barrier();
        {
            const int q0 = T.r[d - 1];
            const double *A = T.core[d - 1] + (size_t)T.RM * (id[d - 1] - 1);
            for (int t = lane; t < q0; t += 64) x[t] = A[t];
        }
        __builtin_amdgcn_wave_barrier();
        for (int i = d - 2; i >= 0; i--) {
            const int q0 = T.r[i], q1 = T.r[i + 1];
            const double *A = T.core[i] + (size_t)T.RM * (id[i] - 1);
            const size_t SS = T.SS;
            if (q0 <= 64) {
                if (lane < q0) {
                    double s = 0.0;
#pragma unroll 8
                    for (int k = 0; k < q1; k++) s = s + A[lane + SS * k] * x[k];
                    z[lane] = s;
                }
            } else {                                                            // ranks above 64: two rows per lane
                const bool two = lane + 64 < q0;
                const double *A1 = two ? A + 64 : A;
                double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
                for (int k = 0; k < q1; k++) { const double xk = x[k]; s0 = s0 + A[lane + SS * k] * xk; s1 = s1 + A1[lane + SS * k] * xk; }
                z[lane] = s0;
                if (two) z[lane + 64] = s1;
            }
            __builtin_amdgcn_wave_barrier();
            double *t_ = x; x = z; z = t_;
        }
        if (lane == 0) out[p] = x[0];
    }
}

// ---- dtt_value (lib/tt.f90:702-728): the index digits of npts coordinate vectors, one thread per point ---------------------------
// plain fp64, no contraction (the library is built with -ffp-contract=off); modes left without a digit keep 0 (-> -3.0 of dtt_ijk)
__global__ __launch_bounds__(256) void k_ev_digits(int d, const int *n, int dd, long long npts, const double *xv, int *ind, int *flag)
{
    const int mm = d / dd;
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < npts; p += (long long)gridDim.x * blockDim.x) {
        int *row = ind + (size_t)p * d;
        for (int i = 0; i < d; i++) row[i] = 0;
        int neg = 0;
        for (int id = 0; id < dd && !neg; id++) {
            double xx = xv[(size_t)p * dd + id];
            if (xx < 0.0) { neg = 1; break; }
            if (xx > 1.0) xx = xx - (double)(int)xx;
            for (int j = 1; j <= mm; j++) {
                const int pos = id * mm + mm - j, np = n[pos];
                int i = (int)((double)np * xx);
                if (i == np) i = np - 1;
                row[pos] = i + 1;
                xx = xx * (double)np - (double)i;
            }
        }
        flag[p] = neg;
    }
}

// ---- MFMA path -------------------------------------------------------------------------------------------------------------------
// validity of every point and the start vector x = U_d(:, i_d, 1) in the point's own slot; one wave per point
__global__ __launch_bounds__(256) void k_ev_init(EvTrain T, int npts, const int *ind, const int *flag, int *valid, double *X, double *out)
{
    const int lane = threadIdx.x & 63, d = T.d;
    for (int p = blockIdx.x * 4 + (threadIdx.x >> 6); p < npts; p += gridDim.x * 4) {
        if (flag && flag[p]) { if (lane == 0) { out[p] = 0.0; valid[p] = 0; } continue; }
        bool bad = false;
        for (int i = lane; i < d; i += 64) { const int v = ind[(size_t)p * d + i]; bad |= (v <= 0 || v > T.n[i]); }
        if (__ballot(bad)) { if (lane == 0) { out[p] = -3.0; valid[p] = 0; } continue; }
        if (lane == 0) valid[p] = 1;
        const int q0 = T.r[d - 1];
        const double *A = T.core[d - 1] + (size_t)T.RM * (ind[(size_t)p * d + d - 1] - 1);
        for (int t = lane; t < q0; t += 64) X[(size_t)p * T.ldx + t] = A[t];
    }
}
// counting sort of the valid points by their index at mode i, step 1: cnt[j] = points with index j+1 (cnt zeroed by the caller)
__global__ __launch_bounds__(256) void k_ev_hist(int d, int i, int nmode, int npts, const int *ind, const int *valid, int *cnt)
{
    extern __shared__ int ev_h[];
    const bool lds = nmode <= TTX_EV_LDSHIST;
    const int per = (npts + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = min(npts, lo + per);
    if (lds) { for (int j = threadIdx.x; j < nmode; j += blockDim.x) ev_h[j] = 0; __syncthreads(); }
    for (int p = lo + threadIdx.x; p < hi; p += blockDim.x)
        if (valid[p]) atomicAdd(lds ? &ev_h[ind[(size_t)p * d + i] - 1] : &cnt[ind[(size_t)p * d + i] - 1], 1);
    if (lds) { __syncthreads(); for (int j = threadIdx.x; j < nmode; j += blockDim.x) if (ev_h[j]) atomicAdd(&cnt[j], ev_h[j]); }
}
// step 2 (one workgroup): off[j] = first position of bucket j, off[nmode] = valid points; tile[j] = first work item of bucket j,
// tile[nmode] = work items; cur[j] = off[j] (the scatter's cursors)
__global__ __launch_bounds__(1024) void k_ev_scan(int nmode, const int *cnt, int *off, int *tile, int *cur)
{
    __shared__ int sa[1024], sb[1024];
    const int tid = threadIdx.x, per = (nmode + 1023) / 1024, lo = tid * per, hi = min(nmode, lo + per);
    int a = 0, b = 0;
    for (int j = lo; j < hi; j++) { a += cnt[j]; b += (cnt[j] + TTX_EV_TP - 1) / TTX_EV_TP; }
    sa[tid] = a; sb[tid] = b;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) {
        const int va = tid >= s ? sa[tid - s] : 0, vb = tid >= s ? sb[tid - s] : 0;
        __syncthreads();
        sa[tid] += va; sb[tid] += vb;
        __syncthreads();
    }
    a = sa[tid] - a; b = sb[tid] - b;
    for (int j = lo; j < hi; j++) { off[j] = a; cur[j] = a; tile[j] = b; a += cnt[j]; b += (cnt[j] + TTX_EV_TP - 1) / TTX_EV_TP; }
    if (tid == 1023) { off[nmode] = sa[1023]; tile[nmode] = sb[1023]; }
}
// step 3: perm[position] = point.  The order inside a bucket is whatever the atomics give: no value depends on it.
__global__ __launch_bounds__(256) void k_ev_scatter(int d, int i, int nmode, int npts, const int *ind, const int *valid, int *cur, int *perm)
{
    extern __shared__ int ev_h[];                                               // [nmode] local counts, then the block's base per bucket
    const bool lds = nmode <= TTX_EV_LDSHIST;
    const int per = (npts + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * per, hi = min(npts, lo + per);
    if (!lds) {
        for (int p = lo + threadIdx.x; p < hi; p += blockDim.x) if (valid[p]) perm[atomicAdd(&cur[ind[(size_t)p * d + i] - 1], 1)] = p;
        return;
    }
    for (int j = threadIdx.x; j < nmode; j += blockDim.x) ev_h[j] = 0;
    __syncthreads();
    for (int p = lo + threadIdx.x; p < hi; p += blockDim.x) if (valid[p]) atomicAdd(&ev_h[ind[(size_t)p * d + i] - 1], 1);
    __syncthreads();
    for (int j = threadIdx.x; j < nmode; j += blockDim.x) { const int c = ev_h[j]; ev_h[j] = c ? atomicAdd(&cur[j], c) : 0; }
    __syncthreads();
    for (int p = lo + threadIdx.x; p < hi; p += blockDim.x) if (valid[p]) perm[atomicAdd(&ev_h[ind[(size_t)p * d + i] - 1], 1)] = p;
}
// Z[:, pts] = U_i(:, j, :) X[:, pts] for one work item = (index j, up to TTX_EV_TP points of bucket j).  The slice is staged in
// LDS once (zero-padded to 16 rows x 4 columns); each wave takes column tiles of 16 points, gathers their states through perm
// (B[k l>>4][col l&15]) and keeps all q0/16 row tiles of the result in registers (MR = row tiles, q0 <= 16 MR).
template <int MR>
__global__ __launch_bounds__(256) void k_ev_gemm(EvTrain T, int i, int nmode, const int *off, const int *tile, const int *perm, const double *X, double *Z)
{
    extern __shared__ __align__(16) double ev_dyn[];
    const int nt = tile[nmode];
    if ((int)blockIdx.x >= nt) return;
    int lo = 0, hi = nmode - 1;                                                 // the bucket of this work item: last j with tile[j] <= blockIdx.x
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (tile[mid] <= (int)blockIdx.x) lo = mid; else hi = mid - 1; }
    const int j = lo, q0 = T.r[i], q1 = T.r[i + 1], lda = ev_lda(q0), kp = (q1 + 3) & ~3, rp = (q0 + 15) & ~15;
    const int first = off[j] + ((int)blockIdx.x - tile[j]) * TTX_EV_TP, last = min(off[j + 1], first + TTX_EV_TP);
    const double *A = T.core[i] + (size_t)T.RM * j;
    for (int e = threadIdx.x; e < rp * kp; e += 256) {
        const int a = e % rp, k = e / rp;
        ev_dyn[a + lda * k] = (a < q0 && k < q1) ? A[a + T.SS * k] : 0.0;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, col = l & 15, kq = l >> 4;
    for (int c0 = first + 16 * wave; c0 < last; c0 += 64) {
        const int c = c0 + col, pt = c < last ? perm[c] : -1;
        const double *xp = X + (size_t)(pt < 0 ? 0 : pt) * T.ldx;
        dbl4 acc[MR];
#pragma unroll
        for (int m = 0; m < MR; m++) acc[m] = dbl4{0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < kp; k0 += 4) {
            const int k = k0 + kq;
            const double b = (pt >= 0 && k < q1) ? xp[k] : 0.0;
#pragma unroll
            for (int m = 0; m < MR; m++)
                if (16 * m < rp) acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(ev_dyn[16 * m + col + lda * k], b, acc[m], 0, 0, 0);
        }
        if (pt >= 0) {
            double *zp = Z + (size_t)pt * T.ldx;
#pragma unroll
            for (int m = 0; m < MR; m++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) { const int row = 16 * m + kq + 4 * reg; if (row < q0) zp[row] = acc[m][reg]; }
        }
    }
}
__global__ __launch_bounds__(256) void k_ev_final(int npts, int ldx, const int *valid, const double *X, double *out)
{
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < npts; p += gridDim.x * blockDim.x) if (valid[p]) out[p] = X[(size_t)p * ldx];
}
