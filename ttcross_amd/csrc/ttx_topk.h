// ttx_topk.h -- the largest elements of the resident tensor train by a beam search along the train (ttx_topk).
//
// The definition is in include/ttx.h.  Modes are searched from the last to the first, so the running state of a candidate is
// dtt_ijk's own chain (k_ev_exact, ttx_eval.h) and the value of the train at a returned index falls out of the search.  Per call:
//   k_tk_gram_w, k_tk_gram_p   the prefix Gram matrices P_1 .. P_(d-1), two launches per step: W = P_(k-1) G_k(:, i, :) per index,
//                              then P_k = sum_i G_k(:, i, :)^T W(:, i, :), ascending i and a in every element
// and per mode k = d .. 1, on the sheet of |C_(k+1)| x |I_k| pairs (flat position c |I_k| + i):
//   k_tk_score_mfma / _exact   s(c, i) = sqrt(max(0, y^T P_(k-1) y)), y = G_k(:, i, :) x_c, written as an ordered 64-bit key
//   k_tk_selinit, k_tk_hist, k_tk_pick   radix select of the K-th largest key, 11 bits per pass from the top (integer atomics only)
//   k_tk_count, k_tk_blkscan, k_tk_scatter   the kept positions in ascending flat position, the largest key not kept, the NaN flag
//   k_tk_advance               one wave per kept pair: x = G_k(:, i, :) x_parent by sm_chain_step (the bits of TTX_EVAL_EXACT)
// and at the end k_tk_back (index rows by back-tracking the kept positions) and k_tk_order (the ordering by `which`).
// Keys: a score is >= +0.0 or NaN; key = its bit pattern + 1, NaN = 0, so that keys order as the definition orders scores (NaN
// below every number, +Inf first) and a selection never looks at a floating-point value.  Every index is formed from positions
// and counts; a stored position is range-checked again where it is read.  No floating-point atomics and no sum whose order
// depends on the grid: a call repeats bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "ttx_eval.h"      // EvTrain
#include "ttx_sample.h"    // sm_chain_step
#include "ttx_ttops.h"     // dbl4

// the sizes TTX_TK_*, the selection's state words TKS_*, tk_u64 and tk_ldy are in ttx_op_plan.h (through ttx_eval.h), shared with the call's plan

__device__ inline tk_u64 tk_key(double s2)
{
    if (s2 != s2) return 0ull;
    const double s = s2 > 0.0 ? sqrt(s2) : 0.0;
    return (tk_u64)__double_as_longlong(s) + 1ull;
}
__device__ inline tk_u64 tk_key_abs(double y) { return y != y ? 0ull : (tk_u64)__double_as_longlong(fabs(y)) + 1ull; }

// ---- Gram chain -----------------------------------------------------------------------------------------------------------------
// W(a, ii, b) = sum_a' P(a, a') G(a', i, b), ascending a' from 0.0; one workgroup per (ii, b), threads along a.  W is compact:
// a + r0 (ii + nI b).  ifix >= 0: the mode is held at that index (nI = 1)
__global__ __launch_bounds__(128) void k_tk_gram_w(const double *G, int RM, size_t SS, int r0, int nI, int ifix, const double *P, int ldp, double *W)
{
    const int ii = blockIdx.x % nI, b = blockIdx.x / nI, i = ifix >= 0 ? ifix : ii, a = threadIdx.x;
    if (a >= r0) return;
    const double *g = G + (size_t)RM * i + SS * b;
    double s = 0.0;
#pragma unroll 4
    for (int q = 0; q < r0; q++) s = s + P[a + (size_t)ldp * q] * g[q];
    W[a + (size_t)r0 * (ii + (size_t)nI * b)] = s;
}
// Pn(b, b') = sum_ii sum_a G(a, i, b) W(a, ii, b'), ascending ii, then ascending a, from 0.0; a workgroup owns 16 x 16 elements and
// walks the sum in LDS tiles of 16 a
__global__ __launch_bounds__(256) void k_tk_gram_p(const double *G, int RM, size_t SS, int r0, int r1, int nI, int ifix, const double *W, double *Pn, int ldp)
{
    __shared__ double gs[16][17], ws[16][17];
    const int t = threadIdx.x, lo = t & 15, hi = t >> 4, b0 = 16 * blockIdx.x, c0 = 16 * blockIdx.y;
    double s = 0.0;
    for (int ii = 0; ii < nI; ii++) {
        const int i = ifix >= 0 ? ifix : ii;
        for (int a0 = 0; a0 < r0; a0 += 16) {
            const int a = a0 + lo;
            __syncthreads();
            gs[hi][lo] = (a < r0 && b0 + hi < r1) ? G[a + (size_t)RM * i + SS * (b0 + hi)] : 0.0;
            ws[hi][lo] = (a < r0 && c0 + hi < r1) ? W[a + (size_t)r0 * (ii + (size_t)nI * (c0 + hi))] : 0.0;
            __syncthreads();
            const int na = min(16, r0 - a0);
            for (int q = 0; q < na; q++) s = s + gs[lo][q] * ws[hi][q];
        }
    }
    if (b0 + lo < r1 && c0 + hi < r1) Pn[(b0 + lo) + (size_t)ldp * (c0 + hi)] = s;
}

// ---- scoring --------------------------------------------------------------------------------------------------------------------
// MFMA: a workgroup owns the indices ii0 .. ii0 + niper - 1 and 64 candidates, 16 per wave; nothing is shared between the waves, so
// there is no workgroup barrier.  Per index a wave forms Y = G_k(:, i, :) X (r0 x 16) on v_mfma_f64_16x16x4_f64, leaves it in its
// LDS tile (column c at c ldy, rows beyond r0 written as 0.0), forms Z = P Y with Y as the B operand from LDS, and adds Y . Z over
// its own rows; the four row groups of a column meet in two shuffles.  Lane maps as k_ev_gemm's: A[row l & 15][k l >> 4],
// B[k l >> 4][col l & 15], result row (l >> 4) + 4 reg, column l & 15.  Rows >= r0, steps >= r1 and candidates >= C are zero-filled
// operands; their results are never read.  first (mode 1, r0 = 1, P_0 = [1]): the score is |y|.
template <int MR>
__global__ __launch_bounds__(256) void k_tk_score_mfma(const double *G, int RM, size_t SS, int r0, int r1, const double *P, int ldp, const double *X, int ldx,
                                                       int C, int nI, int ifix, int niper, int first, tk_u64 *S)
{
    extern __shared__ __align__(16) double tk_dyn[];
    const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, col = l & 15, kq = l >> 4;
    const int c0 = 64 * blockIdx.y + 16 * wave;
    if (c0 >= C) return;
    const int ldy = tk_ldy(r0), rp = (r0 + 15) & ~15, kp1 = (r1 + 3) & ~3, kp0 = (r0 + 3) & ~3;
    const int c = c0 + col;
    const bool cok = c < C;
    const double *xp = X + (size_t)(cok ? c : 0) * ldx;
    double *Yw = tk_dyn + (size_t)wave * 16 * ldy, *yc = Yw + col * ldy;
    const int ii1 = min(nI, (int)(blockIdx.x + 1) * niper);
    for (int ii = blockIdx.x * niper; ii < ii1; ii++) {
        const double *Gi = G + (size_t)RM * (ifix >= 0 ? ifix : ii);
        dbl4 acc[MR];
#pragma unroll
        for (int m = 0; m < MR; m++) acc[m] = dbl4{0.0, 0.0, 0.0, 0.0};
        for (int k0 = 0; k0 < kp1; k0 += 4) {
            const int b = k0 + kq;
            const double bv = (cok && b < r1) ? xp[b] : 0.0;
#pragma unroll
            for (int m = 0; m < MR; m++)
                if (16 * m < rp) {
                    const int a = 16 * m + col;
                    const double av = (a < r0 && b < r1) ? Gi[a + SS * b] : 0.0;
                    acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[m], 0, 0, 0);
                }
        }
        __builtin_amdgcn_wave_barrier();                                        // the previous index's reads of the tile are done
#pragma unroll
        for (int m = 0; m < MR; m++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) { const int row = 16 * m + kq + 4 * reg; if (16 * m < rp) yc[row] = row < r0 ? acc[m][reg] : 0.0; }
        __builtin_amdgcn_wave_barrier();
        tk_u64 key;
        if (first) key = tk_key_abs(yc[0]);
        else {
#pragma unroll
            for (int m = 0; m < MR; m++) acc[m] = dbl4{0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < kp0; k0 += 4) {
                const int a = k0 + kq;
                const double yv = yc[a];
#pragma unroll
                for (int m = 0; m < MR; m++)
                    if (16 * m < rp) {
                        const int ar = 16 * m + col;
                        const double pv = (ar < r0 && a < r0) ? P[ar + (size_t)ldp * a] : 0.0;
                        acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(pv, yv, acc[m], 0, 0, 0);
                    }
            }
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < MR; m++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) { const int row = 16 * m + kq + 4 * reg; if (row < r0) s = s + yc[row] * acc[m][reg]; }
            s = s + __shfl_xor(s, 16);
            s = s + __shfl_xor(s, 32);
            key = tk_key(s);
        }
        if (kq == 0 && cok) S[(size_t)c * nI + ii] = key;
    }
}

// EXACT: one wave per pair, grid-stride; y by sm_chain_step (the chain's own order), z(a) = sum_a' P(a, a') y(a') over ascending a'
// from 0.0, y(a) z(a) added per lane over its rows a = lane, lane + 64, then across the lanes in six xor steps 32 .. 1.
// Dynamic LDS per wave: y[ldx].
__global__ __launch_bounds__(256) void k_tk_score_exact(const double *G, int RM, size_t SS, int r0, int r1, const double *P, int ldp, const double *X, int ldx,
                                                        int C, int nI, int ifix, int first, tk_u64 *S)
{
    extern __shared__ __align__(16) double tk_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    double *y = tk_dyn + (size_t)wave * ldx;
    const long long M = (long long)C * nI;
    for (long long pr = (long long)blockIdx.x * nw + wave; pr < M; pr += (long long)gridDim.x * nw) {
        const int c = (int)(pr / nI), ii = (int)(pr % nI);
        __builtin_amdgcn_wave_barrier();
        sm_chain_step(G + (size_t)RM * (ifix >= 0 ? ifix : ii), SS, r0, r1, X + (size_t)c * ldx, y, lane);
        __builtin_amdgcn_wave_barrier();
        tk_u64 key;
        if (first) key = tk_key_abs(y[0]);
        else {
            double part = 0.0;
            for (int a = lane; a < r0; a += 64) {
                double z = 0.0;
#pragma unroll 4
                for (int q = 0; q < r0; q++) z = z + P[a + (size_t)ldp * q] * y[q];
                part = part + y[a] * z;
            }
            part = wave_sum_xor(part);
            key = tk_key(part);
        }
        if (lane == 0) S[pr] = key;
    }
}

// ---- selection ------------------------------------------------------------------------------------------------------------------
// a mode's selection state; all = 1: everything is kept (T = 0, need = M).  The bound and the NaN flag live across the modes.
__global__ __launch_bounds__(1024) void k_tk_selinit(tk_u64 *st, unsigned *hist, long long K, long long M, int all, int reset)
{
    for (int j = threadIdx.x; j < TTX_TK_BINS; j += 1024) hist[j] = 0u;
    if (threadIdx.x == 0) {
        st[TKS_PREFIX] = 0ull; st[TKS_KREM] = (tk_u64)K;
        st[TKS_T] = 0ull; st[TKS_NEED] = all ? (tk_u64)M : 0ull;
        if (reset) { st[TKS_BOUND] = 0ull; st[TKS_NAN] = 0ull; }
    }
}
// keys whose bits above shift + nbits equal the prefix's, counted by their digit (top: no bits above, every key counts)
__global__ __launch_bounds__(256) void k_tk_hist(const tk_u64 *S, long long M, int shift, int nbits, int top, const tk_u64 *st, unsigned *hist)
{
    __shared__ unsigned h[TTX_TK_BINS];
    const tk_u64 prefix = st[TKS_PREFIX];
    const int up = shift + nbits;
    const unsigned mask = (1u << nbits) - 1u;
    for (int j = threadIdx.x; j < TTX_TK_BINS; j += 256) h[j] = 0u;
    __syncthreads();
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < M; p += (long long)gridDim.x * 256) {
        const tk_u64 key = S[p];
        if (top || (key >> up) == (prefix >> up)) atomicAdd(&h[(unsigned)(key >> shift) & mask], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < TTX_TK_BINS; j += 256) if (h[j]) atomicAdd(&hist[j], h[j]);
}
// the digit at which the count from the top reaches the keys still wanted; one workgroup.  Thread t owns the bins 2047 - 2t and
// 2046 - 2t.  After the last pass (shift = 0) T is the K-th largest key and need the number of keys equal to T that are kept.
__global__ __launch_bounds__(1024) void k_tk_pick(tk_u64 *st, unsigned *hist, int shift)
{
    __shared__ unsigned sc[1024];
    const int t = threadIdx.x, b1 = TTX_TK_BINS - 1 - 2 * t, b2 = b1 - 1;
    const unsigned h1 = hist[b1], h2 = hist[b2];
    const tk_u64 krem = st[TKS_KREM], prefix = st[TKS_PREFIX];
    sc[t] = h1 + h2;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) {
        const unsigned v = t >= s ? sc[t - s] : 0u;
        __syncthreads();
        sc[t] += v;
        __syncthreads();
    }
    const tk_u64 incl = sc[t], excl = incl - (h1 + h2);
    hist[b1] = 0u; hist[b2] = 0u;
    if (excl < krem && krem <= incl) {
        const bool in1 = excl + h1 >= krem;
        const tk_u64 np = prefix | ((tk_u64)(in1 ? b1 : b2) << shift), nk = krem - excl - (in1 ? 0u : h1);
        st[TKS_PREFIX] = np; st[TKS_KREM] = nk;
        if (shift == 0) { st[TKS_T] = np; st[TKS_NEED] = nk; }
    }
}
// per chunk of TTX_TK_CHUNK positions: keys above T (high word) and equal to T (low word)
__global__ __launch_bounds__(1024) void k_tk_count(const tk_u64 *S, long long M, const tk_u64 *st, tk_u64 *blk)
{
    __shared__ tk_u64 part[1024];
    const tk_u64 T = st[TKS_T];
    const long long p0 = (long long)blockIdx.x * TTX_TK_CHUNK + 4 * threadIdx.x;
    tk_u64 s = 0ull;
    for (int j = 0; j < 4; j++) if (p0 + j < M) { const tk_u64 key = S[p0 + j]; s += key > T ? (1ull << 32) : (key == T ? 1ull : 0ull); }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 512; o; o >>= 1) { if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) blk[blockIdx.x] = part[0];
}
// exclusive sums of the chunk counts in place; one workgroup, up to 4096 chunks
__global__ __launch_bounds__(1024) void k_tk_blkscan(tk_u64 *blk, int nblk)
{
    __shared__ tk_u64 sc[1024];
    const int t = threadIdx.x;
    tk_u64 v[4], s = 0ull;
    for (int j = 0; j < 4; j++) { v[j] = 4 * t + j < nblk ? blk[4 * t + j] : 0ull; s += v[j]; }
    sc[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const tk_u64 w = t >= o ? sc[t - o] : 0ull;
        __syncthreads();
        sc[t] += w;
        __syncthreads();
    }
    tk_u64 run = sc[t] - s;
    for (int j = 0; j < 4; j++) if (4 * t + j < nblk) { blk[4 * t + j] = run; run += v[j]; }
}
// the kept positions in ascending order: a key above T at slot (keys above T before it) + min(keys equal to T before it, need); a
// key equal to T is kept while fewer than need came before it.  The largest key not kept goes into the call's bound, a NaN key
// anywhere on the sheet sets the flag (integer atomics).  cap: slots of rec.
__global__ __launch_bounds__(1024) void k_tk_scatter(const tk_u64 *S, long long M, tk_u64 *st, const tk_u64 *blk, int *rec, int cap)
{
    __shared__ tk_u64 sc[1024];
    __shared__ tk_u64 mx[1024];
    const int t = threadIdx.x;
    const tk_u64 T = st[TKS_T], need = st[TKS_NEED];
    const long long p0 = (long long)blockIdx.x * TTX_TK_CHUNK + 4 * t;
    tk_u64 key[4], s = 0ull;
    for (int j = 0; j < 4; j++) {
        key[j] = p0 + j < M ? S[p0 + j] : 0ull;
        if (p0 + j < M) s += key[j] > T ? (1ull << 32) : (key[j] == T ? 1ull : 0ull);
    }
    sc[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const tk_u64 w = t >= o ? sc[t - o] : 0ull;
        __syncthreads();
        sc[t] += w;
        __syncthreads();
    }
    const tk_u64 run = blk[blockIdx.x] + sc[t] - s;
    tk_u64 g = run >> 32, e = run & 0xffffffffull, best = 0ull;
    int nan = 0;
    for (int j = 0; j < 4; j++) {
        if (p0 + j >= M) break;
        long long slot = -1;
        if (key[j] > T) { slot = (long long)(g + (e < need ? e : need)); g++; }
        else if (key[j] == T) { if (e < need) slot = (long long)(g + e); e++; }
        if (key[j] == 0ull) nan = 1;
        if (slot >= 0) { if (slot < cap) rec[slot] = (int)(p0 + j); }
        else if (key[j] > best) best = key[j];
    }
    mx[t] = best | ((tk_u64)nan << 63);                                         // a key is below 2^63: bit 63 carries the flag
    __syncthreads();
    for (int o = 512; o; o >>= 1) {
        if (t < o) { const tk_u64 a = mx[t], b = mx[t + o], ka = a & ~(1ull << 63), kb = b & ~(1ull << 63); mx[t] = (ka > kb ? ka : kb) | ((a | b) & (1ull << 63)); }
        __syncthreads();
    }
    if (t == 0) {
        const tk_u64 k = mx[0] & ~(1ull << 63);
        if (k) atomicMax(&st[TKS_BOUND], k);
        if (mx[0] >> 63) atomicMax(&st[TKS_NAN], 1ull);
    }
}

// ---- advance, back-tracking, ordering --------------------------------------------------------------------------------------------
// one wave per kept pair: its state from the parent's by the chain step of k_ev_exact; at the last mode a copy of G_d(:, i, 1).
// Dynamic LDS per wave: the parent's x [ldx]
__global__ __launch_bounds__(256) void k_tk_advance(const double *G, int RM, size_t SS, int r0, int r1, int last, const int *rec, int Cn, long long M, int nI, int ifix,
                                                    const double *Xo, double *Xn, int ldx)
{
    extern __shared__ __align__(16) double tk_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    double *x = tk_dyn + (size_t)wave * ldx;
    for (int j = blockIdx.x * nw + wave; j < Cn; j += gridDim.x * nw) {
        int p = rec[j];
        if (p < 0 || p >= M) p = 0;
        const int c = p / nI, i = ifix >= 0 ? ifix : p % nI;
        const double *A = G + (size_t)RM * i;
        double *z = Xn + (size_t)j * ldx;
        if (last) { for (int a = lane; a < r0; a += 64) z[a] = A[a]; continue; }
        __builtin_amdgcn_wave_barrier();
        for (int b = lane; b < r1; b += 64) x[b] = Xo[(size_t)c * ldx + b];
        __builtin_amdgcn_wave_barrier();
        sm_chain_step(A, SS, r0, r1, x, z, lane);
    }
}
// row j of the survivors: its indices by walking the kept positions from mode 1 to mode d, and its value x_1(1).
// nI, ifx, cnt: per mode (0-based) the searched indices, the fixed index or -1, and the pairs kept there
__global__ __launch_bounds__(256) void k_tk_back(int d, int K, int nf, const int *rec, const int *nI, const int *ifx, const int *cnt, const long long *sheet,
                                                 const double *X, int ldx, int *tind, double *tval)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nf) return;
    int slot = j;
    for (int k = 0; k < d; k++) {
        if (slot < 0 || slot >= cnt[k]) slot = 0;
        int p = rec[(size_t)k * K + slot];
        if (p < 0 || p >= sheet[k]) p = 0;
        tind[(size_t)j * d + k] = (ifx[k] >= 0 ? ifx[k] : p % nI[k]) + 1;
        slot = p / nI[k];
    }
    tval[j] = X[(size_t)j * ldx];
}
// row j' comes before row j: by `which` (0 |v|, 1 v, both descending; 2 v ascending), a NaN after every number, ties and NaNs among
// themselves by the lexicographically smaller index row
__device__ inline bool tk_before(int which, double va, double vb, const int *ra, const int *rb, int d)
{
    const double a = which == 0 ? fabs(va) : (which == 2 ? -va : va), b = which == 0 ? fabs(vb) : (which == 2 ? -vb : vb);
    const bool na = a != a, nb = b != b;
    if (na != nb) return nb;
    if (!na && a != b) return a > b;
    for (int k = 0; k < d; k++) if (ra[k] != rb[k]) return ra[k] < rb[k];
    return false;
}
// the place of row j is the number of rows before it: a permutation, since the rows differ; oind and oval were zeroed
__global__ __launch_bounds__(256) void k_tk_order(int d, int nf, int which, const int *tind, const double *tval, int *oind, double *oval)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= nf) return;
    const double v = tval[j];
    const int *row = tind + (size_t)j * d;
    int place = 0;
    for (int q = 0; q < nf; q++) place += (q != j && tk_before(which, tval[q], v, tind + (size_t)q * d, row, d)) ? 1 : 0;
    if (place >= nf) place = nf - 1;
    for (int k = 0; k < d; k++) oind[(size_t)place * d + k] = row[k];
    oval[place] = v;
}
