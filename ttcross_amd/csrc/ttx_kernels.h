// ttx_kernels.h -- CDNA4 (gfx950) kernels of one bond step of the dtt_dmrgg sweep on the multi-kernel path: the step states, full
// pivoting, the Ising D/E tables, k_lottery, k_halfstep, k_accept; and dtt_accchk.
// Compiled with -ffp-contract=off: every product and sum below is an individual IEEE fp64 rounding, in the
// order of the netlib reference BLAS the oracle restates, so pivot paths are reproducible bit for bit.
#pragma once
#include "ttx_addr.h"
#include "ttx_bondstep.h" // the rules of a bond step shared by every sweep kernel
#include "ttx_integrands.h"
#include "ttx_wave.h"

// resolve pending partial arg-max records of the previous half-step into the step state
// (lib/dmrgg.f90:540-546 and :573-579)
__device__ inline void resolve_state(StepState &c, const Partial *pt)
{
    if (!c.active || !c.pending) return;
    const int nb = c.npart;                      // records the half-step kernel wrote (its number of fiber workgroups)
    double ba = -1.0, bv = 0.0; int bi = INT_MAX;
    for (int b = 0; b < nb; b++) {
        double a = pt[b].absmax; int ix = pt[b].idx;
        if (a > ba || (a == ba && ix < bi)) { ba = a; bv = pt[b].val; bi = ix; }
    }
    c.done = take_pivot(c.pending == 1, bi, c.r0, c.n2, c.havecol, c.haverow, c.ii, c.jj, c.kk, c.qq);
    c.pivot = bv;
    c.pending = 0;
}

// the same by the first WAVE of a workgroup (all 64 lanes call it; lane 0 writes c): the partial records are loaded by the lanes
// side by side and folded on the DPP path instead of one thread walking them (2 us of every half-step at 26 records)
__device__ inline void resolve_state_wave(StepState &c, const StepState &src, const Partial *pt, int lane)
{
    double ba = -1.0, bv = 0.0; int bi = INT_MAX;
    const bool pend = src.active && src.pending;
    if (pend)
        for (int b = lane; b < src.npart; b += 64) {
            const double a = pt[b].absmax; const int ix = pt[b].idx;
            if (a > ba || (a == ba && ix < bi)) { ba = a; bv = pt[b].val; bi = ix; }
        }
    wave_argmax(ba, bv, bi);
    if (lane != 0) return;
    c = src;
    if (!pend) return;
    c.done = take_pivot(c.pending == 1, bi, c.r0, c.n2, c.havecol, c.haverow, c.ii, c.jj, c.kk, c.qq);
    c.pivot = bv;
    c.pending = 0;
}

// snapshot of the bond this group works on at step pp of the sweep (:325-335); thread 0 only
__device__ inline void bond_state(const DevProb &P, int g, int dir, int pp, StepState &st)
{
    GroupState &gs = P.gs[g];
    const int m = P.d;
    int *r = P.r + (size_t)g * (m + 2);
    if (pp == 1) sweep_start(P, g);
    int nb = gs.last - gs.first + 1;
    st.active = (pp <= nb);
    st.done = 0; st.havecol = 0; st.haverow = 0; st.crs = 0; st.pending = 0; st.npart = 0; st.pivot = 0.0;
    st.ii = st.jj = st.kk = st.qq = 0;
    if (st.active) {
        int p = (dir == 1) ? gs.first + pp - 1 : gs.last + 1 - pp;   // :330-331
        st.p = p; st.r0 = r[p - 1]; st.r1 = r[p]; st.r2 = r[p + 1]; st.n1 = P.n[p]; st.n2 = P.n[p + 1];
    } else { st.p = 0; st.r0 = st.r1 = st.r2 = st.n1 = st.n2 = 0; st.done = 1; }
}

// full pivoting (piv = -1, :341-408): the bond state, then one column half-step per (k,q) (k_halfstep mode 3),
// then the global first arg-max over the partial records
__global__ void k_bond_begin(DevProb P, int dir, int pp)
{
    if (threadIdx.x != 0) return;
    StepState st;
    bond_state(P, blockIdx.x, dir, pp, st);
    P.gs[blockIdx.x].S[0] = st;
}
__global__ __launch_bounds__(256) void k_full_resolve(DevProb P)
{
    __shared__ double sha[4], shv[4]; __shared__ int shi[4];
    const int g = blockIdx.x, tid = threadIdx.x;
    GroupState &gs = P.gs[g];
    StepState st = gs.S[0];
    if (!st.active) return;
    const int nf = st.r0 * st.n1, nb = (nf + TTX_BLK - 1) / TTX_BLK, ncol = st.n2 * st.r2;
    double ba = -1.0, bv = 0.0; int bi = INT_MAX;
    for (int x = tid; x < ncol * nb; x += blockDim.x) {
        const Partial pr = P.pfull[((size_t)g * P.NM * P.RM + x / nb) * P.nfb + x % nb];
        if (pr.absmax > ba || (pr.absmax == ba && pr.idx < bi)) { ba = pr.absmax; bv = pr.val; bi = pr.idx; }
    }
    block_argmax(ba, bv, bi, sha, shv, shi);
    if (tid == 0) {                                       // :388-396
        int x = (bi == INT_MAX) ? 0 : bi;                  // every residual a NaN: the first position, as idamax
        st.qq = x / (nf * st.n2) + 1; x %= nf * st.n2;
        st.kk = x / nf + 1; x %= nf;
        st.jj = x / st.r0 + 1; st.ii = x % st.r0 + 1;
        st.pivot = bv;
        gs.S[0] = st;
    }
}

// piv = -1 as one dense step (lib/dmrgg.f90:384-396): B = A - col(p) * row(p+1) over the whole superblock by fp64 MFMA
// (v_mfma_f64_16x16x4_f64; operand lane maps as k_gemm_mfma in ttx_ttops.h) fused with the arg-max of |B|.
// A = sb [(i,j) fastest, nf = r0*n1 rows][(k,q), nc = n2*r2 columns]; col(p)[(i + RM j) + SS s]; row(p+1)[(k + NM q) + SW s].
// grid = (ceil(nf/64), ceil(nc/64), groups), 256 threads: wave w owns rows 16w..16w+15 of the 64x64 tile, the row-factor
// tile (K x 64) is staged in LDS once per block.  The MFMA accumulates in its own order, so the residuals differ from the
// reference's dgemm in the last bits: this path is checked by tolerance, the column-by-column path (mode 3) stays the
// bit-exact checker.  One Partial per tile, first-max rule on the superblock's linear index t + nf * column.
typedef double dbl4_ __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_full_gemm_argmax(DevProb P)
{
    __shared__ double Bt[64 * 65];                     // row factor tile: Bt[k * 65 + c], K <= 64
    __shared__ double sha[4], shv[4]; __shared__ int shi[4];
    const int g = blockIdx.z, tid = threadIdx.x, wave = tid >> 6, l = tid & 63;
    const GroupState &gs = P.gs[g];
    const StepState &st = gs.S[0];
    if (!st.active) return;
    const int p = st.p, r0 = st.r0, r1 = st.r1, r2 = st.r2, n1 = st.n1, n2 = st.n2, first = gs.first;
    const int nf = r0 * n1, nc = n2 * r2;
    const int tm = blockIdx.x * 64, tn = blockIdx.y * 64;
    if (tm >= nf || tn >= nc) return;
    const double *Cp = core_ptr(P, P.col, g, p, first), *Wq = core_ptr(P, P.row, g, p + 1, first);
    const double *sb = P.sb + (size_t)g * ((size_t)P.RM * P.NM) * ((size_t)P.RM * P.NM);
    for (int x = tid; x < r1 * 64; x += 256) {
        const int k = x >> 6, c = x & 63, col = tn + c;
        double v = 0.0;
        if (col < nc) { const int kk = col % n2, qq = col / n2; v = Wq[kk + (size_t)P.NM * qq + P.SW * k]; }
        Bt[k * 65 + c] = v;
    }
    __syncthreads();
    const int ar = tm + 16 * wave + (l & 15), kq = l >> 4;
    const bool arok = ar < nf;
    const size_t aoff = arok ? (size_t)(ar % r0) + (size_t)P.RM * (ar / r0) : 0;
    dbl4_ acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; nt++) acc[nt] = dbl4_{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < r1; k0 += 4) {
        const int k = k0 + kq;
        const double a = (arok && k < r1) ? Cp[aoff + P.SS * k] : 0.0;
#pragma unroll
        for (int nt = 0; nt < 4; nt++) {
            const double b = (k < r1) ? Bt[k * 65 + 16 * nt + (l & 15)] : 0.0;
            acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[nt], 0, 0, 0);
        }
    }
    double ab = -1.0, bv = 0.0; int bi = INT_MAX;
#pragma unroll
    for (int nt = 0; nt < 4; nt++)
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const int row = tm + 16 * wave + (l >> 4) + 4 * reg, col = tn + 16 * nt + (l & 15);
            if (row < nf && col < nc) {
                const size_t ix = (size_t)row + (size_t)nf * col;
                const double b = sb[ix] - acc[nt][reg];
                const double a_ = fabs(b);
                if (a_ > ab || (a_ == ab && (int)ix < bi)) { ab = a_; bv = b; bi = (int)ix; }
            }
        }
    block_argmax(ab, bv, bi, sha, shv, shi);
    if (tid == 0) { Partial pr; pr.absmax = ab; pr.val = bv; pr.idx = bi; pr.pad = 0; P.pfull2[(size_t)g * P.fp_tiles + blockIdx.y * gridDim.x + blockIdx.x] = pr; }
}
__global__ __launch_bounds__(256) void k_full_resolve2(DevProb P, int gx, int gy)
{
    __shared__ double sha[4], shv[4]; __shared__ int shi[4];
    const int g = blockIdx.x, tid = threadIdx.x;
    GroupState &gs = P.gs[g];
    StepState st = gs.S[0];
    if (!st.active) return;
    const int nf = st.r0 * st.n1, nc = st.n2 * st.r2;
    const int ux = (nf + 63) / 64, uy = (nc + 63) / 64;          // tiles that hold data
    double ba = -1.0, bv = 0.0; int bi = INT_MAX;
    for (int x = tid; x < ux * uy; x += blockDim.x) {
        const Partial pr = P.pfull2[(size_t)g * P.fp_tiles + (x / ux) * gx + (x % ux)];
        if (pr.absmax > ba || (pr.absmax == ba && pr.idx < bi)) { ba = pr.absmax; bv = pr.val; bi = pr.idx; }
    }
    block_argmax(ba, bv, bi, sha, shv, shi);
    if (tid == 0) {                                       // :388-396
        int x = (bi == INT_MAX) ? 0 : bi;                  // every residual a NaN: the first position, as idamax
        st.qq = x / (nf * st.n2) + 1; x %= nf * st.n2;
        st.kk = x / nf + 1; x %= nf;
        st.jj = x / st.r0 + 1; st.ii = x % st.r0 + 1;
        st.pivot = bv;
        gs.S[0] = st;
    }
}

// Ising D / E: per-bond tables of the pair factors that do not span the bond (see de_pairs_tab).  For every left
// pivot c of bond p-1 (dims 1..A, A = p-1) and every start i: TL[c*NP + off(i) + j-i-1] = ((u-1)/(u+1))^2 with
// u = x_{i+1}*...*x_j accumulated left to right (test_crs_ising.f90:188-192), UL[c*(m+1) + i] = u after j = A; the
// same for every right pivot of bond p+1 over its own dims (TR).  One thread per (start, pivot).  A pivot's factors are
// CONTIGUOUS in the order in which an element through that pivot multiplies them, so that a wave whose elements share
// the pivot (k_halfstep_de) streams them with coalesced 512-byte loads and a lone lane (lottery) walks its own row.
__global__ __launch_bounds__(256) void k_de_tables(DevProb P, int dir, int pp)
{
    const int g = blockIdx.y, m = P.d, RM = P.RM;
    const GroupState &gs = P.gs[g];
    const int first = gs.first, last = gs.last;
    if (pp > last - first + 1) return;
    const int p = (dir == 1) ? first + pp - 1 : last + 1 - pp;
    const int *r = P.r + (size_t)g * (m + 2);
    const int r0 = r[p - 1], r2 = r[p + 1], A = p - 1, B = m - p - 1;
    const double *nodes = P.par - 1;
    const size_t NP = (size_t)P.de_npair, tsz = NP * RM;
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    const int c = x % RM, i = (x / RM) % (m + 1), side = x / (RM * (m + 1));
    if (side == 0) {
        if (c >= r0 || i > A) return;
        const short *Lt = L_ptr(P, g, p - 1, first);
        double *TL = P.deTL + (size_t)g * tsz + (size_t)c * NP, *UL = P.deUL + ((size_t)g * RM + c) * (m + 1);
        const size_t off = (size_t)i * A - (size_t)i * (i - 1) / 2;
        double u = 1.0;
        for (int j = i + 1; j <= A; j++) {
            u = u * nodes[Lt[(size_t)(j - 1) * RM + c]];
            const double t = (u - 1.0) / (u + 1.0);
            TL[off + (j - i - 1)] = t * t;
        }
        UL[i] = u;
    } else if (side == 1) {
        if (c >= r2 || i >= B) return;
        const short *Rt = R_ptr(P, g, p + 1, first);
        double *TR = P.deTR + (size_t)g * tsz + (size_t)c * NP;
        const size_t off = (size_t)i * B - (size_t)i * (i - 1) / 2;
        double u = 1.0;
        for (int j = i + 1; j <= B; j++) {
            u = u * nodes[Rt[(size_t)(j - 1) * RM + c]];
            const double t = (u - 1.0) / (u + 1.0);
            TR[off + (j - i - 1)] = t * t;
        }
    }
}

// Ising D / E with all nodes in [0,1] (P.de_cut): the COMPACT tables.  One workgroup per pivot of the two sets of the bond step
// (left pivots of bond p-1, right pivots of bond p+1).  Row i of a pivot (start at its dim i+1): the factors ((u-1)/(u+1))^2 of
// u = x_{i+1} ... x_j, j = i+1, i+2, ..., while u > 2^-54 -- at u <= 2^-54 the factor is exactly 1 and, u being non-increasing, so is
// every later one of the row.  A pivot's rows are CONTIGUOUS in the order in which an element through that pivot multiplies
// them; CL / CR[i] = entries of row i, [m] = their total; UL[i] = the running product of row i through the pivot's last dim when
// the row gets that far, else 0 (UL[A] = 1: the row that starts behind the pivot); UL[m] = first such row i0 (all later ones get
// that far too), CL[m-1] = entries of the rows before it.  ~12 % of the full triangle at D_256.
// grid = (2 RM, groups), 256 threads, dynamic LDS d doubles.
__global__ __launch_bounds__(256) void k_de_ctables(DevProb P, int dir, int pp)
{
    extern __shared__ __align__(16) double xs[];
    __shared__ int s_w[4], s_carry;
    const int g = blockIdx.y, m = P.d, RM = P.RM, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const GroupState &gs = P.gs[g];
    const int first = gs.first, last = gs.last;
    if (pp > last - first + 1) return;
    const int p = (dir == 1) ? first + pp - 1 : last + 1 - pp;
    const int *r = P.r + (size_t)g * (m + 2);
    const int side = (int)blockIdx.x / RM, c = (int)blockIdx.x % RM;
    if (c >= (side == 0 ? r[p - 1] : r[p + 1])) return;
    const int len = side == 0 ? p - 1 : m - p - 1;
    const short *tab = side == 0 ? L_ptr(P, g, p - 1, first) : R_ptr(P, g, p + 1, first);
    const size_t NP = (size_t)P.de_npair, tsz = NP * RM;
    double *T = (side == 0 ? P.deTL : P.deTR) + (size_t)g * tsz + (size_t)c * NP;
    int *C = (side == 0 ? P.deCL : P.deCR) + ((size_t)g * RM + c) * (m + 1);
    double *UL = P.deUL + ((size_t)g * RM + c) * (m + 1);
    __shared__ int s_i0, s_pre;
    for (int k = tid; k < len; k += 256) xs[k] = P.par[tab[(size_t)k * RM + c] - 1];
    if (tid == 0) { s_carry = 0; s_i0 = len; s_pre = -1; }
    __syncthreads();
    for (int base = 0; base < len; base += 256) {
        const int i = base + tid;
        int cnt = 0; double u = 1.0;
        if (i < len) for (int j = i; j < len; j++) { u = u * xs[j]; if (u <= 0x1p-54) break; cnt++; }
        // exclusive scan of cnt over the workgroup
        // (the scan written out, not wave_scan of ttx_wave.h: through the function this kernel's compares come out in another order)
        int inc = cnt;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int y = __shfl_up(inc, o, 64); if (lane >= o) inc += y; }
        if (lane == 63) s_w[wv] = inc;
        if (i < len && cnt == len - i) atomicMin(&s_i0, i);          // the row gets through the pivot's last dim: it and all later ones span the bond
        __syncthreads();
        int off = s_carry + inc - cnt;
        for (int w = 0; w < wv; w++) off += s_w[w];
        if (i == s_i0 && i < len) s_pre = off;
        if (i < len) {
            C[i] = cnt;
            if (side == 0) UL[i] = (cnt == len - i) ? u : 0.0;
            double uu = 1.0;
            for (int t = 0; t < cnt; t++) { uu = uu * xs[i + t]; T[off + t] = de_t2<true>(uu); }
        }
        __syncthreads();
        if (tid == 0) s_carry += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
    // rows 0 .. i0-1 end inside the pivot's dims: their C[m-1] factors form one run without a bond-spanning tail in between
    if (tid == 0) { C[m] = s_carry; C[m - 1] = (s_pre >= 0) ? s_pre : s_carry; if (side == 0) { UL[len] = 1.0; UL[m] = (double)s_i0; } }
}

// ------------------------------------------------------------------------------------------------
// K_lottery: lottery2 candidates, their values and residuals, start pivot (lib/dmrgg.f90:410-484)
// one block per group
// ------------------------------------------------------------------------------------------------
template <int FUN>
__global__ __launch_bounds__(512) void k_lottery(DevProb P, int dir, int pp, int vals, int phase)
{
    extern __shared__ __align__(16) double dyn[];
    __shared__ StepState st;
    __shared__ int zc[128], zr[128], zcs[128], zrs[128], keepc[128], keepr[128];
    __shared__ int nzc, nzr, nsc, nsr;
    __shared__ ttx_cdfseg segc[TTX_MAXSEG], segr[TTX_MAXSEG];
    __shared__ double sha[8], shv[8]; __shared__ int shi[8];
    __shared__ int s_last;
    const int g = blockIdx.y, tid = threadIdx.x, m = P.d;
    const int nbl = (int)gridDim.x, blk = (int)blockIdx.x;
    GroupState &gs = P.gs[g];
    STAMP_DECL;
    // phase 0: everything in this launch.  Ising D/E (one candidate per wave, ttx_de.h): phase 1 draws the candidates into
    // P.lotc and leaves the state in gs.S[0]; k_lottery_eval_de fills P.lotf; phase 2 takes residuals, arg-max and state.
    if (tid == 0) { if (phase == 2) st = gs.S[0]; else bond_state(P, g, dir, pp, st); }
    __syncthreads();
    if (!st.active) { if (tid == 0 && phase != 2) gs.S[0] = st; return; }
    STAMP(gs, 0);   // 0: state
    const int p = st.p, r0 = st.r0, r1 = st.r1, r2 = st.r2, n1 = st.n1, n2 = st.n2, first = gs.first;
    const int nlot = r0 + n1 + n2 + r2;
    // LDS: par | lot[4*nlot] (int) | LT[r0][VS] | RT[r2][VS] (short): the pivot tables of bonds p-1 and p+1,
    // transposed so that the multi-index of a left / right pivot is one contiguous 16-byte-aligned row
    const int VS = ((m + 7) & ~7) + 8;
    double *par = dyn;
    int *lot = (int *)(dyn + ((P.npar + 1) & ~1));
    short *LT = (short *)(lot + ((4 * nlot + 3) & ~3));
    short *RT = LT + (size_t)r0 * VS;
    const double *Cp = core_ptr(P, P.col, g, p, first), *Wq = core_ptr(P, P.row, g, p + 1, first);
    const short *Lt = L_ptr(P, g, p - 1, first), *Rt = R_ptr(P, g, p + 1, first);
    for (int x = tid; x < P.npar; x += blockDim.x) par[x] = P.par[x];
    // mvn: rows of differences x - mu (doubles) take the place of the index rows (host sized the LDS for them: vals)
    const bool fastp = fast_path(P, FUN);           // TTX_ARITH=fast: candidates from the tables of k_fast_tables (vals = LDS rows per side)
    const bool usem = (FUN == FUN_MVN) && (vals != 0) && !fastp;
    double *DLv = (double *)(((size_t)LT + 15) & ~(size_t)15), *DRv = DLv + (size_t)r0 * VS;
    double *sNL = DLv, *sNR = DLv + (size_t)vals * P.RM;
    __shared__ int s_mc[2];
    int fcap = 0;
    if (phase != 0) {
        // no evaluation in this launch: the pivot rows are not needed
    } else if (fastp) {
        if (FUN == FUN_ISING && vals > 0) {
            // the leading rows of the two decay tables (those above the cut for at least one pivot, at most vals) into LDS
            if (tid < 2) s_mc[tid] = 0;
            __syncthreads();
            for (int x = tid; x < r0; x += blockDim.x) atomicMax(&s_mc[0], (int)fast_piv(P, 0, g, p - 1, first)[FP_N * P.RM + x]);
            for (int x = tid; x < r2; x += blockDim.x) atomicMax(&s_mc[1], (int)fast_piv(P, 1, g, p + 1, first)[FP_N * P.RM + x]);
            __syncthreads();
            fcap = min(vals, max(s_mc[0], s_mc[1]));
            const double *nL = fast_near(P, 0, g, p - 1, first), *nR = fast_near(P, 1, g, p + 1, first);
            for (int x = tid; x < fcap * P.RM; x += blockDim.x) { const int c = x % P.RM; sNL[x] = (c < r0) ? nL[x] : 0.0; sNR[x] = (c < r2) ? nR[x] : 0.0; }
        }
    } else if (usem) {
        __syncthreads();
        const double *mu = P.aux;
        for (int x = tid; x < r0 * VS; x += blockDim.x) { const int c = x / VS, o = x - c * VS; DLv[x] = (o < p - 1) ? par[Lt[(size_t)o * P.RM + c] - 1] - mu[o] : 0.0; }
        for (int x = tid; x < r2 * VS; x += blockDim.x) { const int c = x / VS, o = x - c * VS; DRv[x] = (o < m - p - 1) ? par[Rt[(size_t)o * P.RM + c] - 1] - mu[p + 1 + o] : 0.0; }
    } else {
    for (int x = tid; x < r0 * VS; x += blockDim.x) { const int c = x / VS, o = x - c * VS; LT[x] = (o < p - 1) ? Lt[(size_t)o * P.RM + c] : (short)1; }
    for (int x = tid; x < r2 * VS; x += blockDim.x) { const int c = x / VS, o = x - c * VS; RT[x] = (o < m - p - 1) ? Rt[(size_t)o * P.RM + c] : (short)1; }
    }
    // rnd.f90:120: d(nlot,2) column-major from the (never seeded) run-time generator.  Draw #k comes from the
    // generator word 48271^(2k+1): split as [48271^(2 pos+1)] * [48271^2]^il so that the long jump-ahead is done
    // once per block (threads 32/33) while every thread raises the short power
    __shared__ unsigned long long sA[2];
    int Kc = 0, Kr = 0;
    const int CH = (nbl == 1) ? nlot : 64;                     // candidates per block
    const int il_first = blk * CH + tid, il_end = min(nlot, (blk + 1) * CH);
    unsigned long long bil = 0;
    if (phase != 2) {
    if (tid == 32) sA[0] = ttx_minstd_pow(2 * gs.rngpos + 1);
    if (tid == 33) sA[1] = ttx_minstd_pow(2 * (gs.rngpos + nlot) + 1);
    bil = ttx_minstd_pow(2ull * (unsigned long long)il_first);
    // zero-weight positions (existing pivots), :432-439
    bond_zero_lists(vip_ptr(P, g, p, first), r1, r0, n2, tid, zc, zr, zcs, zrs, keepc, keepr, &nzc, &nzr);
    STAMP(gs, 0);   // 1: tables + powers + zero lists
    Kc = r0 * n1 - nzc; Kr = n2 * r2 - nzr;
    if (P.cdf_tab && Kc <= P.cdf_kmax && Kr <= P.cdf_kmax) {
        // segment tables depend on K only: precomputed at ttx_create, copied here
        if (tid < 64) { if (tid < P.cdf_ns[Kc]) segc[tid] = P.cdf_tab[(size_t)Kc * TTX_TABSEG + tid]; if (tid == 0) nsc = P.cdf_ns[Kc]; }
        else if (tid < 128) { const int t2 = tid - 64; if (t2 < P.cdf_ns[Kr]) segr[t2] = P.cdf_tab[(size_t)Kr * TTX_TABSEG + t2]; if (t2 == 0) nsr = P.cdf_ns[Kr]; }
    } else {
        if (tid == 0) nsc = ttx_cdf_build(Kc, segc);
        if (tid == 64) nsr = ttx_cdf_build(Kr, segr);
    }
    }
    __syncthreads();
    STAMP(gs, 0);   // 2: cdf
    double ma = 0.0;
    double ba = -1.0, bv = 0.0; int bi = INT_MAX;
    for (int il = il_first; il < il_end; il += blockDim.x) {
        int i, j, k, q;
        if (phase != 2) {
            double d1, d2;
            if (il == il_first) { d1 = ttx_flang_from_word(ttx_mulmod31(sA[0], bil)); d2 = ttx_flang_from_word(ttx_mulmod31(sA[1], bil)); }
            else { d1 = ttx_flang_draw(gs.rngpos + il); d2 = ttx_flang_draw(gs.rngpos + nlot + il); }
            const int x = ttx_lottery_index(segc, nsc, Kc, r0 * n1, zc, nzc, d1);      // rnd.f90:122-123
            const int y = ttx_lottery_index(segr, nsr, Kr, n2 * r2, zr, nzr, d2);
            i = (x - 1) % r0 + 1; j = (x - 1) / r0 + 1; k = (y - 1) % n2 + 1; q = (y - 1) / n2 + 1;   // :447-452
            if (phase == 1) { int *c_ = P.lotc + ((size_t)g * P.lot_max + il) * 4; c_[0] = i; c_[1] = j; c_[2] = k; c_[3] = q; continue; }
        } else {
            const int *c_ = P.lotc + ((size_t)g * P.lot_max + il) * 4;
            i = c_[0]; j = c_[1]; k = c_[2]; q = c_[3];
        }
        lot[4 * il] = i; lot[4 * il + 1] = j; lot[4 * il + 2] = k; lot[4 * il + 3] = q;
        double f;
        if (phase == 2) f = P.lotf[(size_t)g * P.lot_max + il];
        else if (fastp) f = (FUN == FUN_MVN) ? mvn_fast_value(P, g, p, first, i - 1, j - 1, k - 1, q - 1, mvn_fast_cross(P, g, p, first, i - 1, q - 1))
                                             : de_fast_elem4(P, g, p, first, i - 1, j - 1, k - 1, q - 1, sNL, sNR, fcap);
        else if (usem) f = f_mvn_rows<2>(m, P.auxT, P.mvn_norm, DLv + (size_t)(i - 1) * VS, p - 1, par[j - 1] - P.aux[p - 1], par[k - 1] - P.aux[p],
                                    DRv + (size_t)(q - 1) * VS);
        else if (FUN == FUN_ISING && P.ising_id != 1 && P.deTL) {
            const size_t NP = (size_t)P.de_npair, tsz = NP * P.RM;
            const double *TL = P.deTL + (size_t)g * tsz + (size_t)(i - 1) * NP, *UL = P.deUL + ((size_t)g * P.RM + (i - 1)) * (m + 1);
            const double *TR = P.deTR + (size_t)g * tsz + (size_t)(q - 1) * NP;
            const short *pa_ = LT + (size_t)(i - 1) * VS, *pb_ = RT + (size_t)(q - 1) * VS;
            const double ap = P.de_cut ? de_pairs_ctab(m, par - 1, p - 1, TL, P.deCL + ((size_t)g * P.RM + (i - 1)) * (m + 1), UL, j, k, pb_, 0, TR,
                                                       P.deCR + ((size_t)g * P.RM + (q - 1)) * (m + 1))
                            : P.de_unit ? de_pairs_tab<true>(m, par - 1, p - 1, TL, UL, j, k, pb_, 0, TR)
                                        : de_pairs_tab<false>(m, par - 1, p - 1, TL, UL, j, k, pb_, 0, TR);
            f = de_finish<2>(P.ising_id, ap, m, P.n[1], par, pa_, p - 1, j, k, pb_);
        } else {
            Src4 sx{LT + (size_t)(i - 1) * VS, p - 1, j, k, RT + (size_t)(q - 1) * VS};
            f = eval_src4<FUN>(P, par, sx, (long)g * P.HS + il);                   // :455-463
        }
        ma = fmax(ma, fabs(f));
        const double *c = Cp + (i - 1) + (size_t)P.RM * (j - 1), *w = Wq + (k - 1) + (size_t)P.NM * (q - 1);
        double t = 0.0;                                                            // ddot, :474
#pragma unroll 8
        for (int s = 0; s < r1; s++) t = t + c[P.SS * s] * w[P.SW * s];
        const double b = f - t;
        const double a = fabs(b);
        if (a > ba || (a == ba && il < bi)) { ba = a; bv = b; bi = il; }
    }
    STAMP(gs, 0);   // 3: selection + eval + ddot
    if (phase == 1) { if (tid == 0) gs.S[0] = st; return; }
    if (HOST_PASS1(FUN, P)) return;
    ma = block_max(ma, sha);
    block_argmax(ba, bv, bi, sha, shv, shi);
    if (nbl > 1) {
        STAMP(gs, 0);   // (several blocks: block reductions; the fold of the partials is not stamped)
        STAMP_END(gs, 0);
        // this block's partial, then the arrival counter; the last block folds all partials (blocks sit on different XCDs:
        // the fence pair makes the records visible across their L2s)
        LotPart *lp = P.lotp + (size_t)g * P.lot_nb;
        if (tid == 0) {
            LotPart r; r.ab = ba; r.bv = bv; r.ma = ma; r.il = bi; r.pad = 0;
            if (bi != INT_MAX) { r.i = lot[4 * bi]; r.j = lot[4 * bi + 1]; r.k = lot[4 * bi + 2]; r.q = lot[4 * bi + 3]; } else if (il_first < nlot) { r.i = lot[4 * il_first]; r.j = lot[4 * il_first + 1]; r.k = lot[4 * il_first + 2]; r.q = lot[4 * il_first + 3]; }   // no comparable candidate: the block's first one
            else { r.i = r.j = r.k = r.q = 1; }
            lp[blk] = r;
            __threadfence();
            s_last = (atomicAdd(&P.lot_ctr[g], 1u) == (unsigned)(nbl - 1));
        }
        __syncthreads();
        if (!s_last) return;
        if (tid == 0) {
            __threadfence();
            P.lot_ctr[g] = 0u;
            int wi = 0, wj = 0, wk = 0, wq = 0;
            ba = -1.0; bv = 0.0; bi = INT_MAX; ma = 0.0;
            for (int b = 0; b < nbl; b++) {
                const LotPart r = lp[b];
                ma = fmax(ma, r.ma);
                if (r.ab > ba || (r.ab == ba && r.il < bi)) { ba = r.ab; bv = r.bv; bi = r.il; wi = r.i; wj = r.j; wk = r.k; wq = r.q; }
            }
            if (bi == INT_MAX) { const LotPart r0 = lp[0]; wi = r0.i; wj = r0.j; wk = r0.k; wq = r0.q; }   // every residual a NaN: the first candidate, as idamax
            gs.amax = fmax(gs.amax, ma);                         // :467
            gs.neval += nlot;                                    // :465
            gs.rngpos += 2ull * nlot;
            st.ii = wi; st.jj = wj; st.kk = wk; st.qq = wq;      // :479-484
            st.pivot = bv;
            gs.S[0] = st;
        }
        return;
    }
    if (tid == 0) {
        gs.amax = fmax(gs.amax, ma);                             // :467
        gs.neval += nlot;                                        // :465
        gs.rngpos += 2ull * nlot;
        if (bi == INT_MAX) bi = 0;                               // every residual a NaN: the first candidate, as idamax
        st.ii = lot[4 * bi]; st.jj = lot[4 * bi + 1]; st.kk = lot[4 * bi + 2]; st.qq = lot[4 * bi + 3];   // :479-484
        st.pivot = bv;
        gs.S[0] = st;
    }
    STAMP(gs, 0);   // 7: reductions + state
    STAMP_END(gs, 0);
}

// ------------------------------------------------------------------------------------------------
// K_halfstep: one rook half-step = fiber evaluation (K1) + residual against the cross factor (K2, the
// "maxvol" kernel of the north star: a bandwidth-bound slab sweep) + block arg-max.
// lib/dmrgg.f90:518-582 (rook), :492-513 (piv=0).  grid = (fiber blocks, groups).
// mode 0: rook (type alternates, residual unless crs reached 2*piv); mode 1: piv=0 (h=0 column, h=1 row,
// no residual).
// ------------------------------------------------------------------------------------------------
template <int FUN>
__global__ __launch_bounds__(TTX_BLK) void k_halfstep(DevProb P, int h, int dir, int mode, int vals)
{
    extern __shared__ __align__(16) double dyn[];
    __shared__ StepState cur;
    __shared__ double sha[4], shv[4]; __shared__ int shi[4];
    const int g = blockIdx.y, tid = threadIdx.x, m = P.d;
    GroupState &gs = P.gs[g];
    STAMP_DECL;
    if (tid < 64) {
        resolve_state_wave(cur, gs.S[h], gs.Pt[(h + 1) & 1], tid);
        if (tid == 0 && (mode == 3 || mode == 4)) { cur.kk = ((int)blockIdx.z + P.zbase) % cur.n2 + 1; cur.qq = ((int)blockIdx.z + P.zbase) / cur.n2 + 1; }   // :356-369 column (k,q)
    }
    __syncthreads();
    const int zcol = (int)blockIdx.z + P.zbase;
    if (mode == 3 || mode == 4) { if (!cur.active || zcol >= cur.n2 * cur.r2) return; }
    else if (!cur.active || cur.done) { if (blockIdx.x == 0 && tid == 0) gs.S[h + 1] = cur; return; }
    STAMP(gs, 1);   // 0: resolve
    const bool iscol = (mode == 3 || mode == 4) ? true : rook_iscol(mode, h, dir);
    const int p = cur.p, r0 = cur.r0, r1 = cur.r1, r2 = cur.r2, n1 = cur.n1, n2 = cur.n2, first = gs.first;
    const int nf = iscol ? r0 * n1 : n2 * r2;
    if ((int)(blockIdx.x * TTX_BLK) >= nf) return;
    // LDS: par | xs[RM] | then either VALUE rows (Ising C when they fit: node and weight doubles, one 16-byte
    // aligned row per varying index + one fixed row) or INDEX rows (short) for the generic integrands
    const int VS = ((m + 7) & ~7) + 8;
    double *par = dyn, *xs = dyn + ((P.npar + 1) & ~1);
    double *vbase = xs + ((P.RM + 1) & ~1);
    const double *Cp = core_ptr(P, P.col, g, p, first), *Wq = core_ptr(P, P.row, g, p + 1, first);
    const short *Lt = L_ptr(P, g, p - 1, first), *Rt = R_ptr(P, g, p + 1, first);
    for (int x = tid; x < P.npar; x += TTX_BLK) par[x] = P.par[x];
    const int vrows = iscol ? p - 1 : m - p - 1, vcols = iscol ? r0 : r2;
    const bool usev = (FUN == FUN_ISING) && (P.ising_id == 1) && (vals != 0);
    const int n1m = P.n[1];
    // TTX_ARITH=fast (ttx_fast.h): the fixed side of the fiber as a decay vector far[] (Ising D/E) or the cross terms of the
    // varying pivots with the fixed pivot (mvn), then O(small) work per element from the tables of k_fast_tables
    const bool fastp = fast_path(P, FUN);
    double *far = vbase, *Xv = vbase + ((max(P.FD, TTX_FNR) + 3) & ~1);
    __shared__ int s_nfar; __shared__ double s_rfix;
    const int fside = iscol ? 0 : 1;                                         // the varying side
    const int vfix = iscol ? cur.qq - 1 : cur.ii - 1, xfix = iscol ? cur.kk - 1 : cur.jj - 1;   // fixed pivot (other side), fixed mode index next to the free dim
    if (fastp && FUN == FUN_ISING) de_fast_fiber_stage(P, fside, g, p, first, vfix, xfix, far, s_nfar, s_rfix, tid);
    if (fastp && FUN == FUN_MVN) mvn_fast_fiber_stage(P, iscol, g, p, first, iscol ? r0 : r2, vfix, Xv, tid);
    __syncthreads();      // par is read below when staging values
    if (usev) {
        // rows: [0 .. vcols) varying index, row vcols = fixed side; each row: VS node values then VS weight values
        double *fn = vbase + (size_t)vcols * 2 * VS, *fw = fn + VS;
        for (int x = tid; x < vcols * VS; x += TTX_BLK) {
            const int c = x / VS, o = x % VS;
            int ix = 1;
            if (o < vrows) ix = iscol ? Lt[(size_t)o * P.RM + c] : Rt[(size_t)o * P.RM + c];
            vbase[(size_t)c * 2 * VS + o] = par[ix - 1];
            vbase[(size_t)c * 2 * VS + VS + o] = par[n1m + ix - 1];
        }
        for (int x = tid; x < VS; x += TTX_BLK) {
            int ix = 1;
            if (iscol) { if (x == 0) ix = cur.kk; else if (x < m - p) ix = Rt[(size_t)(x - 1) * P.RM + (cur.qq - 1)]; }
            else       { if (x < p - 1) ix = Lt[(size_t)x * P.RM + (cur.ii - 1)]; else if (x == p - 1) ix = cur.jj; }
            fn[x] = par[ix - 1]; fw[x] = par[n1m + ix - 1];
        }
    }
    const bool usem = (FUN == FUN_MVN) && (vals != 0);      // rows of differences x - mu (doubles): [vcols][VS] + fixed row
    if (usem) {
        const double *mu = P.aux;
        double *df = vbase + (size_t)vcols * VS;
        if (iscol) {
            for (int x = tid; x < vcols * VS; x += TTX_BLK) { const int c = x / VS, o = x % VS; vbase[x] = (o < vrows) ? par[Lt[(size_t)o * P.RM + c] - 1] - mu[o] : 0.0; }
            for (int x = tid; x < VS; x += TTX_BLK)
                df[x] = (x == 0) ? par[cur.kk - 1] - mu[p] : (x < m - p) ? par[Rt[(size_t)(x - 1) * P.RM + (cur.qq - 1)] - 1] - mu[p + x] : 0.0;
        } else {
            for (int x = tid; x < vcols * VS; x += TTX_BLK) { const int c = x / VS, o = x % VS; vbase[x] = (o < vrows) ? par[Rt[(size_t)o * P.RM + c] - 1] - mu[p + 1 + o] : 0.0; }
            for (int x = tid; x < VS; x += TTX_BLK)
                df[x] = (x < p - 1) ? par[Lt[(size_t)x * P.RM + (cur.ii - 1)] - 1] - mu[x] : (x == p - 1) ? par[cur.jj - 1] - mu[p - 1] : 0.0;
        }
    }
    short *fxs = (short *)vbase;
    short *vt = fxs + VS;
    if (!usev && !usem && !fastp) {
        if (iscol) {   // varying: left pivot i (dims 1..p-1) and j; fixed: kk and the right multi-index of qq (dims p+1..m)
            for (int x = tid; x < vcols * VS; x += TTX_BLK) { const int c = x / VS, o = x % VS; vt[x] = (o < vrows) ? Lt[(size_t)o * P.RM + c] : (short)1; }
            for (int x = tid; x < VS; x += TTX_BLK) fxs[x] = (x == 0) ? (short)cur.kk : (x < m - p) ? Rt[(size_t)(x - 1) * P.RM + (cur.qq - 1)] : (short)1;
        } else {       // varying: k and right pivot q (dims p+2..m); fixed: left multi-index of ii and jj (dims 1..p)
            for (int x = tid; x < vcols * VS; x += TTX_BLK) { const int c = x / VS, o = x % VS; vt[x] = (o < vrows) ? Rt[(size_t)o * P.RM + c] : (short)1; }
            for (int x = tid; x < VS; x += TTX_BLK) fxs[x] = (x < p - 1) ? Lt[(size_t)x * P.RM + (cur.ii - 1)] : (x == p - 1) ? (short)cur.jj : (short)1;
        }
    }
    if (iscol) for (int s = tid; s < r1; s += TTX_BLK) xs[s] = Wq[(cur.kk - 1) + (size_t)P.NM * (cur.qq - 1) + P.SW * s];
    else       for (int s = tid; s < r1; s += TTX_BLK) xs[s] = Cp[(cur.ii - 1) + (size_t)P.RM * (cur.jj - 1) + P.SS * s];
    __syncthreads();
    STAMP(gs, 1);   // 1: staging
    const int t = blockIdx.x * TTX_BLK + tid;
    const bool live = t < nf;
    double a = 0.0;
    int u = 0, v = 0;                         // col: (i,j) 0-based ; row: (k,q) 0-based
    if (live) {
        if (iscol) { u = t % r0; v = t / r0; } else { u = t % n2; v = t / n2; }
        if (fastp && FUN == FUN_ISING) {
            a = de_fast_fiber_elem(P, iscol, g, p, first, iscol ? u : v, iscol ? v : u, vfix, xfix, par, far, s_nfar, s_rfix);
        } else if (fastp && FUN == FUN_MVN) {
            a = mvn_fast_fiber_elem(P, iscol, g, p, first, u, v, vfix, xfix, Xv);
        } else if (usev) {
            const double *fn = vbase + (size_t)vcols * 2 * VS, *fw = fn + VS;
            if (iscol) { const double *rn = vbase + (size_t)u * 2 * VS; a = f_ising_c3v(m, p - 1, rn, rn + VS, par[v], par[n1m + v], fn, fw); }
            else       { const double *rn = vbase + (size_t)v * 2 * VS; a = f_ising_c3v(m, p, fn, fw, par[u], par[n1m + u], rn, rn + VS); }
        } else if (FUN == FUN_ISING && P.ising_id != 1 && P.deTL) {
            const size_t NP = (size_t)P.de_npair, tsz = NP * P.RM;
            const double *TL = P.deTL + (size_t)g * tsz, *UL = P.deUL + (size_t)g * P.RM * (m + 1), *TR = P.deTR + (size_t)g * tsz;
            double pa_;
            const int *CL = P.deCL + (size_t)g * P.RM * (m + 1), *CR = P.deCR + (size_t)g * P.RM * (m + 1);
            if (P.de_cut) {
                if (iscol) pa_ = de_pairs_ctab(m, par - 1, p - 1, TL + (size_t)u * NP, CL + (size_t)u * (m + 1), UL + (size_t)u * (m + 1), v + 1, cur.kk, fxs, 1,
                                               TR + (size_t)(cur.qq - 1) * NP, CR + (size_t)(cur.qq - 1) * (m + 1));
                else pa_ = de_pairs_ctab(m, par - 1, p - 1, TL + (size_t)(cur.ii - 1) * NP, CL + (size_t)(cur.ii - 1) * (m + 1), UL + (size_t)(cur.ii - 1) * (m + 1), cur.jj, u + 1,
                                         vt + (size_t)v * VS, 0, TR + (size_t)v * NP, CR + (size_t)v * (m + 1));
                a = iscol ? de_finish<1>(P.ising_id, pa_, m, n1m, par, vt + (size_t)u * VS, p - 1, v + 1, 0, fxs) : de_finish<1>(P.ising_id, pa_, m, n1m, par, fxs, p, u + 1, 0, vt + (size_t)v * VS);
            } else
            if (iscol) {     // left pivot u varies, s1 = v+1, s2 = kk, right pivot qq fixed (fxs = [kk, right dims])
                pa_ = de_pairs_tab<false>(m, par - 1, p - 1, TL + (size_t)u * NP, UL + (size_t)u * (m + 1), v + 1, cur.kk, fxs, 1, TR + (size_t)(cur.qq - 1) * NP);
                a = de_finish<1>(P.ising_id, pa_, m, n1m, par, vt + (size_t)u * VS, p - 1, v + 1, 0, fxs);
            } else {         // left pivot ii fixed (fxs = [left dims, jj]), s1 = jj, s2 = u+1, right pivot v varies
                pa_ = de_pairs_tab<false>(m, par - 1, p - 1, TL + (size_t)(cur.ii - 1) * NP, UL + (size_t)(cur.ii - 1) * (m + 1), cur.jj, u + 1, vt + (size_t)v * VS, 0, TR + (size_t)v * NP);
                a = de_finish<1>(P.ising_id, pa_, m, n1m, par, fxs, p, u + 1, 0, vt + (size_t)v * VS);
            }
        } else if (usem) {
            const double *mu = P.aux, *df = vbase + (size_t)vcols * VS;
            if (iscol) a = f_mvn_rows<1>(m, P.auxT, P.mvn_norm, vbase + (size_t)u * VS, p - 1, par[v] - mu[p - 1], 0.0, df);
            else       a = f_mvn_rows<1>(m, P.auxT, P.mvn_norm, df, p, par[u] - mu[p], 0.0, vbase + (size_t)v * VS);
        } else {
            Src3 sx;
            if (iscol) { sx.pa = vt + (size_t)u * VS; sx.A = p - 1; sx.self = v + 1; sx.pb = fxs; }
            else       { sx.pa = fxs; sx.A = p; sx.self = u + 1; sx.pb = vt + (size_t)v * VS; }
            a = eval_src3<FUN, true>(P, par, sx, (long)g * P.HS + t);         // :520-526 / :553-559
        }
        if (mode == 4) P.sb[(size_t)g * ((size_t)P.RM * P.NM) * ((size_t)P.RM * P.NM) + (size_t)nf * zcol + t] = a;   // superblock column (k,q)
        else if (mode != 3) (iscol ? P.acol : P.arow)[(size_t)g * P.RM * P.NM + t] = a;
    }
    STAMP(gs, 1);   // 2: eval
    if (HOST_PASS1(FUN, P)) return;
    double mx = block_max(live ? fabs(a) : 0.0, sha);
    if (tid == 0 && mode != 1) atomic_max_pos(&gs.amax, mx);                  // :531 / :564 (the piv = 0 branch :492-513 does not touch amax)
    const RookTurn turn = rook_turn(P.piv, mode, h, dir, cur.crs, cur.havecol, cur.haverow);     // (modes 3, 4: resid = false, the rest unused -- they return before the publish)
    const bool resid = (mode == 3) || turn.resid;
    if (resid) {
        double b = a, ab = -1.0; int bi = INT_MAX;
        if (live) {
            if (iscol) {   // dgemv 'n', alpha=-1 (:538): b += (-x_s) * col(:, s)
                const double *c = Cp + u + (size_t)P.RM * v;
#pragma unroll 8
                for (int s = 0; s < r1; s++) b = b + (-xs[s]) * c[P.SS * s];
            } else {       // dgemv 't', alpha=-1 (:571): b += -1 * sum_s row(s, kq) * x_s
                const double *w = Wq + u + (size_t)P.NM * v;
                double tt = 0.0;
#pragma unroll 8
                for (int s = 0; s < r1; s++) tt = tt + w[P.SW * s] * xs[s];
                b = b + (-1.0) * tt;
            }
            ab = fabs(b); bi = t;
        }
        STAMP(gs, 1);   // 3: residual
        block_argmax(ab, b, bi, sha, shv, shi);
        if (tid == 0) {
            Partial pr; pr.absmax = ab; pr.val = b; pr.idx = bi; pr.pad = 0;
            if (mode == 3) {   // superblock linear index ijkq = t + r0*n1*(column), :388-394
                if (bi != INT_MAX) pr.idx = bi + r0 * n1 * zcol;
                P.pfull[((size_t)g * P.NM * P.RM + zcol) * P.nfb + blockIdx.x] = pr;
            } else gs.Pt[h & 1][blockIdx.x] = pr;
        }
    }
    if (mode == 3 || mode == 4) {
        if (blockIdx.x == 0 && zcol == 0 && tid == 0 && P.hostpass != 1) gs.neval += (long long)r0 * n1 * n2 * r2;   // :372
        return;
    }
    if (blockIdx.x == 0 && tid == 0) halfstep_publish(gs, h, cur, turn, mode, nf, r1, (nf + TTX_BLK - 1) / TTX_BLK);
    STAMP(gs, 1);   // 4: argmax + state
    STAMP_END(gs, 1);
}

// ------------------------------------------------------------------------------------------------
// K_accept: threshold test and in-place append of the new cross (lib/dmrgg.f90:598-758).
// block roles along grid.x: [0,nA) column factor + raw column; [nA,2nA) row factor + raw row;
// [2nA, 2nA+NM) left-neighbour row fix-up (one column j each); [.., +NM) right-neighbour column fix-up
// (one row k each); last block: scalars, packed LU, pivot sets and index tables.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TTX_BLK) void k_accept(DevProb P, int H, int nA)
{
    extern __shared__ __align__(16) double dyn[];
    __shared__ StepState cur;
    __shared__ int s_upd;
    __shared__ double s_bc;
    const int g = blockIdx.y, tid = threadIdx.x, m = P.d;
    GroupState &gs = P.gs[g];
    if (tid < 64) resolve_state_wave(cur, gs.S[H], gs.Pt[(H + 1) & 1], tid);
    if (tid == 0) {
        s_upd = cur.active && accept_pivot(cur.pivot, gs.amax, gs.pivotmax_prev, P.small_element, P.small_pivot);
    }
    __syncthreads();
    if (!cur.active) return;
    const int p = cur.p, r0 = cur.r0, r1 = cur.r1, r2 = cur.r2, n1 = cur.n1, n2 = cur.n2, first = gs.first;
    const int bx = blockIdx.x, nblk = gridDim.x;
    int *tape = P.tape + ((size_t)g * (m + 2) + p) * 4;
    if (!s_upd) {
        if (bx == nblk - 1 && tid == 0) { tape[0] = tape[1] = tape[2] = tape[3] = -1; P.upd[(size_t)g * (m + 2) + p] = 0; }
        return;
    }
    const int ii = cur.ii - 1, jj = cur.jj - 1, kk = cur.kk - 1, qq = cur.qq - 1;   // 0-based
    double *Ap = core_ptr(P, P.arg, g, p, first), *Aq = core_ptr(P, P.arg, g, p + 1, first);
    double *Cp = core_ptr(P, P.col, g, p, first), *Wq = core_ptr(P, P.row, g, p + 1, first);
    const double *acol = P.acol + (size_t)g * P.RM * P.NM, *arow = P.arow + (size_t)g * P.RM * P.NM;
    double *xs = dyn;   // RM doubles

    if (bx < nA) {
        // role A: arg(p)(:,:,r1+1) = acol1 (:662-668); col(p)(:,:,r1+1) = (acol1 - col*Ucol) / pivot (:701, d2_lual from=r1+1)
        for (int s = tid; s < r1; s += TTX_BLK) xs[s] = Wq[kk + (size_t)P.NM * qq + P.SW * s];
        __syncthreads();
        int t = bx * TTX_BLK + tid;
        if (t < r0 * n1) {
            int i = t % r0, j = t / r0;
            size_t o = i + (size_t)P.RM * j;
            double a = acol[t];
            Ap[o + P.SS * r1] = a;
            double y = a;
            for (int s = 0; s < r1; s++) y = y + (-xs[s]) * Cp[o + P.SS * s];
            y = (1.0 / cur.pivot) * y;
            Cp[o + P.SS * r1] = y;
        }
    } else if (bx < 2 * nA) {
        // role B: arg(p+1)(r1+1,:,:) = arow1 (:669-674); row(p+1)(r1+1,:,:) = arow1 - Lrow'*row (:702, d2_luar from=r1+1)
        for (int s = tid; s < r1; s += TTX_BLK) xs[s] = Cp[ii + (size_t)P.RM * jj + P.SS * s];
        __syncthreads();
        int t = (bx - nA) * TTX_BLK + tid;
        if (t < n2 * r2) {
            int k = t % n2, q = t / n2;
            double a = arow[t];
            Aq[r1 + (size_t)P.RM * k + P.SS * q] = a;
            size_t o = k + (size_t)P.NM * q;
            double tt = 0.0;
            for (int s = 0; s < r1; s++) tt = tt + Wq[o + P.SW * s] * xs[s];
            Wq[o + P.SW * r1] = a + (-1.0) * tt;
        }
    } else if (bx < 2 * nA + P.NM) {
        // role C: row(p)(:, j, r1+1) = L(p-1)^-1 * acol1(:, j)  (:715-728, d2_luar full) -- wavefront over i
        int j = bx - 2 * nA;
        if (p <= first || j >= n1) return;
        const double *gI = inv_ptr(P, g, p - 1, first);
        double *Wp = core_ptr(P, P.row, g, p, first);
        double a = (tid < r0) ? acol[tid + r0 * j] : 0.0, tmp = 0.0, xf = 0.0;
        if (r0 <= 64) {                               // one wave: the solve runs as a lane-read wavefront over the LDS-staged LU (as k_exch_boundary)
            double *lu = dyn;
            for (int x = tid; x < r0 * r0; x += TTX_BLK) lu[x] = gI[x];
            __syncthreads();
            if (tid < 64) xf = dev_solve_L<1>(lu, r0, a, tid, 0);
        } else
        for (int s = 0; s < r0; s++) {
            if (tid == s) { xf = a + (-1.0) * tmp; if (s == 0) xf = a; s_bc = xf; }
            __syncthreads();
            if (tid > s && tid < r0) tmp = tmp + s_bc * gI[tid * tid + s];
            __syncthreads();
        }
        if (tid < r0) Wp[j + (size_t)P.NM * r1 + P.SW * tid] = xf;
    } else if (bx < 2 * nA + 2 * P.NM) {
        // role D: col(p+1)(r1+1, k, :) = arow1(k, :) * U(p+1)^-1  (:730-749, d2_lual full) -- wavefront over q
        int k = bx - 2 * nA - P.NM;
        if (p >= gs.last || k >= n2) return;
        const double *gI = inv_ptr(P, g, p + 1, first);
        double *Cq = core_ptr(P, P.col, g, p + 1, first);
        double y = (tid < r2) ? arow[k + n2 * tid] : 0.0;
        if (r2 <= 64) {
            double *lu = dyn;
            for (int x = tid; x < r2 * r2; x += TTX_BLK) lu[x] = gI[x];
            __syncthreads();
            if (tid < 64) y = dev_solve_U<1>(lu, r2, y, dev_solve_rdg(lu, r2, tid), tid, 0);
        } else
        for (int s = 0; s < r2; s++) {
            if (tid == s) { y = (1.0 / gI[(s + 1) * (s + 1) - 1]) * y; s_bc = y; }
            __syncthreads();
            if (tid > s && tid < r2) y = y + (-gI[tid * tid + tid + s]) * s_bc;
            __syncthreads();
        }
        if (tid < r2) Cq[r1 + (size_t)P.RM * k + P.SS * tid] = y;
    } else {
        // role E: scalars (:604-635), packed LU (:649-660), index tables (replaces the vip walk of :1062-1075)
        double *gI = inv_ptr(P, g, p, first);
        for (int s = tid; s < r1; s += TTX_BLK) {
            gI[r1 * r1 + s] = Cp[ii + (size_t)P.RM * jj + P.SS * s];
            gI[r1 * r1 + r1 + s] = Wq[kk + (size_t)P.NM * qq + P.SW * s];
        }
        append_tables(P, g, p, first, r1, cur.ii, cur.jj, cur.kk, cur.qq, tid, TTX_BLK);
        if (P.arith && P.fpersist && tid < 128) {
            // TTX_ARITH=fast, Ising D/E: the table entries of the new pivot as a LEFT multi-index of bond p (parent: left pivot ii of bond
            // p-1, extended by node jj) and as a RIGHT multi-index of bond p (parent: right pivot qq of bond p+1, extended by node kk)
            const int sd = tid >> 6, lane_ = tid & 63;
            const double *pn = fast_near(P, sd, g, sd == 0 ? p - 1 : p + 1, first) + (sd == 0 ? ii : qq);
            const double *pp_ = fast_piv(P, sd, g, sd == 0 ? p - 1 : p + 1, first) + (sd == 0 ? ii : qq);
            const int nd = sd == 0 ? jj : kk;
            if (P.fun_id == FUN_MVN) {       // mvn: the new dimension is p-1 (0-based) behind the left parent's p-1 dims, p in front of the right parent's m-p-1
                const int dnew = sd == 0 ? p - 1 : p, plen = sd == 0 ? p - 1 : m - p - 1;
                mvn_entry_child(P, sd, fast_dv(P, sd, g, sd == 0 ? p - 1 : p + 1, first) + (sd == 0 ? ii : qq), pn, pp_, plen, dnew, P.par[nd] - P.aux[dnew],
                                fast_dv(P, sd, g, p, first) + r1, fast_near(P, sd, g, p, first) + r1, fast_piv(P, sd, g, p, first) + r1, lane_);
            } else
            fast_entry_child(pn, pp_, P.par[nd], P.par[P.n[1] + nd], fast_near(P, sd, g, p, first) + r1, fast_piv(P, sd, g, p, first) + r1, P.RM, lane_);
        }
        if (tid == 0) {
            append_scalars(P, g, p, first, r1, cur.ii, cur.jj, cur.kk, cur.qq, cur.pivot);
            pivot_range(gs.pivotmax, gs.pivotmin, fabs(cur.pivot));
        }
    }
}

// ------------------------------------------------------------------------------------------------
// dtt_accchk (lib/dmrgg.f90:1081-1166): one wave per random sample.  out[4*il..] = (|aval-bval|, (aval-bval)^2,
// aval, aval^2); ind_out[il*d..] = the sample's multi-index
// ------------------------------------------------------------------------------------------------
struct ListIdx { const int *ind; __device__ __forceinline__ int operator()(int s) const { return ind[s - 1]; } };
template <int FUN>
__global__ __launch_bounds__(64) void k_accchk(DevProb P, unsigned long long rngpos, int nlot, const int *owner, double *out, int *ind_out, int il0)
{
    extern __shared__ __align__(16) double dyn[];
    const int il = il0 + blockIdx.x, tid = threadIdx.x, m = P.d;
    double *par = dyn, *x = dyn + ((P.npar + 1) & ~1), *z = x + P.RM;
    int *ind = (int *)(z + P.RM);
    for (int s = tid; s < P.npar; s += 64) par[s] = P.par[s];
    for (int i = tid; i < m; i += 64) {                      // irnd: int(d*maxi)+1, draws in sample-major order (:1119-1122)
        double d = ttx_flang_draw(rngpos + (unsigned long long)il * m + i);
        ind[i] = (int)(d * P.n[i + 1]) + 1;
        ind_out[(size_t)il * m + i] = ind[i];
    }
    __syncthreads();
    double aval = 0.0;
    if (tid == 0) { ListIdx ix{ind}; aval = eval_fun<FUN>(P, par, ix, (long)blockIdx.x); }
    if (HOST_PASS1(FUN, P)) return;
    // dtt_ijk (lib/tt.f90:630-652): x = U_m(:, ind_m, 1); for i = m-1..1: x = U_i(:, ind_i, :) x
    {
        const int g = owner[m], first = P.gs[g].first;
        const int *r = P.r + (size_t)g * (m + 2);
        const double *A = core_ptr(P, P.arg, g, m, first);
        if (tid < r[m - 1]) x[tid] = A[tid + (size_t)P.RM * (ind[m - 1] - 1)];
    }
    __syncthreads();
    for (int i = m - 1; i >= 1; i--) {
        const int g = owner[i], first = P.gs[g].first;
        const int *r = P.r + (size_t)g * (m + 2);
        const int q0 = r[i - 1], q1 = r[i];
        const double *A = core_ptr(P, P.arg, g, i, first) + (size_t)P.RM * (ind[i - 1] - 1);
        for (int t = tid; t < q0; t += 64) {
            double s = 0.0;
            for (int k = 0; k < q1; k++) s = s + A[t + P.SS * k] * x[k];
            z[t] = s;
        }
        __syncthreads();
        for (int t = tid; t < q0; t += 64) x[t] = z[t];
        __syncthreads();
    }
    if (tid == 0) {
        const double bval = x[0], e = aval - bval;
        out[4 * (size_t)il] = fabs(e); out[4 * (size_t)il + 1] = e * e; out[4 * (size_t)il + 2] = aval; out[4 * (size_t)il + 3] = aval * aval;
    }
}
