// ttx_exchange.h -- the per-sweep neighbour exchange between bond groups: pack, MAX, apply, boundary blocks, and all of it in one
// launch (k_exch_tail).
#pragma once
#include "ttx_kernels.h"
#include "ttx_de.h"       // de_corner_wave
#include "ttx_mvn.h"      // mvn_corner_wave

// ------------------------------------------------------------------------------------------------
// per-sweep neighbour exchange between bond groups (lib/dmrgg.f90:763-958; the right-going block lost in
// the fp64 source is restated from lib/dmrggmp.f90:572-629).  Instead of propagating the 4-int pivot tape
// through every rank (which makes far bonds lag by one sweep per hop), the owner ships the FLATTENED
// multi-index of its new boundary pivot to its direct neighbour -- the only rank that ever evaluates with it.
// ------------------------------------------------------------------------------------------------
// The two outgoing messages of group g and its entry of the MAX all-reduce, each half called by every thread of a block.  The halves
// write disjoint memory and read nothing the other writes, so two blocks may run them side by side (the cluster kernel's exit,
// cl_pack_block of ttx_cluster_rules.h).  The flag, the ranks and the mode size of a half are requested together, ahead of the copies.
// right: red[] and the message to the right neighbour -- own last bond q = last, boundary core q+1
__device__ __forceinline__ void exch_pack_right(const DevProb &P, int g)
{
    const int tid = threadIdx.x, m = P.d;
    GroupState &gs = P.gs[g];
    const int first = gs.first, last = gs.last;
    const int *r = P.r + (size_t)g * (m + 2), *rr = P.rr + (size_t)g * (m + 2), *upd = P.upd + (size_t)g * (m + 2);
    if (tid == 0) {
        double *red = P.red + (size_t)g * 4;
        red[0] = gs.amax; red[1] = gs.pivotmax; red[2] = (gs.pivotmin > 0.0) ? -gs.pivotmin : -999e9;   // :853-859
    }
    const int q = last, u = upd[q], rq = r[q], rrq1 = rr[q + 1], n2 = P.n[q + 1];
    char *base = P.msgR + (size_t)g * P.MSZ;
    int *hh = (int *)base; int *ix = hh + XH; double *dd = (double *)(base + P.IOFF);
    if (tid == 0) { hh[0] = u; hh[1] = rq; }
    const double *gI = inv_ptr(P, g, q, first);
    for (int x = tid; x < rq * rq; x += blockDim.x) dd[(size_t)P.RM * P.NM + x] = gI[x];           // inv(q) for dtt_lua, :1225
    if (u) {
        const short *Lt = L_ptr(P, g, q, first);
        for (int x = tid; x < q; x += blockDim.x) ix[x] = Lt[(size_t)x * P.RM + (rq - 1)];
        // newest row of core q+1: arg(q+1)(r(q), :, 1:rr(q+1))  (dmrggmp.f90:580)
        const double *A = core_ptr(P, P.arg, g, q + 1, first);
        for (int x = tid; x < n2 * rrq1; x += blockDim.x) dd[x] = A[(rq - 1) + (size_t)P.RM * (x % n2) + P.SS * (x / n2)];
    }
}
// left: the message to the left neighbour -- own first bond q = first, boundary core q
__device__ __forceinline__ void exch_pack_left(const DevProb &P, int g)
{
    const int tid = threadIdx.x, m = P.d;
    const int first = P.gs[g].first;
    const int *r = P.r + (size_t)g * (m + 2), *rr = P.rr + (size_t)g * (m + 2), *upd = P.upd + (size_t)g * (m + 2);
    const int q = first, u = upd[q], rq = r[q], rr0 = rr[q - 1], n1 = P.n[q];
    char *base = P.msgL + (size_t)g * P.MSZ;
    int *hh = (int *)base; int *ix = hh + XH; double *dd = (double *)(base + P.IOFF);
    if (tid == 0) { hh[0] = u; hh[1] = rq; }
    if (u) {
        const short *Rt = R_ptr(P, g, q, first);
        for (int x = tid; x < m - q; x += blockDim.x) ix[x] = Rt[(size_t)x * P.RM + (rq - 1)];
        // newest column of core q: arg(q)(1:rr(q-1), :, r(q))  (dmrgg.f90:889)
        const double *A = core_ptr(P, P.arg, g, q, first);
        for (int x = tid; x < rr0 * n1; x += blockDim.x) dd[x] = A[(x % rr0) + (size_t)P.RM * (x / rr0) + P.SS * (rq - 1)];
    }
}
__device__ __forceinline__ void exch_pack_group(const DevProb &P, int g) { exch_pack_right(P, g); exch_pack_left(P, g); }

// MAX all-reduce (:861), stage 1: combine the groups of this GPU into redsend[0..2]
__global__ void k_exch_localmax(DevProb P)
{
    if (P.ctl[0]) return;
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double a = -1e300, b = -1e300, c = -1e300;
    for (int g = 0; g < P.G; g++) { a = fmax(a, P.red[4 * g]); b = fmax(b, P.red[4 * g + 1]); c = fmax(c, P.red[4 * g + 2]); }
    P.redsend[0] = a; P.redsend[1] = b; P.redsend[2] = c; P.redsend[3] = 0.0;
}
// apply the neighbours' pivots: ranks, index tables, inv of the left boundary bond (:822-850, :1209-1246)
__device__ __forceinline__ void exch_apply_group(const DevProb &P, int g)
{
    const int tid = threadIdx.x, m = P.d;
    GroupState &gs = P.gs[g];
    const int first = gs.first, last = gs.last;
    int *r = P.r + (size_t)g * (m + 2), *upd = P.upd + (size_t)g * (m + 2);
    if (P.inL[g]) {
        const int bl = first - 1;
        const int *hh = (const int *)P.inL[g], *ix = hh + XH; const double *dd = (const double *)(P.inL[g] + P.IOFF);
        const int u = hh[0], rnew = hh[1];
        if (u) { short *Lt = L_ptr(P, g, bl, first); for (int x = tid; x < bl; x += blockDim.x) Lt[(size_t)x * P.RM + (rnew - 1)] = (short)ix[x]; }
        double *gI = inv_ptr(P, g, bl, first);
        for (int x = tid; x < rnew * rnew; x += blockDim.x) gI[x] = dd[(size_t)P.RM * P.NM + x];
        if (tid == 0) { upd[bl] = u; r[bl] = rnew; }
        if (u && P.arith && P.fpersist && tid < 64) {        // fast tables: the neighbour's new pivot as a left multi-index of bond bl, from scratch
            extern __shared__ __align__(16) double dyn_x[];
            double *xs = dyn_x, *ws = xs + m + 8;
            if (P.fun_id == FUN_MVN) {
                for (int k = tid; k < bl; k += 64) xs[k] = P.par[ix[k] - 1] - P.aux[k];
                __builtin_amdgcn_wave_barrier();
                mvn_entry_scratch(P, xs, bl, 0, fast_dv(P, 0, g, bl, first) + (rnew - 1), fast_near(P, 0, g, bl, first) + (rnew - 1), fast_piv(P, 0, g, bl, first) + (rnew - 1), tid);
            } else {
            for (int k = tid; k < bl; k += 64) { xs[k] = P.par[ix[k] - 1]; ws[k] = P.par[P.n[1] + ix[k] - 1]; }
            __builtin_amdgcn_wave_barrier();
            fast_entry_scratch(xs, ws, bl, 0, fast_near(P, 0, g, bl, first) + (rnew - 1), fast_piv(P, 0, g, bl, first) + (rnew - 1), P.RM, tid);
            }
        }
    }
    if (P.inR[g]) {
        const int br = last + 1;
        const int *hh = (const int *)P.inR[g], *ix = hh + XH;
        const int u = hh[0], rnew = hh[1];
        if (u) { short *Rt = R_ptr(P, g, br, first); for (int x = tid; x < m - br; x += blockDim.x) Rt[(size_t)x * P.RM + (rnew - 1)] = (short)ix[x]; }
        if (tid == 0) { upd[br] = u; r[br] = rnew; }
        if (u && P.arith && P.fpersist && tid >= 64 && tid < 128) {   // ... and as a right multi-index of bond br
            extern __shared__ __align__(16) double dyn_x[];
            double *xs = dyn_x + 2 * (m + 8), *ws = xs + m + 8;
            const int lane_ = tid - 64;
            if (P.fun_id == FUN_MVN) {
                for (int k = lane_; k < m - br; k += 64) xs[k] = P.par[ix[k] - 1] - P.aux[br + k];
                __builtin_amdgcn_wave_barrier();
                mvn_entry_scratch(P, xs, m - br, br, fast_dv(P, 1, g, br, first) + (rnew - 1), fast_near(P, 1, g, br, first) + (rnew - 1), fast_piv(P, 1, g, br, first) + (rnew - 1), lane_);
            } else {
            for (int k = lane_; k < m - br; k += 64) { xs[k] = P.par[ix[k] - 1]; ws[k] = P.par[P.n[1] + ix[k] - 1]; }
            __builtin_amdgcn_wave_barrier();
            fast_entry_scratch(xs, ws, m - br, 1, fast_near(P, 1, g, br, first) + (rnew - 1), fast_piv(P, 1, g, br, first) + (rnew - 1), P.RM, lane_);
            }
        }
    }
}

// force: the finalisation's pack, which runs behind the stop flag without clearing it first
__global__ __launch_bounds__(256) void k_exch_pack(DevProb P, int force) { if (P.ctl[0] && !force) return; exch_pack_group(P, blockIdx.x); }
__global__ __launch_bounds__(256) void k_exch_apply(DevProb P) { exch_apply_group(P, blockIdx.x); }

// MAX all-reduce result (:867-870, :961) folded into the apply launch: every block reduces the same inputs and
// writes only its own group.  from_recv: P.redrecv already holds the job-wide maxima (after the RCCL all-reduce)
__device__ __forceinline__ void exch_max_group(const DevProb &P, int g, int from_recv)      // one thread of the group
{
    double a = -1e300, b = -1e300, c = -1e300;
    if (from_recv) { a = P.redrecv[0]; b = P.redrecv[1]; c = P.redrecv[2]; }
    else for (int x = 0; x < P.G; x++) { a = fmax(a, P.red[4 * x]); b = fmax(b, P.red[4 * x + 1]); c = fmax(c, P.red[4 * x + 2]); }
    GroupState &gs = P.gs[g];
    gs.amax = a; gs.pivotmax = b; gs.pivotmin = (-c == 999e9) ? -1.0 : -c;
    gs.pivotmax_prev = b;
}
__global__ __launch_bounds__(256) void k_exch_max_apply(DevProb P, int from_recv, int do_apply)
{
    if (P.ctl[0]) return;
    const int g = blockIdx.x;
    if (threadIdx.x == 0) exch_max_group(P, g, from_recv);
    if (do_apply) exch_apply_group(P, g);
}

// grow the boundary cores with the neighbours' fibers, evaluate the corner entries, LU-apply
// blocks [0,NM): "share blocks to the LEFT" receive side (:912-952), one mode index k each;
// blocks [NM,2NM): "share blocks to the RIGHT" receive side (dmrggmp.f90:598-627), one mode index j each
// One boundary block (bx, g), called by every thread of the workgroup.  MSG = false (k_exch_boundary): the launch behind
// k_exch_max_apply, which copied the neighbour's flag, rank and pivot index from the message into upd, r and the index tables.
// MSG = true (k_exch_tail): the apply block runs BESIDE this one, so nothing it writes may be read here -- the flag hh[0], the
// rank hh[1] and the dims beyond the bond ix[] come from the message itself (complete before the launch: the sweep kernel packs
// it at its end), the corner maximum goes to gs.amax_bnd[par] and the evaluation count is left to the apply block
// (boundary_neval).  What remains shared is read-only in the launch (own ranks, flags, tables, inv of the own bonds; the apply
// block writes column hh[1] - 1 of the tables of bonds first - 1 / last + 1, a corner reads columns of older pivots there).
template <int FUN, bool MSG>
__device__ __forceinline__ void exch_boundary_block(const DevProb &P, int bx, int g, int par_, int lean)
{
    extern __shared__ __align__(16) double dyn[];
    __shared__ double s_bc;
    const int tid = threadIdx.x, m = P.d;
    GroupState &gs = P.gs[g];
    double *amax_to = MSG ? &gs.amax_bnd[par_] : &gs.amax;
    const int first = gs.first, last = gs.last;
    const int *r = P.r + (size_t)g * (m + 2), *rr = P.rr + (size_t)g * (m + 2), *upd = P.upd + (size_t)g * (m + 2);
    double *par = dyn;
    // corner evaluation: the multi-index as two 16-byte aligned, padded rows (dims 1..p-1 | dims p+1..m) around dim p,
    // the layout the fast chunked evaluators read
    const int VSr = ((m + 7) & ~7) + 8;
    short *rowA = (short *)(((size_t)(dyn + P.npar) + 15) & ~(size_t)15), *rowB = rowA + VSr;
    double *lu = (double *)(rowB + VSr);                  // packed LU of the boundary bond (ranks <= 64)
    double *wscr = lu + 64 * 64 + 4;                      // scratch of the one-element-per-wave evaluator (Ising D/E, P.bnd_wave)
    __shared__ double s_corner;
    const bool dewave = (FUN == FUN_ISING) && P.ising_id != 1 && P.bnd_wave;
    const bool mvwave = (FUN == FUN_MVN) && P.bnd_wave;
    // lean (TTX_TAIL_LEAN, profiles/sweep_gap_mi355x.txt): the words a block decides on -- the message's address, then its header, the
    // own ranks, flag and mode size -- are requested together, each batch one round trip, from addresses that are valid whatever the
    // decisions turn out to be; a block that returns early still returns before it writes anything.  And the corner of Ising C is
    // evaluated as in the cluster kernel: all threads stage the node and weight VALUES of the multi-index (in the region of lu, which
    // is staged behind the evaluation), and the one thread runs the same chains over them (f_ising_c3v: the operations of
    // f_ising_c3 in its order) without an index and a table lookup in front of every step.
    const char *in_r = nullptr, *in_l = nullptr;
    if (lean) { in_r = P.inR[g]; in_l = P.inL[g]; }
    const bool cval = (FUN == FUN_ISING) && lean && P.ising_id == 1 && 4 * VSr <= 64 * 64;
    double *cAn = lu, *cAw = cAn + VSr, *cBn = cAw + VSr, *cBw = cBn + VSr;
    const double *gnodes = P.par - 1, *gweights = gnodes + (cval ? P.n[1] : 0);       // node / weight of index i: gnodes[i], gweights[i]
    if (bx < P.NM) {
        const int k = bx, p = last, br = last + 1;
        const char *in = lean ? in_r : P.inR[g];
        const int *hh = (const int *)in, *ix = hh + XH;               // the message's header and flattened pivot index (dims br+1..m)
        int rp, rrp, snew, n2, up = 0;
        if (lean) {
            const int *hq = in ? hh : &gs.first;                      // no message: two ints that are there
            const int u_in = MSG ? hq[0] : upd[br];
            rp = r[p]; rrp = rr[p]; snew = (MSG ? hq[1] : r[br]) - 1; n2 = P.n[br]; up = upd[p];
            asm volatile("" ::: "memory");                            // the requests stay in front of the decisions
            if (!in || !u_in || k >= n2) return;
        } else {
            if (!in) return;
            if (!(MSG ? hh[0] : upd[br]) || k >= P.n[br]) return;
            rp = r[p]; rrp = rr[p]; snew = (MSG ? hh[1] : r[br]) - 1; n2 = P.n[br];
        }
        const double *msg = (const double *)(in + P.IOFF);            // (rr(p), n(p+1))
        double *A = core_ptr(P, P.arg, g, br, first), *W = core_ptr(P, P.row, g, br, first);
        double a = 0.0;
        if (tid < rrp) a = msg[tid + (size_t)rrp * k];
        if (!lean) up = upd[p];
        if (up) {                                                    // corner arg(p+1)(r(p), k, r(p+1)), :925-937
            const int *vp = vip_ptr(P, g, p, first) + 4 * (rp - 1);
            const short *Lt = L_ptr(P, g, p - 1, first), *Rt = R_ptr(P, g, br, first);
            auto dimv = [&](int s) -> short { return (s < p) ? Lt[(size_t)(s - 1) * P.RM + (vp[0] - 1)] : (s == p) ? (short)vp[1] : (s == p + 1) ? (short)(k + 1) : MSG ? (short)ix[s - p - 2] : Rt[(size_t)(s - p - 2) * P.RM + snew]; };
            if (cval) {
                for (int x = tid; x < VSr; x += TTX_BLK) {
                    const int ia = (x < p - 1) ? dimv(x + 1) : 0, ib = (x < m - p) ? dimv(p + 1 + x) : 0;
                    cAn[x] = ia ? gnodes[ia] : 0.0; cAw[x] = ia ? gweights[ia] : 0.0; cBn[x] = ib ? gnodes[ib] : 0.0; cBw[x] = ib ? gweights[ib] : 0.0;
                }
            } else {
                for (int x = tid; x < P.npar; x += TTX_BLK) par[x] = P.par[x];
                for (int x = tid; x < VSr; x += TTX_BLK) { rowA[x] = (x < p - 1) ? dimv(x + 1) : (short)1; rowB[x] = (x < m - p) ? dimv(p + 1 + x) : (short)1; }
            }
            __syncthreads();
            if (dewave || mvwave) {
                if (tid < 64) {
                    const double c_ = dewave ? de_corner_wave(P, par, rowA, p, (int)vp[1], rowB, wscr, tid) : mvn_corner_wave(P, par, rowA, p, (int)vp[1], rowB, wscr, tid);
                    if (tid == 0) s_corner = c_;
                }
                __syncthreads();
            }
            if (tid == rrp) {
                Src3 sx{rowA, p - 1, (int)vp[1], rowB};
                if (cval) a = f_ising_c3v(m, p - 1, cAn, cAw, gnodes[vp[1]], gweights[vp[1]], cBn, cBw);
                else a = (dewave || mvwave) ? s_corner : eval_src3<FUN, true>(P, par, sx, (long)g * P.HS + k);
                if (!HOST_PASS1(FUN, P)) {
                    atomic_max_pos(amax_to, fabs(a));
                    if (!MSG && k == 0) atomicAdd((unsigned long long *)&gs.neval, (unsigned long long)n2);   // :936
                }
            }
        }
        if (HOST_PASS1(FUN, P)) return;
        if (tid < rp) A[tid + (size_t)P.RM * k + P.SS * snew] = a;
        // row(p+1)(:, k, new) = L(p)^-1 * column : d2_luar(n(p+1), r(p), inv(p), .) :940-951
        const double *gI = inv_ptr(P, g, p, first);
        double tmp = 0.0, xf = 0.0;
        if (rp <= 64) {                               // one wave: the solve runs as a lane-read wavefront over LDS-staged LU
            __syncthreads();
            for (int x = tid; x < rp * rp; x += TTX_BLK) lu[x] = gI[x];
            __syncthreads();
            if (tid < 64) xf = dev_solve_L<1>(lu, rp, a, tid, 0);
        } else
        for (int s = 0; s < rp; s++) {
            if (tid == s) { xf = (s == 0) ? a : a + (-1.0) * tmp; s_bc = xf; }
            __syncthreads();
            if (tid > s && tid < rp) tmp = tmp + s_bc * gI[tid * tid + s];
            __syncthreads();
        }
        if (tid < rp) W[k + (size_t)P.NM * snew + P.SW * tid] = xf;
    } else {
        const int j = bx - P.NM, p = first, bl = first - 1;
        const char *in = lean ? in_l : P.inL[g];
        const int *hh = (const int *)in, *ix = hh + XH;               // ... dims 1..bl
        int rp, rrp, inew, n1, up = 0;
        if (lean) {
            const int *hq = in ? hh : &gs.first;
            const int u_in = MSG ? hq[0] : upd[bl];
            rp = r[p]; rrp = rr[p]; inew = (MSG ? hq[1] : r[bl]) - 1; n1 = P.n[p]; up = upd[p];
            asm volatile("" ::: "memory");
            if (!in || !u_in || j >= n1) return;
        } else {
            if (!in) return;
            if (!(MSG ? hh[0] : upd[bl]) || j >= P.n[p]) return;
            rp = r[p]; rrp = rr[p]; inew = (MSG ? hh[1] : r[bl]) - 1; n1 = P.n[p];
        }
        const double *msg = (const double *)(in + P.IOFF);            // (n(p), rr(p))
        double *A = core_ptr(P, P.arg, g, p, first), *C = core_ptr(P, P.col, g, p, first);
        double y = 0.0;
        if (tid < rrp) y = msg[j + (size_t)n1 * tid];
        if (!lean) up = upd[p];
        if (up) {                                                    // corner arg(p)(r(p-1), j, r(p)), dmrggmp.f90:608-616
            const int *vp = vip_ptr(P, g, p, first) + 4 * (rp - 1);
            const short *Lt = L_ptr(P, g, bl, first), *Rt = R_ptr(P, g, p + 1, first);
            auto dimv = [&](int s) -> short { return (s < p) ? (MSG ? (short)ix[s - 1] : Lt[(size_t)(s - 1) * P.RM + inew]) : (s == p) ? (short)(j + 1) : (s == p + 1) ? (short)vp[2] : Rt[(size_t)(s - p - 2) * P.RM + (vp[3] - 1)]; };
            if (cval) {
                for (int x = tid; x < VSr; x += TTX_BLK) {
                    const int ia = (x < p - 1) ? dimv(x + 1) : 0, ib = (x < m - p) ? dimv(p + 1 + x) : 0;
                    cAn[x] = ia ? gnodes[ia] : 0.0; cAw[x] = ia ? gweights[ia] : 0.0; cBn[x] = ib ? gnodes[ib] : 0.0; cBw[x] = ib ? gweights[ib] : 0.0;
                }
            } else {
                for (int x = tid; x < P.npar; x += TTX_BLK) par[x] = P.par[x];
                for (int x = tid; x < VSr; x += TTX_BLK) { rowA[x] = (x < p - 1) ? dimv(x + 1) : (short)1; rowB[x] = (x < m - p) ? dimv(p + 1 + x) : (short)1; }
            }
            __syncthreads();
            if (dewave || mvwave) {
                if (tid < 64) {
                    const double c_ = dewave ? de_corner_wave(P, par, rowA, p, j + 1, rowB, wscr, tid) : mvn_corner_wave(P, par, rowA, p, j + 1, rowB, wscr, tid);
                    if (tid == 0) s_corner = c_;
                }
                __syncthreads();
            }
            if (tid == rrp) {
                Src3 sx{rowA, p - 1, j + 1, rowB};
                if (cval) y = f_ising_c3v(m, p - 1, cAn, cAw, gnodes[j + 1], gweights[j + 1], cBn, cBw);
                else y = (dewave || mvwave) ? s_corner : eval_src3<FUN, true>(P, par, sx, (long)g * P.HS + P.NM + j);
                if (!HOST_PASS1(FUN, P)) {
                    atomic_max_pos(amax_to, fabs(y));
                    if (!MSG && j == 0) atomicAdd((unsigned long long *)&gs.neval, (unsigned long long)n1);
                }
            }
        }
        if (HOST_PASS1(FUN, P)) return;
        if (tid < rp) A[inew + (size_t)P.RM * j + P.SS * tid] = y;
        // col(p)(new, j, :) = row * U(p)^-1 : d2_lual(n(p), r(p), inv(p), .) dmrggmp.f90:622
        const double *gI = inv_ptr(P, g, p, first);
        if (rp <= 64) {
            __syncthreads();
            for (int x = tid; x < rp * rp; x += TTX_BLK) lu[x] = gI[x];
            __syncthreads();
            if (tid < 64) y = dev_solve_U<1>(lu, rp, y, dev_solve_rdg(lu, rp, tid), tid, 0);
        } else
        for (int s = 0; s < rp; s++) {
            if (tid == s) { y = (1.0 / gI[(s + 1) * (s + 1) - 1]) * y; s_bc = y; }
            __syncthreads();
            if (tid > s && tid < rp) y = y + (-gI[tid * tid + tid + s]) * s_bc;
            __syncthreads();
        }
        if (tid < rp) C[inew + (size_t)P.RM * j + P.SS * tid] = y;
    }
}
template <int FUN>
__global__ __launch_bounds__(TTX_BLK) void k_exch_boundary(DevProb P, int lean)
{
    if (P.ctl[0]) return;
    exch_boundary_block<FUN, false>(P, (int)blockIdx.x, (int)blockIdx.y, 0, lean);
}
// MAX / apply and the boundary blocks of sweep `it` in ONE launch (single process, device integrand): grid (2 NM + 1, G), blocks
// x < 2 NM are the boundary blocks, block x = 2 NM is the group's apply block.  The blocks are independent: no block reads what
// another one of the launch writes (exch_boundary_block), and nothing is counted, fenced or waited for.
template <int FUN>
__global__ __launch_bounds__(TTX_BLK) void k_exch_tail(DevProb P, int it, int lean)
{
    if (P.ctl[0]) return;
    const int g = blockIdx.y;
    if ((int)blockIdx.x < 2 * P.NM) { exch_boundary_block<FUN, true>(P, (int)blockIdx.x, g, it & 1, lean); return; }
    if (threadIdx.x == 0) {
        exch_max_group(P, g, 0);
        GroupState &gs = P.gs[g];
        const int *upd = P.upd + (size_t)g * (P.d + 2);
        const int u_r = P.inR[g] ? ((const int *)P.inR[g])[0] : 0, u_l = P.inL[g] ? ((const int *)P.inL[g])[0] : 0;
        gs.neval += boundary_neval(P.inR[g] != nullptr, u_r, upd[gs.last], P.n[gs.last + 1], P.inL[g] != nullptr, u_l, upd[gs.first], P.n[gs.first]);
    }
    exch_apply_group(P, g);
    if (!P.tail_side) return;
    // the group's records of this sweep for the side stream and the next sweep kernel's entry (ttx_dev.h); the ranks behind the apply
    __syncthreads();
    const int m = P.d, tid = threadIdx.x, par = it & 1;
    const GroupState &gs = P.gs[g];
    const int *r = P.r + (size_t)g * (m + 2), *tp = P.tape + (size_t)g * (m + 2) * 4;
    int *rq = P.rq + (size_t)g * (m + 2), *tq = P.tail_tape + ((size_t)par * P.G + g) * (m + 2) * 4;
    for (int x = tid; x < m + 2; x += blockDim.x) rq[x] = r[x];
    for (int x = 4 * gs.first + tid; x < 4 * (gs.last + 1); x += blockDim.x) tq[x] = tp[x];
    if (tid == 0) {
        TailRec t;
        t.amax = gs.amax; t.pivotmax = gs.pivotmax; t.pivotmin = gs.pivotmin; t.bytes_half = gs.bytes_half; t.initval = gs.initval;
        t.neval = gs.neval; t.n_resid = gs.n_resid;
        P.tailrec[(size_t)par * P.G + g] = t;
    }
}
