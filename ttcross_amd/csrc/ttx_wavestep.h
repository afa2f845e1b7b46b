// ttx_wavestep.h -- the frame of a wave half-step, once.
//
// Five of the six chain half-step kernels run one wave per (varying pivot, 64-mode chunk) slot of the fiber: k_halfstep_de,
// _dec, _de5, _det (ttx_de.h) and k_halfstep_mvn (ttx_mvn.h); de5 and det add helper waves, the slot is still one wave's.  They
// differ in how the value of a fiber element is evaluated and in nothing around it.  What is around it lives here, for the four
// Ising kernels; k_halfstep_mvn keeps the second and last copy of slot and finish in its own text (measured: every shared form
// cost it time, see the comment there), so a change to wave_slot or wave_finish is made there too:
//   WaveSlot / wave_slot   which slot a workgroup has and what it steers by, from the LDS-resident StepState behind the barrier;
//   wave_finish            fiber store, amax, residual in the reference's two dgemv orders, arg-max and the Partial record;
//   de_finish_split        Ising D/E: the id-2 b-part and the weights with dims p and p+1 split out of the pivots' rows;
//   stage_pivot_rows       Ising D/E: the pivots' node and weight rows from the index tables into LDS.
// The kernels keep, in their own text: the thread-0 load with resolve_state, the barrier, the inactive-or-done exit, the publish by
// slot 0 and the exit of a slot past the fiber (k_halfstep_det's fault count ahead of them), and the evaluation.
//
// A header of its own rather than a section of ttx_bondstep.h: that one is rules and cold code, this one is a kernel's frame on
// top of the reductions of ttx_wave.h and resolve_state of ttx_kernels.h.
// k_halfstep (a block per 256 entries), k_sweep_fused and k_sweep_cluster reduce differently and are not served.
#pragma once
#include "ttx_kernels.h"

struct WaveSlot {
    bool iscol, resid; RookTurn turn;                      // :517,550 / :534,567
    int p, r0, r1, r2, n1, n2, first, ii, jj, kk, qq;      // the bond's state; the pivot 1-based, reference names
    int nf, nch, npart;                                    // fiber entries, chunks of 64 modes per pivot, slots of the half-step
    int w, pv, vmode; bool live;                           // this slot, its varying pivot, this lane's mode index (0-based) and whether the fiber has it
    int pl, qr, i1, i2;                                    // left / right pivot of the wave, node index of dim p / p+1 (0-based)
};

// What steers the control flow is made wave-uniform explicitly (values read from LDS / global memory are per-lane registers to the
// compiler: loop counters and branches would otherwise run on the vector unit).  All lanes of the wave call it, behind the barrier
// that follows thread 0's write of cur.
__device__ __forceinline__ WaveSlot wave_slot(const DevProb &P, const GroupState &gs, const StepState &cur, int h, int dir, int mode, int lane)
{
    WaveSlot s;
    s.turn = rook_turn(P.piv, mode, h, dir, UNI(cur.crs), UNI(cur.havecol), UNI(cur.haverow));
    s.iscol = s.turn.iscol; s.resid = s.turn.resid;
    s.p = UNI(cur.p); s.r0 = UNI(cur.r0); s.r1 = UNI(cur.r1); s.r2 = UNI(cur.r2);
    s.n1 = UNI(cur.n1); s.n2 = UNI(cur.n2); s.first = UNI(gs.first);
    s.ii = UNI(cur.ii); s.jj = UNI(cur.jj); s.kk = UNI(cur.kk); s.qq = UNI(cur.qq);
    s.nf = s.iscol ? s.r0 * s.n1 : s.n2 * s.r2;
    const int nv = s.iscol ? s.r0 : s.r2, nm = s.iscol ? s.n1 : s.n2;
    s.nch = (nm + 63) >> 6;
    s.npart = nv * s.nch;
    s.w = blockIdx.x;
    s.pv = s.w / s.nch; s.vmode = (s.w - s.pv * s.nch) * 64 + lane;
    s.live = s.vmode < nm;
    s.pl = s.iscol ? s.pv : s.ii - 1; s.qr = s.iscol ? s.qq - 1 : s.pv;
    s.i1 = s.iscol ? (s.live ? s.vmode : 0) : s.jj - 1; s.i2 = s.iscol ? s.kk - 1 : (s.live ? s.vmode : 0);
    return s;
}

// The value a of this lane's fiber element is in: fiber store, amax, residual, arg-max, as k_halfstep, on the fiber's linear index
// t.  All 64 lanes of the slot's wave call it; lane 0 writes the Partial record of slot w.
__device__ __forceinline__ void wave_finish(const DevProb &P, GroupState &gs, int g, const WaveSlot &s, int h, int mode, double a, int lane)
{
    const int u_ = s.iscol ? s.pv : s.vmode, v_ = s.iscol ? s.vmode : s.pv;        // col: (i, j) ; row: (k, q), 0-based
    const int t = s.iscol ? (u_ + s.r0 * v_) : (u_ + s.n2 * v_);
    if (s.live) (s.iscol ? P.acol : P.arow)[(size_t)g * P.RM * P.NM + t] = a;
    const double mx = wave_max(s.live ? fabs(a) : 0.0);
    if (lane == 0 && mode != 1) atomic_max_pos(&gs.amax, mx);          // :531 / :564 (the piv = 0 branch :492-513 does not touch amax)
    if (!s.resid) return;
    const double *Cp = core_ptr(P, P.col, g, s.p, s.first), *Wq = core_ptr(P, P.row, g, s.p + 1, s.first);
    double bb = a, ab = -1.0; int bi = INT_MAX;                        // no live lane, or every residual a NaN: bi stays INT_MAX (take_pivot)
    if (s.live) {
        if (s.iscol) {   // dgemv 'n', alpha=-1 (:538): b += (-x_s) * col(:, s), x_s = row(p+1)(s, kk, qq)
            const double *c = Cp + u_ + (size_t)P.RM * v_;
            const double *xq = Wq + (s.kk - 1) + (size_t)P.NM * (s.qq - 1);
#pragma unroll 8
            for (int x = 0; x < s.r1; x++) bb = bb + (-xq[P.SW * x]) * c[P.SS * x];
        } else {         // dgemv 't', alpha=-1 (:571): b += -1 * sum_s row(s, kq) * x_s, x_s = col(p)(ii, jj, s)
            const double *wv = Wq + u_ + (size_t)P.NM * v_;
            const double *xc = Cp + (s.ii - 1) + (size_t)P.RM * (s.jj - 1);
            double tt = 0.0;
#pragma unroll 8
            for (int x = 0; x < s.r1; x++) tt = tt + wv[P.SW * x] * xc[P.SS * x];
            bb = bb + (-1.0) * tt;
        }
        ab = fabs(bb); bi = t;
    }
    wave_argmax(ab, bb, bi);
    if (lane == 0) { Partial pr; pr.absmax = ab; pr.val = bb; pr.idx = bi; pr.pad = 0; gs.Pt[h & 1][s.w] = pr; }
}

// Ising D/E: b-part (id 2) and the weights (test_crs_ising.f90:197-218), order of de_finish, from the pair product a.  Dims p and
// p+1 come as x1, x2, w1, w2 (per lane), the A dims left and the B dims right of them as the pivots' rows xl, wl, xr, wr.
__device__ __forceinline__ double de_finish_split(int id, double a, int A, int B, double x1, double x2, double w1, double w2,
                                                  const double *xl, const double *wl, const double *xr, const double *wr)
{
    double b = 0.0;
    if (id == 2) {
        double v = 1.0, ww = 1.0, vk = 1.0, wk = 1.0;
        for (int j = B - 1; j >= 0; j--) { vk = vk * xr[j]; v = v + vk; }
        vk = vk * x2; v = v + vk;
        vk = vk * x1; v = v + vk;
        for (int j = A - 1; j >= 0; j--) { vk = vk * xl[j]; v = v + vk; }
        for (int j = 0; j < A; j++) { wk = wk * xl[j]; ww = ww + wk; }
        wk = wk * x1; ww = ww + wk;
        wk = wk * x2; ww = ww + wk;
        for (int j = 0; j < B; j++) { wk = wk * xr[j]; ww = ww + wk; }
        b = 1.0 / (v * ww);
    }
    double f = (id == 2) ? 2 * a * b : 2 * a;
    for (int j = 0; j < A; j++) f = f * wl[j];
    f = f * w1; f = f * w2;
    for (int j = 0; j < B; j++) f = f * wr[j];
    return f;
}

// Ising D/E: node and weight of the A dims of left pivot pl (rows of Lt) and of the B dims of right pivot qr (rows of Rt) into
// xl, wl / xr, wr; threads tid, tid + nthreads, ...
__device__ __forceinline__ void stage_pivot_rows(const DevProb &P, const short *Lt, const short *Rt, int pl, int qr, int A, int B, int tid, int nthreads,
                                                 const double *nodes, const double *weights, double *xl, double *wl, double *xr, double *wr)
{
    for (int x = tid; x < A; x += nthreads) { const int ix = Lt[(size_t)x * P.RM + pl] - 1; xl[x] = nodes[ix]; wl[x] = weights[ix]; }
    for (int x = tid; x < B; x += nthreads) { const int ix = Rt[(size_t)x * P.RM + qr] - 1; xr[x] = nodes[ix]; wr[x] = weights[ix]; }
}
