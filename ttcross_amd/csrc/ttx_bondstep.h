// ttx_bondstep.h -- the rules of one bond step of the cross sweep (lib/dmrgg.f90:410-758), once.
//
// Eight kernels run a bond step: the chain half-steps (k_halfstep, k_halfstep_de, _dec, _de5, _det, _mvn) with k_lottery /
// k_accept / k_exch_boundary around them, and the two whole-sweep kernels (k_sweep_fused, k_sweep_cluster).  What they
// must agree on lives here: whose turn it is and when the rook search stops, how a pivot is taken from an arg-max, the
// acceptance test and the pivot range, the traffic count, and the cold device code around them (publishing the next
// step state, the lottery's zero-weight lists, the two triangular wave solves of the append, the tables and scalars
// of an accepted pivot, the start of a sweep).  The kernels keep their evaluation, reduction and exchange -- except the four
// Ising half-steps with one wave per (pivot, 64-mode chunk) slot (_de, _dec, _de5, _det), which keep the evaluation only: their
// slot, reduction and Partial record are ttx_wavestep.h, on top of this file and ttx_kernels.h (_mvn, the fifth of that kind,
// keeps a copy of that frame: measured, see ttx_mvn.h).
//
// The rule part is plain functions of values and compiles on the host (tests/bondstep_main.cpp); values that must be
// wave-uniform are made so by the caller.  The device part follows behind __HIPCC__.
#pragma once
#include <limits.h>
#include <math.h>
#include "ttx_cdf.h"     // TTX_HD
#include "ttx_wave_solve.h"   // the two triangular wave solves of the append (host + device)

// ------------------------------------------------------------------------------------------------
// rule part (host + device)
// ------------------------------------------------------------------------------------------------
// One turn of the rook search (:516-582) or of the piv = 0 branch (:492-513).  mode 0: rook -- the type alternates,
// a left-going step (dir 2) begins with the row, and the search stops once both types were seen and 2*piv fibers
// were evaluated; a residual is taken unless the turn stops.  mode 1 / 2: piv = 0 -- h = 0 column, h = 1 row, then
// stop, no residual (mode 2 differs from 1 only in what halfstep_publish counts).  Any other mode (k_halfstep's full
// pivoting, 3 and 4) gets resid = false and nothing else of use: that caller sets type and residual itself and
// returns before the turn is published.
struct RookTurn { bool iscol, resid; int crs, havecol, haverow, done; };
TTX_HD bool rook_iscol(int mode, int h, int dir)
{ return (mode == 1 || mode == 2) ? (h == 0) : (((h + (dir == 2 ? 1 : 0)) & 1) == 0); }    // :517,550
TTX_HD RookTurn rook_turn(int piv, int mode, int h, int dir, int crs, int havecol, int haverow)
{
    const bool iscol = rook_iscol(mode, h, dir);
    crs = crs + 1;
    havecol = havecol | (iscol ? 1 : 0); haverow = haverow | (iscol ? 0 : 1);
    const int done = (mode == 1 || mode == 2) ? (h == 1) : (havecol && haverow && (crs >= 2 * piv));   // :534 / :567
    const bool resid = (mode == 0) && !done;
    return RookTurn{iscol, resid, crs, havecol, haverow, done};
}

// algorithmic traffic of a half-step over nf fiber entries at rank r1: factor slabs + vector + fiber in/out when a
// residual is taken, else the fiber
TTX_HD double halfstep_traffic(int nf, int r1, bool resid)
{ return resid ? 8.0 * ((double)nf * r1 + r1 + 2.0 * nf) : 8.0 * nf; }

// The next pivot from the arg-max position ix of a residual fiber (:540-546 column, :573-579 row): the pair on the
// fiber's side is replaced, the other stays.  Returns done: both types seen and the same pivot again.  ix = INT_MAX
// means nothing compared (every residual a NaN): the first position, as idamax returns (no wild index).
TTX_HD int take_pivot(bool iscol, int ix, int r0, int n2, int havecol, int haverow, int &ii, int &jj, int &kk, int &qq)
{
    if (ix == INT_MAX) ix = 0;
    int done;
    if (iscol) { const int i = ix % r0 + 1, j = ix / r0 + 1; done = havecol && haverow && (i == ii && j == jj); ii = i; jj = j; }
    else       { const int k = ix % n2 + 1, q = ix / n2 + 1; done = havecol && haverow && (k == kk && q == qq); kk = k; qq = q; }
    return done;
}

// acceptance test of the new cross (:599-600); strict on both sides, so a NaN pivot is refused
TTX_HD bool accept_pivot(double pivot, double amax, double pivotmax_prev, double small_element, double small_pivot)
{ return (fabs(pivot) > small_element * amax) && (fabs(pivot) > small_pivot * pivotmax_prev); }

// pivot range of the sweep; negative = no pivot accepted yet
TTX_HD void pivot_range(double &pivotmax, double &pivotmin, double ap)
{
    pivotmax = (pivotmax < 0.0) ? ap : fmax(pivotmax, ap);
    pivotmin = (pivotmin < 0.0) ? ap : fmin(pivotmin, ap);
}

// The stopping rule at the end of sweep it (:1011-1019): the rank limit, or -- with accuracy >= 0 -- the third sweep in a row
// whose largest pivot is at most accuracy * amax (a comparison with a NaN is false: such a sweep resets the strikes).  One
// function for the device (k_sweep_end) and the host (process_sweep of run_impl), which must decide alike.
struct StopRule { int ready, strikes; };
TTX_HD StopRule stop_rule(int it, int maxrank, double accuracy, double pmax, double amax, int strikes_prev)
{
    StopRule s{(it + 1 >= maxrank) ? 1 : 0, strikes_prev};
    if (accuracy >= 0.0) {
        s.strikes = (pmax <= accuracy * amax) ? strikes_prev + 1 : 0;
        s.ready = (s.ready || s.strikes >= 3) ? 1 : 0;
    }
    return s;
}

// Evaluations the boundary step of a sweep counts for one group (:936 and its right-going twin): n(last+1) where the right
// neighbour sent a pivot (u_r) and the own last bond took one this sweep (upd_last), n(first) likewise on the left.  These are the
// conditions under which corner block 0 of either side of k_exch_boundary adds them; the apply block of k_exch_tail adds the sum.
TTX_HD long long boundary_neval(bool has_r, int u_r, int upd_last, int n_r, bool has_l, int u_l, int upd_first, int n_l)
{ return ((has_r && u_r && upd_last) ? (long long)n_r : 0) + ((has_l && u_l && upd_first) ? (long long)n_l : 0); }

#if defined(__HIPCC__)
// ------------------------------------------------------------------------------------------------
// device part.  UNI stays defined for every header that includes this one.
// ------------------------------------------------------------------------------------------------
#include "ttx_addr.h"
#define UNI(x) __builtin_amdgcn_readfirstlane(x)

// sweep start (:325-327); one thread of the group
__device__ __forceinline__ void sweep_start(const DevProb &P, int g)
{
    GroupState &gs = P.gs[g];
    gs.pivotmax = -1.0; gs.pivotmin = -1.0;
    const int *r = P.r + (size_t)g * (P.d + 2);
    int *rr = P.rr + (size_t)g * (P.d + 2);
    for (int s = 0; s <= P.d; s++) rr[s] = r[s];
}

// a chain half-step hands the state to the next launch and counts its work; one thread of the group
__device__ __forceinline__ void halfstep_publish(GroupState &gs, int h, const StepState &cur, const RookTurn &t, int mode, int nf, int r1, int npart)
{
    StepState nx = cur;
    nx.crs = t.crs; nx.havecol = t.havecol; nx.haverow = t.haverow; nx.done = t.done;
    nx.pending = t.resid ? (t.iscol ? 1 : 2) : 0;
    nx.npart = npart;
    gs.S[h + 1] = nx;
    if (mode != 2) gs.neval += nf;                                        // :527 / :560 / :509
    gs.bytes_half += halfstep_traffic(nf, r1, t.resid);
    gs.n_resid += t.resid ? 1 : 0;
}

// Zero-weight positions of the lottery (:432-439): the flattened column / row positions of the r1 pivots of the bond
// (vp: its pivot set), sorted and distinct, into zc[0..nzc) / zr[0..nzr).  Called by the whole workgroup (at least r1
// threads); zcs..keepr hold r1 ints each; complete behind the last of its four barriers.
__device__ __forceinline__ void bond_zero_lists(const int *vp, int r1, int r0, int n2, int tid, int *zc, int *zr, int *zcs, int *zrs,
                                                int *keepc, int *keepr, int *nzc, int *nzr)
{
    if (tid < r1) {
        zc[tid] = (vp[4 * tid + 0] - 1) + r0 * (vp[4 * tid + 1] - 1) + 1;
        zr[tid] = (vp[4 * tid + 2] - 1) + n2 * (vp[4 * tid + 3] - 1) + 1;
    }
    __syncthreads();
    if (tid < r1) {          // rank sort (total order with index tie-break)
        int a = zc[tid], b = zr[tid], ra = 0, rb = 0;
        for (int u = 0; u < r1; u++) {
            ra += (zc[u] < a) || (zc[u] == a && u < tid);
            rb += (zr[u] < b) || (zr[u] == b && u < tid);
        }
        zcs[ra] = a; zrs[rb] = b;
    }
    __syncthreads();
    if (tid < r1) { keepc[tid] = (tid == 0) || (zcs[tid] != zcs[tid - 1]); keepr[tid] = (tid == 0) || (zrs[tid] != zrs[tid - 1]); }
    __syncthreads();
    if (tid < r1) {          // compaction of distinct values into zc / zr
        int pc = 0, pr = 0;
        for (int u = 0; u < tid; u++) { pc += keepc[u]; pr += keepr[u]; }
        if (keepc[tid]) zc[pc] = zcs[tid];
        if (keepr[tid]) zr[pr] = zrs[tid];
        if (tid == r1 - 1) { *nzc = pc + keepc[tid]; *nzr = pr + keepr[tid]; }
    }
    __syncthreads();
}

// The two triangular solves of the append along the rank index (roles C and D: dev_solve_L, dev_solve_rdg, dev_solve_U) are
// ttx_wave_solve.h, included above: the value of lane s by lane reads instead of a shuffle, the LU entries requested ahead of
// their step, the update by a select -- checked on the host by tests/wave_solve_main.cpp.

// role E of an accepted pivot (ii, jj, kk, qq: 1-based) at bond p of rank r1 (:604-635).
// index tables of the new pivot (replaces the vip walk of :1062-1075); threads tid, tid + nthr, ...
__device__ __forceinline__ void append_tables(const DevProb &P, int g, int p, int first, int r1, int ii, int jj, int kk, int qq, int tid, int nthr)
{
    short *Ln = L_ptr(P, g, p, first), *Rn = R_ptr(P, g, p, first);
    const short *Lo = L_ptr(P, g, p - 1, first), *Ro = R_ptr(P, g, p + 1, first);
    for (int x = tid; x < p; x += nthr) Ln[(size_t)x * P.RM + r1] = (x < p - 1) ? Lo[(size_t)x * P.RM + (ii - 1)] : (short)jj;
    for (int x = tid; x < P.d - p; x += nthr) Rn[(size_t)x * P.RM + r1] = (x == 0) ? (short)kk : Ro[(size_t)(x - 1) * P.RM + (qq - 1)];
}
// The same in two parts (k_sweep_cluster): thread tid requests its entry of either table (x = tid) ahead of the work that does not
// need it, and stores it later; entries beyond the first nthr (d > nthr) are copied at the store as above.
struct AppendTab { short l, r; };
__device__ __forceinline__ AppendTab append_tables_fetch(const DevProb &P, int g, int p, int first, int ii, int qq, int tid)
{
    const short *Lo = L_ptr(P, g, p - 1, first), *Ro = R_ptr(P, g, p + 1, first);
    AppendTab t{0, 0};
    if (tid < p - 1) t.l = Lo[(size_t)tid * P.RM + (ii - 1)];
    if (tid >= 1 && tid < P.d - p) t.r = Ro[(size_t)(tid - 1) * P.RM + (qq - 1)];
    return t;
}
__device__ __forceinline__ void append_tables_store(const DevProb &P, int g, int p, int first, int r1, int ii, int jj, int kk, int qq, int tid, int nthr, AppendTab t)
{
    short *Ln = L_ptr(P, g, p, first), *Rn = R_ptr(P, g, p, first);
    const short *Lo = L_ptr(P, g, p - 1, first), *Ro = R_ptr(P, g, p + 1, first);
    if (tid < p) Ln[(size_t)tid * P.RM + r1] = (tid < p - 1) ? t.l : (short)jj;
    if (tid < P.d - p) Rn[(size_t)tid * P.RM + r1] = (tid == 0) ? (short)kk : t.r;
    for (int x = tid + nthr; x < p; x += nthr) Ln[(size_t)x * P.RM + r1] = (x < p - 1) ? Lo[(size_t)x * P.RM + (ii - 1)] : (short)jj;
    for (int x = tid + nthr; x < P.d - p; x += nthr) Rn[(size_t)x * P.RM + r1] = (x == 0) ? (short)kk : Ro[(size_t)(x - 1) * P.RM + (qq - 1)];
}
// corner of the packed LU, pivot set, tape, update flag and the new rank; one thread
__device__ __forceinline__ void append_scalars(const DevProb &P, int g, int p, int first, int r1, int ii, int jj, int kk, int qq, double pivot)
{
    inv_ptr(P, g, p, first)[(r1 + 1) * (r1 + 1) - 1] = pivot;
    int *vq = vip_ptr(P, g, p, first) + 4 * r1, *tape = P.tape + ((size_t)g * (P.d + 2) + p) * 4;
    vq[0] = tape[0] = ii; vq[1] = tape[1] = jj; vq[2] = tape[2] = kk; vq[3] = tape[3] = qq;
    P.upd[(size_t)g * (P.d + 2) + p] = 1;
    P.r[(size_t)g * (P.d + 2) + p] = r1 + 1;                                // :752
}
#endif
