// ttx_pullback.h -- TTX_FUN_PULLBACK: the integrand of a sweep is a loaded device function of a point pulled back through up to
// TTX_PULLBACK_MAX resident squared-train transports, fun(i) = h(x, logq, val) with x = Q_1(Q_2(.. Q_m(u(i)))), u_k(i) = ref_k(i_k).
//
// The definition is in include/ttx.h: the chain of ttx_sample_sq_real(.., TTX_EVAL_EXACT) calls on the layers, operation by operation.
// The sweep is the two-pass one of TTX_FUN_TRAINS (ttx_trainfun.h): pass 1 raises slots, k_pb_slots fills tval[s][0 .. d+1] = x, logq,
// val on the engine's stream, the loaded combiner's slot kernel turns them into hval behind it, pass 2 reads them.  Nothing is
// synchronised.  k_pb_list is the twin over a 32-bit index list (ttx_pullback_points, ttx_eval_device).
//
// Launch shape (pb_plan, ttx_pullback_plan.h): one wave64 per raised slot, up to 4 waves per workgroup, a capped grid that strides;
// the flags are walked with k_tf_slots's ballot.  Per wave the dynamic LDS holds two state vectors of the largest ldx over the
// layers, two sheets of the largest mode, the running point and the index row: nothing is shared between waves, wave barriers only,
// so a call repeats bit for bit whatever the grid.  Per layer t = m .. 1 and mode k = d .. 1 the ONE wave does what ttx_sample_sq_real
// does in three launches, with the same device functions (ttx_sample_sq_real.h):
//   rows    lane i, striding by 64 over 0 .. n-1: sqr_rows_one (k_sqr_rows_exact's body) into the wave's two sheets
//   pick    sqr_pick_one (k_sqr_pick's body) on those sheets; sm_bad_u on the first mode of a layer
//   step    sqr_step_one (k_sqr_step's body)
// x_k overwrites u_k in the wave's LDS row: the draw of mode k reads only u_k.  A layer's logq is summed from 0.0 over its modes and
// then added to the transport's, logq = lq_m, then logq + lq_t for t = m-1 .. 1.  A sample that fails at any layer gives the
// sampler's failed row -- x NaN, logq NaN, val 0.0 -- which is what the chain of public calls gives: a NaN row fails the next layer.
// Every index comes from lane numbers and counts, never from a value.  No atomics except the two counters (elements, failed), one
// add per busy wave each.  This kernel is latency-bound by design: one wave walks m d dependent mode steps (profiles/pullback_mi355x.txt).
// The compiler's report for gfx950: 123 / 121 VGPRs, 106 SGPRs (18 spilled to VGPR lanes), no static LDS, 36 bytes of scratch per lane
// reserved, which no instruction of either kernel touches (profiles/pullback_mi355x.txt).
// Open: an MFMA variant of the rows; held modes; a private head per layer where one engine is two layers with different nodes.
#pragma once
#include <hip/hip_runtime.h>
#include "ttx_pullback_plan.h"      // pb_lds_doubles, TTX_PB_WAVES
#include "ttx_sample_sq_real.h"     // sqr_rows_one, sqr_pick_one, sqr_step_one

// one layer as the kernels see it: the head tables of its engine (sq_head: H, the defensive terms g, the node block) with the plan's
// rows l and offsets (a mode's nodes start where its weights do), and the train with its OWN layout
struct PbLayerDev {
    const double *H, *g, *nodes;
    const int *l;                   // [d+1]
    const size_t *hoff, *woff;      // [d+1]
    const double *const *core;      // [d], 0-based mode
    const int *r, *n;               // [d+1], [d]
    int RM;
    size_t SS;
};
struct PbOps {
    int m, d, ldx, nmax;            // layers, modes, doubles per state vector and per sheet
    const int *n;                   // [d] the engine's mode sizes: the reference grid
    const double *ref;              // the reference rows, mode k at roff[k]
    const size_t *roff;             // [d]
    PbLayerDev t[TTX_PULLBACK_MAX];
};
struct PbWave { double *x, *z, *S, *C, *u; int *id; };
__device__ inline PbWave pb_wave(double *dyn, const PbOps &O, int wave)
{
    PbWave W;
    W.x = dyn + pb_lds_doubles(O.ldx, O.nmax, O.d) * wave; W.z = W.x + O.ldx; W.S = W.z + O.ldx; W.C = W.S + O.nmax; W.u = W.C + O.nmax;
    W.id = (int *)(W.u + O.d);
    return W;
}
// an index row into the wave's LDS; true when every entry lies in 1..n (wave-uniform)
template <class I>
__device__ inline bool pb_load_row(const PbOps &O, const I *row, int *id, int lane)
{
    bool bad = false;
    for (int i = lane; i < O.d; i += 64) { const int v = (int)row[i]; id[i] = v; bad |= (v <= 0 || v > O.n[i]); }
    const bool ok = __ballot(bad) == 0ull;
    __builtin_amdgcn_wave_barrier();
    return ok;
}
// The transport of the point of the index row W.id (checked): W.u ends as x.  Returns true if the sample failed at some layer
// (wave-uniform; logq and val are not to be used then).
__device__ inline bool pb_transport(const PbOps &O, const PbWave &W, int lane, double &logq, double &val)
{
    const int d = O.d;
    for (int i = lane; i < d; i += 64) W.u[i] = O.ref[O.roff[i] + (size_t)(W.id[i] - 1)];
    __builtin_amdgcn_wave_barrier();
    logq = 0.0; val = 0.0;
    for (int t = O.m - 1; t >= 0; t--) {
        const PbLayerDev &Y = O.t[t];
        bool fail = sm_bad_u(W.u, d, lane, [](int) { return false; }, (double *)nullptr);
        if (fail) return true;
        double *xa = W.x, *za = W.z;
        if (lane == 0) xa[0] = 1.0;                                             // x of the empty suffix
        double lq = 0.0;
        __builtin_amdgcn_wave_barrier();
        for (int k = d - 1; k >= 0; k--) {
            const int n = Y.n[k], r0 = Y.r[k], r1 = Y.r[k + 1];
            const double *Hk = Y.H + Y.hoff[k];
            for (int i = lane; i < n; i += 64) {
                double s, cr;
                sqr_rows_one(Hk, Y.l[k], n, r1, xa, i, s, cr);
                W.S[i] = s;
                if (i + 1 < n) W.C[i] = cr;
            }
            __builtin_amdgcn_wave_barrier();
            int ci = 0, cj = -1;
            double f0 = 1.0, f1 = 0.0, xk = 0.0;
            sqr_pick_one(n, Y.nodes + Y.woff[k], Y.g[k], W.S, W.C, W.u[k], lane, fail, lq, ci, cj, f0, f1, xk);
            if (fail) return true;
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) W.u[k] = xk;
            sqr_step_one(Y.core[k], Y.RM, Y.SS, r0, r1, n, ci, f0, f1, xa, za, lane);
            __builtin_amdgcn_wave_barrier();
            double *s_ = xa; xa = za; za = s_;
        }
        logq = t == O.m - 1 ? lq : logq + lq;
        val = xa[0];
        __builtin_amdgcn_wave_barrier();
    }
    return false;
}
// what a point writes: its d coordinates to xo, logq and val; a bad row NaN everywhere, a failed sample x NaN, logq NaN, val 0.0
__device__ inline void pb_store(const PbWave &W, int d, bool ok, bool fail, double logq, double val, double *xo, double *lo, double *vo, int lane)
{
    const double nan = __builtin_nan("");
    for (int i = lane; i < d; i += 64) xo[i] = (ok && !fail) ? W.u[i] : nan;
    if (lane == 0) { *lo = (ok && !fail) ? logq : nan; *vo = !ok ? nan : fail ? 0.0 : val; }
}

// ---- the slot kernel: behind pass 1 on the engine's stream ------------------------------------------------------------------------
// tval[s][0 .. d-1] = x, tval[s][d] = logq, tval[s][d+1] = val; the flag stays raised for the loaded combiner.  A row with an entry
// outside 1..n (the sweep writes none) reads nothing and gives NaN.  cnt[0]: the elements this launch evaluated, cnt[1]: the failed ones
__global__ __launch_bounds__(64 * TTX_PB_WAVES) void k_pb_slots(PbOps O, long long nslot, const short *hidx, const unsigned char *hreq, double *tval, unsigned long long *cnt)
{
    extern __shared__ __align__(16) double pb_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwg = blockDim.x >> 6, d = O.d;
    const PbWave W = pb_wave(pb_dyn, O, wave);
    const long long nw = (long long)gridDim.x * nwg, w = (long long)blockIdx.x * nwg + wave;
    unsigned long long done = 0, failed = 0;
    for (long long base = w; base < nslot; base += 64 * nw) {
        const long long mine = base + (long long)lane * nw;
        unsigned long long todo = __ballot(mine < nslot && hreq[mine] != 0);
        done += __popcll(todo);
        while (todo) {
            const int b = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const long long s = base + (long long)b * nw;
            __builtin_amdgcn_wave_barrier();
            const bool ok = pb_load_row(O, hidx + (size_t)s * d, W.id, lane);
            double logq = 0.0, val = 0.0;
            const bool fail = ok && pb_transport(O, W, lane, logq, val);
            failed += fail ? 1 : 0;
            double *row = tval + (size_t)s * (d + 2);
            pb_store(W, d, ok, fail, logq, val, row, row + d, row + d + 1, lane);
        }
    }
    if (lane == 0 && done) atomicAdd(cnt, done);
    if (lane == 0 && failed) atomicAdd(cnt + 1, failed);
}

// ---- the list twin (ttx_pullback_points, ttx_eval_device): one wave per point of a 32-bit index list ---------------------------------
// tval != null: the rows go to tval[npts][d+2] for the combiner's list kernel; otherwise to the caller's x [npts][d], logq and val.
// The host entries refuse an index outside the modes before anything is launched; a row that is out of range all the same reads nothing
__global__ __launch_bounds__(64 * TTX_PB_WAVES) void k_pb_list(PbOps O, long long npts, const int *ind, double *x, double *lq, double *vl, double *tval, unsigned long long *cnt)
{
    extern __shared__ __align__(16) double pb_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwg = blockDim.x >> 6, d = O.d;
    const PbWave W = pb_wave(pb_dyn, O, wave);
    const long long nw = (long long)gridDim.x * nwg;
    unsigned long long done = 0, failed = 0;
    for (long long p = (long long)blockIdx.x * nwg + wave; p < npts; p += nw) {
        done++;
        __builtin_amdgcn_wave_barrier();
        const bool ok = pb_load_row(O, ind + (size_t)p * d, W.id, lane);
        double logq = 0.0, val = 0.0;
        const bool fail = ok && pb_transport(O, W, lane, logq, val);
        failed += fail ? 1 : 0;
        if (tval) { double *row = tval + (size_t)p * (d + 2); pb_store(W, d, ok, fail, logq, val, row, row + d, row + d + 1, lane); }
        else pb_store(W, d, ok, fail, logq, val, x + (size_t)p * d, lq + p, vl + p, lane);
    }
    if (lane == 0 && done) atomicAdd(cnt, done);
    if (lane == 0 && failed) atomicAdd(cnt + 1, failed);
}
