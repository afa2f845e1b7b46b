// ttx_sweep_end.h -- what the end of a sweep reports: the summary of a sweep and the stopping rule.
#pragma once
#include "ttx_bondstep.h"   // stop_rule
#include "ttx_dev.h"
#include "ttx_wave.h"       // max_pos

// The end of sweep `it` from the records of its tail launch (single process): summary into the pinned slot `out`, stopping rule.  It
// runs on the quadrature's stream beside sweep kernel it+1 and reads nothing that kernel writes.  It never clears the stop flag (an
// abort of the running sweep kernel may have raised it) and raises it only where every block of that kernel decides the same at its
// entry; then no sweep kernel runs any more and the groups' amax take the corner maxima, as k_sweep_end leaves them.
__global__ __launch_bounds__(256) void k_sweep_summary(DevProb P, int it, double *out)
{
    const int m = P.d, tid = threadIdx.x, par = it & 1;
    if (tid == 0) P.ctl[2] = P.ctl[0];
    if (P.ctl[0]) return;
    const TailRec *rec = P.tailrec + (size_t)par * P.G;
    const int p_lo = P.gs[0].first, p_hi = P.gs[P.G - 1].last;
    for (int p = p_lo + tid; p <= p_hi; p += blockDim.x) {   // owner of bond p, its rank and tape entry
        int g = 0;
        while (g + 1 < P.G && P.gs[g + 1].first <= p) g++;
        const int *r = P.rq + (size_t)g * (m + 2), *tp = P.tail_tape + ((size_t)par * P.G + g) * (m + 2) * 4;
        double *e = out + SUM_HDR + P.nprocs + 5 * p;
        e[0] = (double)r[p]; e[1] = (double)tp[4 * p]; e[2] = (double)tp[4 * p + 1]; e[3] = (double)tp[4 * p + 2]; e[4] = (double)tp[4 * p + 3];
    }
    if (tid < P.G) out[SUM_HDR + P.gs[tid].gglobal] = rec[tid].initval;
    if (tid != 0) return;
    double nev = 0.0, by = 0.0, nr = 0.0;
    for (int g = 0; g < P.G; g++) { nev += (double)rec[g].neval; by += rec[g].bytes_half; nr += (double)rec[g].n_resid; }
    const double amax = max_pos(rec[0].amax, P.gs[0].amax_bnd[par]), pmax = rec[0].pivotmax;
    out[SUM_NEVAL] = nev; out[SUM_BYTES] = by; out[SUM_NRESID] = nr;
    out[SUM_AMAX] = amax; out[SUM_PMAX] = pmax; out[SUM_PMIN] = rec[0].pivotmin;
    out[SUM_VAL] = 0.0;
    const StopRule s = stop_rule(it, P.maxrank, P.accuracy, pmax, amax, P.strk[(it - 1) & 1]);
    P.strk[par] = s.strikes;
    P.ctl[1] = s.strikes;
    if (s.ready) {
        for (int g = 0; g < P.G; g++) P.gs[g].amax = max_pos(P.gs[g].amax, P.gs[g].amax_bnd[par]);
        P.ctl[0] = 1;
    }
}

// per-sweep summary of this GPU in the job-wide layout (slots of other GPUs stay zero; SUM all-reduce)
__device__ __forceinline__ void collect_summary(const DevProb &P)
{
    const int m = P.d, tid = threadIdx.x;
    double *o = P.sumsend;
    for (int g = 0; g < P.G; g++) {                                   // one thread per own bond of the group
        const GroupState &gs = P.gs[g];
        const int *r = P.r + (size_t)g * (m + 2), *tp = P.tape + (size_t)g * (m + 2) * 4;
        for (int p = gs.first + tid; p <= gs.last; p += blockDim.x) {
            double *e = o + SUM_HDR + P.nprocs + 5 * p;
            e[0] = (double)r[p]; e[1] = (double)tp[4 * p]; e[2] = (double)tp[4 * p + 1]; e[3] = (double)tp[4 * p + 2]; e[4] = (double)tp[4 * p + 3];
        }
    }
    if (tid != 0) return;
    double nev = 0.0, by = 0.0, nr = 0.0;
    for (int g = 0; g < P.G; g++) {
        const GroupState &gs = P.gs[g];
        nev += (double)gs.neval; by += gs.bytes_half; nr += (double)gs.n_resid;
        o[SUM_HDR + gs.gglobal] = gs.initval;
        if (gs.gglobal == 0) { o[SUM_AMAX] = gs.amax; o[SUM_PMAX] = gs.pivotmax; o[SUM_PMIN] = gs.pivotmin; }
    }
    o[SUM_NEVAL] = nev; o[SUM_BYTES] = by; o[SUM_NRESID] = nr;
    if (P.g0 == 0) o[SUM_VAL] = P.gs[0].val;     // identical on every GPU; contributed once
}
__global__ __launch_bounds__(256) void k_collect(DevProb P)
{
    if (blockIdx.x != 0 || P.ctl[0]) return;
    collect_summary(P);
}
// single-GPU end of sweep in one launch: snapshot for the forked quadrature, summary (written straight into the
// pinned host slot `out`), stopping rule
// fold: the sweep's exchange was k_exch_tail, whose corner maxima wait in gs.amax_bnd[it & 1] (ttx_dev.h) -- they go into the
// groups' amax first (the maximum of the same bit patterns atomic_max_pos would have combined, a NaN's included) and the slot is cleared
__global__ __launch_bounds__(256) void k_sweep_end(DevProb P, int it, double *out, int fold)
{
    const int n = P.G * (P.d + 2), m = P.d, tid = threadIdx.x;
    for (int x = tid; x < n; x += blockDim.x) P.rq[x] = P.r[x];
    if (tid == 0) P.ctl[2] = P.ctl[0];
    if (P.ctl[0]) return;
    if (fold) {
        if (tid < P.G) {
            GroupState &gs = P.gs[tid];
            gs.amax = max_pos(gs.amax, gs.amax_bnd[it & 1]);
            gs.amax_bnd[it & 1] = 0.0;
        }
        __syncthreads();
    }
    // multi-GPU job: `out` is this GPU's contribution to a SUM all-reduce -- only the bonds of its own groups, and the
    // job-wide scalars from the GPU that holds global group 0 (after k_exch_max_apply every GPU has the same maxima)
    const int p_lo = P.gs[0].first, p_hi = P.gs[P.G - 1].last;
    for (int p = p_lo + tid; p <= p_hi; p += blockDim.x) {   // owner of bond p, its rank and tape entry
        int g = 0;
        while (g + 1 < P.G && P.gs[g + 1].first <= p) g++;
        const int *r = P.r + (size_t)g * (m + 2), *tp = P.tape + (size_t)g * (m + 2) * 4;
        double *e = out + SUM_HDR + P.nprocs + 5 * p;
        e[0] = (double)r[p]; e[1] = (double)tp[4 * p]; e[2] = (double)tp[4 * p + 1]; e[3] = (double)tp[4 * p + 2]; e[4] = (double)tp[4 * p + 3];
    }
    if (tid < P.G) out[SUM_HDR + P.gs[tid].gglobal] = P.gs[tid].initval;
    if (tid != 0) return;
    double nev = 0.0, by = 0.0, nr = 0.0;
    for (int g = 0; g < P.G; g++) { const GroupState &gs = P.gs[g]; nev += (double)gs.neval; by += gs.bytes_half; nr += (double)gs.n_resid; }
    const double amax = P.gs[0].amax, pmax = P.gs[0].pivotmax;    // job-wide maxima (k_exch_max_apply), the same on every GPU
    out[SUM_NEVAL] = nev; out[SUM_BYTES] = by; out[SUM_NRESID] = nr;
    if (P.g0 == 0) { out[SUM_AMAX] = amax; out[SUM_PMAX] = pmax; out[SUM_PMIN] = P.gs[0].pivotmin; }
    out[SUM_VAL] = 0.0;
    const StopRule s = stop_rule(it, P.maxrank, P.accuracy, pmax, amax, P.ctl[1]);
    P.ctl[1] = s.strikes;
    P.ctl[0] = s.ready;
}
