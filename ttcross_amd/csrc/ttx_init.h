// ttx_init.h -- the start of a run: the initial cross (k_init_*) and k_reset.
#pragma once
#include "ttx_integrands.h"
#include "ttx_wave.h"

// ------------------------------------------------------------------------------------------------
// K0: initial cross (lib/dmrgg.f90:151-248)
// ------------------------------------------------------------------------------------------------
struct DiagIdx { const int *n; int k, s; __device__ __forceinline__ int operator()(int p) const { return (k - 1 + s * (p - 1)) % n[p] + 1; } };
struct FixIdx { const int *ind; int self, selfval; __device__ __forceinline__ int operator()(int s) const { return s == self ? selfval : ind[s]; } };

// every group evaluates all nn*snum shifted-diagonal samples (a few hundred) so that the MAXLOC of :196
// needs no exchange; each group is charged only its own share of evaluations (:160,181)
// ldsrows: 0 the generic accessor; 1 one index row per thread in LDS, the mode sizes read from global memory by every thread, 256
// threads; 2 (InitSamplesPlan, ttx_create_plan.h) the same rows with the mode sizes staged in LDS once behind them, and a block of
// up to 512 threads so that the few hundred samples take ONE pass instead of a full and a part-empty one.  The sample a thread
// takes, its row, its evaluation and the first-maximum rule on the sample number are the same in every form.
template <int FUN>
__global__ __launch_bounds__(512) void k_init_samples(DevProb P, int snum, int nn, int ldsrows, int shift_hi)
{
    extern __shared__ __align__(16) double dyn[];
    double *par = dyn;
    __shared__ double sha[8], shv[8]; __shared__ int shi[8];
    const int g = blockIdx.x, tid = threadIdx.x;
    GroupState &gs = P.gs[g];
    for (int x = tid; x < P.npar; x += blockDim.x) par[x] = P.par[x];
    __syncthreads();
    double ba = -1.0, bv = 0.0; int bi = INT_MAX;
    // each thread writes the multi-index of its sample once into an aligned, padded LDS row (dims 1..m-1 | dim m) and
    // evaluates through the chunked evaluators instead of recomputing the shifted-diagonal index in every pass
    const int m = P.d, VSr = ((m + 7) & ~7) + 8;
    short *rows = (short *)(((size_t)(dyn + P.npar) + 15) & ~(size_t)15);
    short *row = rows + (size_t)tid * VSr;
    if (FUN == FUN_ISING && P.arith && P.ising_id != 1 && ldsrows) {
        // TTX_ARITH=fast, Ising D/E: one WAVE per sample (de_fast_point_wave: the lanes share the range ends).  A shifted diagonal with
        // shift 0 repeats one node in every dimension; for a node close to 1 no range reaches the cut and one thread would walk the
        // whole pair triangle (7 ms of the 220 ms of D_256 went into this kernel)
        const int lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6, n1m = P.n[1];
        double *xv = (double *)rows + (size_t)wv * 2 * (m + 64), *wvv = xv + (m + 64);
        int *nl = (int *)((double *)rows + (size_t)nw * 2 * (m + 64));      // mode sizes (one global round trip instead of one per sample)
        for (int x = tid; x < m; x += blockDim.x) nl[x] = P.n[x + 1];
        __syncthreads();
        for (int il = wv; il < nn * snum; il += nw) {
            const int k = il % nn + 1, sft = il / nn;
            __builtin_amdgcn_wave_barrier();
            for (int x = lane; x < m; x += 64) { const int ix = (k - 1 + sft * x) % nl[x]; xv[x] = par[ix]; wvv[x] = par[n1m + ix]; }
            __builtin_amdgcn_wave_barrier();
            const double f = de_fast_point_wave(P.ising_id, m, xv, wvv, lane);
            const double a = fabs(f);
            if (lane == 0 && (a > ba || (a == ba && il < bi))) { ba = a; bv = f; bi = il; }
        }
    } else
    if (!ldsrows)                                             // rows do not fit the LDS: generic accessor
        for (int il = tid; il < nn * snum; il += blockDim.x) {
            DiagIdx ix{P.n, il % nn + 1, il / nn};
            double f = eval_fun<FUN>(P, par, ix, (long)g * P.HS + il);
            double a = fabs(f);
            if (a > ba || (a == ba && il < bi)) { ba = a; bv = f; bi = il; }
        }
    else {
    const int *nl = P.n + 1;                                  // nl[p - 1]: the size of mode p
    if (ldsrows == 2) {
        int *nls = (int *)(((size_t)(rows + (size_t)blockDim.x * VSr) + 15) & ~(size_t)15);
        for (int x = tid; x < m; x += blockDim.x) nls[x] = P.n[x + 1];
        __syncthreads();
        nl = nls;
    }
    for (int il = tid; il < nn * snum; il += blockDim.x) {
        const int k = il % nn + 1, sft = il / nn;
        for (int p = 1; p <= m; p++) row[p - 1] = (short)((k - 1 + sft * (p - 1)) % nl[p - 1] + 1);
        for (int x = m; x < VSr; x++) row[x] = 1;
        row[m - 1 + 0] = row[m - 1];                          // (dim m stays readable as `self`)
        const int self = row[m - 1];
        row[m - 1] = 1;                                       // pad of the dims 1..m-1 part
        Src3 sx{row, m - 1, self, row + m};                   // empty right part: nb = 0, never read
        double f = eval_src3<FUN, true>(P, par, sx, (long)g * P.HS + il);
        double a = fabs(f);
        if (a > ba || (a == ba && il < bi)) { ba = a; bv = f; bi = il; }
    }
    }
    if (HOST_PASS1(FUN, P)) return;
    block_argmax(ba, bv, bi, sha, shv, shi);
    if (tid == 0) {
        gs.amax = ba;                                             // :180,201
        // :153-156 shifts(p) = int(dble(snum)*dble(p)/nproc); own share of the samples (:160,181)
        int gg = gs.gglobal;
        int lo = (int)((double)snum * (double)gg / P.nprocs);
        int hi = (gg + 1 == P.nprocs) ? snum : (int)((double)snum * (double)(gg + 1) / P.nprocs);
        gs.neval = (long long)nn * (hi - lo);
        if (g == 0) {
            if (bi == INT_MAX) bi = 0;                            // every sample a NaN: the first one, as idamax
            int s = bi / nn, k = bi % nn + 1;
            for (int p = 1; p <= P.d; p++) P.ind0[p] = (k - 1 + s * (p - 1)) % P.n[p] + 1;   // :205-209
            P.ind0[P.d + 1] = 1;
        }
    }
}

// fibers through the initial index for own cores (:221-232)
template <int FUN>
__global__ __launch_bounds__(256) void k_init_fibers(DevProb P)
{
    extern __shared__ __align__(16) double dyn[];
    double *par = dyn;
    __shared__ double shm[4];
    const int g = blockIdx.y, tid = threadIdx.x;
    GroupState &gs = P.gs[g];
    const int p = gs.first + blockIdx.x;
    if (p > gs.last + 1) return;
    for (int x = tid; x < P.npar; x += blockDim.x) par[x] = P.par[x];
    __syncthreads();
    double *A = core_ptr(P, P.arg, g, p, gs.first);
    double mx = 0.0;
    for (int j = tid; j < P.n[p]; j += blockDim.x) {
        FixIdx ix{P.ind0, p, j + 1};
        double f = eval_fun<FUN>(P, par, ix, (long)g * P.HS + (long)blockIdx.x * P.NM + j);
        A[(size_t)P.RM * j] = f;
        mx = fmax(mx, fabs(f));
    }
    if (HOST_PASS1(FUN, P)) return;
    mx = block_max(mx, shm);
    if (tid == 0) { atomic_max_pos(&gs.amax, mx); atomicAdd((unsigned long long *)&gs.neval, (unsigned long long)P.n[p]); }
}

// inv, col, row, index tables of the rank-1 start (:213-217, :235-248)
__global__ __launch_bounds__(256) void k_init_factors(DevProb P)
{
    const int g = blockIdx.y, tid = threadIdx.x;
    GroupState &gs = P.gs[g];
    const int first = gs.first, p = first + blockIdx.x, m = P.d;
    if (p > gs.last + 1) return;
    const double *A = core_ptr(P, P.arg, g, p, first);
    if (p <= gs.last) {
        double piv = A[(size_t)P.RM * (P.ind0[p] - 1)];
        double rp = 1.0 / piv;
        double *C = core_ptr(P, P.col, g, p, first);
        for (int j = tid; j < P.n[p]; j += blockDim.x) C[(size_t)P.RM * j] = rp * A[(size_t)P.RM * j];  // d2_lual, r=1
        if (tid == 0) {
            inv_ptr(P, g, p, first)[0] = piv;
            int *v = vip_ptr(P, g, p, first);
            v[0] = 1; v[1] = P.ind0[p]; v[2] = P.ind0[p + 1]; v[3] = 1;
        }
    }
    if (p >= first + 1) {
        double *W = core_ptr(P, P.row, g, p, first);
        for (int k = tid; k < P.n[p]; k += blockDim.x) W[k] = A[(size_t)P.RM * k];                      // d2_luar, r=1: identity
    }
    // tables: L for bonds first-1..last (block b handles bond first-1+b), R for bonds first..last+1
    {
        int s = first - 1 + blockIdx.x;                    // L bond
        short *Lt = L_ptr(P, g, s, first);
        for (int x = tid; x < s; x += blockDim.x) Lt[(size_t)x * P.RM] = (short)P.ind0[x + 1];
        int s2 = first + blockIdx.x;                       // R bond
        short *Rt = R_ptr(P, g, s2, first);
        for (int x = tid; x < m - s2; x += blockDim.x) Rt[(size_t)x * P.RM] = (short)P.ind0[s2 + 1 + x];
        if (tid == 0 && blockIdx.x == 0) inv_ptr(P, g, first - 1, first)[0] = 1.0;   // :147
        if (P.arith && P.fpersist) {
            // TTX_ARITH=fast, Ising D/E: the table entries of the rank-1 start (pivot 0 of every bond) from scratch: wave 0 the left
            // multi-index ind0[1..s] of bond s, wave 1 the right multi-index ind0[s2+1..m] of bond s2
            extern __shared__ __align__(16) double dyn_i[];
            const int wv_ = tid >> 6, lane_ = tid & 63;
            if (wv_ < 2) {
                double *xs = dyn_i + (size_t)wv_ * 2 * (m + 8), *ws = xs + m + 8;
                const int len = wv_ == 0 ? s : m - s2, o0 = wv_ == 0 ? 1 : s2 + 1, bnd = wv_ == 0 ? s : s2;
                if (P.fun_id == FUN_MVN) {                     // mvn: dv = x - mu, Y = S dv, Q (entry k of the right side is dim s2 + k, 0-based)
                    for (int k = lane_; k < len; k += 64) xs[k] = P.par[P.ind0[o0 + k] - 1] - P.aux[o0 - 1 + k];
                    __builtin_amdgcn_wave_barrier();
                    mvn_entry_scratch(P, xs, len, o0 - 1, fast_dv(P, wv_, g, bnd, first), fast_near(P, wv_, g, bnd, first), fast_piv(P, wv_, g, bnd, first), lane_);
                } else {
                for (int k = lane_; k < len; k += 64) { const int ix = P.ind0[o0 + k]; xs[k] = P.par[ix - 1]; ws[k] = P.par[P.n[1] + ix - 1]; }
                __builtin_amdgcn_wave_barrier();
                fast_entry_scratch(xs, ws, len, wv_, fast_near(P, wv_, g, bnd, first), fast_piv(P, wv_, g, bnd, first), P.RM, lane_);
                }
            }
        }
    }
}

// pivotmax_prev (:234) and the group's factor of the initial quadrature value (:250-258); one block per group: the ddot of every
// core, then the ordered product.
// wave = 0: one THREAD per core for the ddot, then thread 0 multiplies with one global load per core (the form the kernel had).
// wave = 1: one WAVE per core.  The lanes load A_j and w_j and multiply, one product per lane; the ordered sum t = t + A_j * w_j
// takes the products in j order out of the lanes' registers (two v_readlane_b32 per term, lane_get of ttx_wave.h), so every
// lane adds the same operands in the same order as the one thread did: the bits stay.  The divisors of the serial product are
// loaded by all threads ahead of it.
// out != nullptr (the head of the single-process pipelined loop, LoopPlan::head_direct): the initial summary goes straight into the
// pinned slot `out` from this launch, as k_sweep_end writes a sweep's -- everything collect_summary would read is final here
// (ranks 1 and tapes -1 from k_reset, the groups' counters and maxima after k_init_fibers, the value 0), and every entry of the
// slot is written: block g its bonds and its factor, block 0 the scalars and the zeros of the entries nobody owns.
__global__ __launch_bounds__(256) void k_init_final(DevProb P, int wave, double *out)
{
    __shared__ double dots[256], divs[256];
    const int g = blockIdx.x, tid = threadIdx.x;
    GroupState &gs = P.gs[g];
    const bool lastgroup = (gs.last + 1 == P.d && gs.gglobal == P.nprocs - 1);
    const int ncore = gs.last - gs.first + 1 + (lastgroup ? 1 : 0);
    double val = 1.0;
    if (P.has_quad) {
        for (int c0 = 0; c0 < ncore; c0 += 256) {
            if (wave) {
                const int lane = tid & 63, nw = blockDim.x >> 6, cend = min(ncore, c0 + 256);
                for (int c = c0 + (tid >> 6); c < cend; c += nw) {
                    const int p = gs.first + c, np_ = P.n[p];
                    const double *A = core_ptr(P, P.arg, g, p, gs.first), *w = P.quadw + (size_t)p * P.NM;
                    double t = 0.0;
                    for (int b = 0; b < np_; b += 64) {
                        const int j = b + lane, nb = min(64, np_ - b);
                        const double pr = j < np_ ? A[(size_t)P.RM * j] * w[j] : 0.0;
                        for (int k = 0; k < nb; k++) t = t + lane_get(pr, k);
                    }
                    if (lane == 0) dots[c - c0] = t;
                }
                if (c0 + tid < cend) { const int p = gs.first + c0 + tid; divs[tid] = p <= gs.last ? inv_ptr(P, g, p, gs.first)[0] : 0.0; }
            } else {
            const int c = c0 + tid;
            if (c < ncore) {
                const int p = gs.first + c;
                const double *A = core_ptr(P, P.arg, g, p, gs.first), *w = P.quadw + (size_t)p * P.NM;
                double t = 0.0;
                for (int j = 0; j < P.n[p]; j++) t = t + A[(size_t)P.RM * j] * w[j];
                dots[tid] = t;
            }
            }
            __syncthreads();
            if (tid == 0)
                for (int c2 = c0; c2 < min(ncore, c0 + 256); c2++) {
                    const int p = gs.first + c2;
                    if (p <= gs.last) val = val * dots[c2 - c0] / (wave ? divs[c2 - c0] : inv_ptr(P, g, p, gs.first)[0]);
                    else val = val * dots[c2 - c0];
                }
            __syncthreads();
        }
    }
    if (tid == 0) { gs.pivotmax_prev = gs.amax; gs.pivotmax = -1.0; gs.pivotmin = -1.0; gs.initval = val; }
    if (!out) return;
    const int m = P.d;
    const int *r = P.r + (size_t)g * (m + 2), *tp = P.tape + (size_t)g * (m + 2) * 4;
    for (int p = gs.first + tid; p <= gs.last; p += blockDim.x) {
        double *e = out + SUM_HDR + P.nprocs + 5 * p;
        e[0] = (double)r[p]; e[1] = (double)tp[4 * p]; e[2] = (double)tp[4 * p + 1]; e[3] = (double)tp[4 * p + 2]; e[4] = (double)tp[4 * p + 3];
    }
    if (g == 0)
        for (int p = tid; p <= m; p += blockDim.x)
            if (p < P.gs[0].first || p > P.gs[P.G - 1].last) { double *e = out + SUM_HDR + P.nprocs + 5 * p; for (int x = 0; x < 5; x++) e[x] = 0.0; }
    if (tid != 0) return;
    out[SUM_HDR + gs.gglobal] = val;
    if (gs.gglobal == 0) { out[SUM_AMAX] = gs.amax; out[SUM_PMAX] = -1.0; out[SUM_PMIN] = -1.0; }
    if (g != 0) return;
    double nev = 0.0, by = 0.0, nr = 0.0;
    for (int x = 0; x < P.G; x++) { const GroupState &o = P.gs[x]; nev += (double)o.neval; by += o.bytes_half; nr += (double)o.n_resid; }
    out[SUM_NEVAL] = nev; out[SUM_BYTES] = by; out[SUM_NRESID] = nr;
    out[SUM_VAL] = P.gs[0].val;
    for (int x = SUM_VAL + 1; x < SUM_HDR; x++) out[x] = 0.0;
}

// start of a run (lib/dmrgg.f90:96-100, 141-148, 279-288): every per-run quantity back to its initial value in ONE launch
// (the bond ranges first/last/gglobal of the groups never change and are set when the engine is created)
__global__ __launch_bounds__(256) void k_reset(DevProb P, size_t SB, size_t QB)
{
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
    const size_t nr = (size_t)P.G * (P.d + 2);
    for (size_t x = t0; x < nr; x += nt) { P.r[x] = 1; P.rr[x] = 1; P.upd[x] = 0; }
    for (size_t x = t0; x < 4 * nr; x += nt) P.tape[x] = -1;
    for (size_t x = t0; x < SB; x += nt) P.sumsend[x] = 0.0;
    for (size_t x = t0; x < QB; x += nt) P.qsend[x] = 0.0;
    if (t0 < 4) P.ctl[t0] = 0;
    if (t0 < 2) P.strk[t0] = 0;
    if (P.lot_ctr) for (size_t x = t0; x < (size_t)P.G; x += nt) P.lot_ctr[x] = 0u;
    if (P.cl_ctr) {
        for (size_t x = t0; x < (size_t)P.G; x += nt) P.cl_ctr[x] = 0u;
        ClPart z; z.ab = 0.0; z.bb = 0.0; z.mx = 0.0; z.ix = 0; z.pad = 0;
        for (size_t x = t0; x < (size_t)2 * P.G * TTX_CLREC; x += nt) P.cl_part[x] = z;
    }
    for (size_t g = t0; g < (size_t)P.G; g += nt) {
        GroupState &gs = P.gs[g];
        gs.amax = 0.0; gs.pivotmax = -1.0; gs.pivotmin = -1.0; gs.pivotmax_prev = 0.0;
        gs.neval = 0; gs.rngpos = 0; gs.val = 0.0; gs.initval = 0.0; gs.bytes_half = 0.0; gs.n_resid = 0;
        gs.amax_bnd[0] = 0.0; gs.amax_bnd[1] = 0.0;
        gs.rngword = 0; gs.rngword_pos = 0; gs.zk_epoch = 0; gs.n_zload = 0; gs.n_wload = 0;     // nothing carried into a run (ttx_dev.h)
#ifdef TTX_STAMPS
        for (int a = 0; a < 2; a++) { gs.nstamp[a] = 0; for (int b = 0; b < 16; b++) gs.stamp[a][b] = 0; }
#endif
    }
}
