// ttx_cluster.h -- the whole sweep of one bond group in ONE launch by a CLUSTER of workgroups (Ising C fast path).
//
// The multi-kernel path pays six dependent launches per bond step and the single-workgroup kernel (ttx_fused.h)
// pushes every fiber through one CU.  Here NB workgroups of 256 threads share a bond group and stay resident for
// the whole sweep (lib/dmrgg.f90:329-760):
//   * the blocks of a group are placed on ONE XCD (workgroups are dealt round-robin to the 8 XCDs -- checked by
//     ttx_k_xcc_map -- so block ids g, g+8, g+16, ... share an L2): what they exchange stays in that L2;
//   * each block owns a slice of the mode index (j of the column fiber, k of the row fiber): it evaluates, keeps
//     (LDS) and later appends exactly that slice, so fibers never travel between blocks;
//   * the small serial parts (lottery draw and its arg-max, acceptance test, pivot lists) are computed redundantly and
//     identically by every block, so the only cross-block traffic per rook half-step is ONE tagged 32-byte record per
//     block (its partial arg-max), written with one 16-byte store pair and polled with L1-bypassing loads -- no fence,
//     no counter; once per bond step a counter barrier with release/acquire publishes the appended slabs;
//   * everything that is fixed during a bond step is staged in LDS once: node/weight VALUES of both pivot sets, the
//     prefix states of the integrand's two running sums per pivot row, the neighbour LU factors, the factor rows at
//     the current pivot, and -- for the whole launch -- the sorted pivot lists of every own bond;
//   * every wait is bounded: a block that waits too long raises the abort flag (pinned host memory), all blocks leave,
//     and the host reports the failure instead of hanging the GPU.
// All blocks of all groups must be resident at once.  The host takes this path only when the grid fits HALF of what the
// occupancy calculator says the device can hold for this kernel's LDS footprint (room for the forked quadrature and a
// second engine); TTX_CLUSTER_COOP=1 additionally launches it as a COOPERATIVE kernel (the runtime itself then refuses a
// grid that cannot be co-resident; ~30 us per launch dearer).  Should a wait still time out, the kernel stops every later
// kernel of the sweep (ctl[0]) and ttx_run replays the run on the multi-kernel chain, which gives the identical result
// (ttx_cluster_fallbacks).
// Arithmetic and its order are identical to the other two paths (and to the oracle): same device functions, the
// first-max rule is applied on global fiber positions, reused partial results are bit-identical by construction.
#pragma once
#include "ttx_fused.h"
#include "ttx_mvn.h"
#include "ttx_cluster_rules.h"   // cl_slice, cl_wact, cl_key, cl_ordered_sum: the rules a host program checks

#define CB 256      // threads of a cluster workgroup

// Memory operands of the residual sums (cl_ordered_sum, ttx_cluster_rules.h).  ClStrided: the entries base[at + stride * s],
// s = 0, 1, ... of a factor -- a running wave-uniform pointer, stepped by a scalar add per term, and the lane's fixed byte
// offset (an element's place within a slab: far below 2^32), so a load costs the vector unit no address arithmetic.
struct ClD2 { double a, b; };
struct ClStrided {
    const char *p; size_t sb; unsigned at;
    __device__ __forceinline__ ClStrided(const double *base, size_t at_, size_t stride) : p((const char *)base), sb(8 * stride), at((unsigned)(8 * at_)) {}
    __device__ __forceinline__ double operator()() { const double v = *(const double *)(p + at); p += sb; return v; }
};

// Ising C integrand from VALUE rows, with the two running sums resumed from per-row prefix states: (pv, pvk) is the
// state of the descending sum after the right row bn (dims A+3..m), (pw, pwk) the state of the ascending sum after
// the left row an (dims 1..A).  The states are produced by exactly the operations f_ising_c4v would perform, so the
// result is bit-identical; per element this saves one of the three passes over the m dimensions.
__device__ __forceinline__ double f_ising_c4p(int m, int A, const double *an, const double *aw, double s1n, double s1w,
                                              double s2n, double s2w, const double *bn, const double *bw,
                                              double pv, double pvk, double pw, double pwk)
{
    const int nb = m - A - 2;
    double v = pv, w = pw, vk = pvk, wk = pwk;
    auto vstep = [&](double xv) { vk = vk * xv; v = v + vk; };
    auto wstep = [&](double xv) { wk = wk * xv; w = w + wk; };
    vstep(s2n); vstep(s1n);
    chain8v<true>(an, A, vstep);
    wstep(s1n); wstep(s2n);
    chain8v<false>(bn, nb, wstep);
    double b = 1.0 / (v * w);
    double f = 2 * b;
    auto fstep = [&](double xv) { f = f * xv; };
    chain8v<false>(aw, A, fstep);
    fstep(s1w); fstep(s2w);
    chain8v<false>(bw, nb, fstep);
    return f;
}

// The same integrand from rows PADDED to whole chunks of 8 with neutral elements (staged so by k_sweep_cluster<false, true>): the
// chains take chunk COUNTS (cA over the left row, cB over the right row) and hold no remainder and no test.
//   * weight rows end in 1.0:  f * 1.0 == f, always;
//   * node rows end in 0.0 BEHIND the last entry in processing order: vk = vk * 0.0 is +-0 while vk is finite and v + (+-0) == v
//     for every v but -0 (v starts at 1.0 or at a prefix state that did, and only grows by products of nodes >= 0), so v and w come
//     out bit for bit; vk and wk are dead behind the chain.  inf * 0.0 is NaN: the host takes this evaluator only after it has seen
//     every node in [0,1] (all running products finite).
// an is the left node row in PROCESSING order of the descending sum (dimension A first); aw, bn, bw are in dimension order.
// One loop form: a chunk is four ds_read_b128 and 16 dependent instructions.  (A two-register-set form with the reads of chunk c+1
// issued ahead of the steps of chunk c measured the same: profiles/HISTORY.md.)
template <class STEP>
__device__ __forceinline__ void chain8w(const double *p, int nc, STEP step)
{
#pragma unroll 1
    for (int ch = 0; ch < nc; ch++) {
        double x[8];
        ld8d(p + 8 * ch, x);
#pragma unroll
        for (int k = 0; k < 8; k++) step(x[k]);
    }
}
__device__ __forceinline__ double f_ising_c4w(int cA, int cB, const double *an, const double *aw, double s1n, double s1w,
                                              double s2n, double s2w, const double *bn, const double *bw,
                                              double pv, double pvk, double pw, double pwk)
{
    double v = pv, w = pw, vk = pvk, wk = pwk;
    auto vstep = [&](double xv) { vk = vk * xv; v = v + vk; };
    auto wstep = [&](double xv) { wk = wk * xv; w = w + wk; };
    vstep(s2n); vstep(s1n);
    chain8w(an, cA, vstep);
    wstep(s1n); wstep(s2n);
    chain8w(bn, cB, wstep);
    double b = 1.0 / (v * w);
    double f = 2 * b;
    auto fstep = [&](double xv) { f = f * xv; };
    chain8w(aw, cA, fstep);
    fstep(s1w); fstep(s2w);
    chain8w(bw, cB, fstep);
    return f;
}

// Maximum over a wave of the doubles the rook loop reduces, by their integer key (ttx_cluster_rules.h): the fiber maxima
// mx (fmax of |values| from 0.0: fmax drops a NaN operand) and the residual maxima ab (|b| that compared greater than the
// start value -1.0, or that start value: a NaN compares false) are >= +0.0 or -1.0 and never a NaN.  Two integer trees of
// one v_max_*_dpp per step (wave_max_i, wave_max_u) -- the high words, then the low words of the lanes that hold the largest high
// word -- where wave_max on the register pair takes six instructions per step.  Bit for bit the value wave_max returns.
__device__ __forceinline__ double wave_max_key(double x)
{
    const ClKey k = cl_key(x);
    const int hmax = wave_max_i(k.hi);
    const unsigned lmax = wave_max_u(cl_key_lo_at(k, hmax));
    return cl_unkey(ClKey{hmax, lmax});
}
// arg-max over a wave by the first-max rule (larger |.| wins, ties go to the lower position) in two cheap passes on the DPP
// path: the maximum of |.| (wave_max_key), then the smallest (position, sign) key among the lanes that hold it (wave_min_i of
// ttx_wave.h, an integer min per step) -- a fraction of the instructions of the three-operand compare-and-select of wave_argmax.  a
// is never NaN (a NaN residual never replaces the start value -1), so the maximum and == are exact here.  Result in every lane.
__device__ __forceinline__ void wave_argmax2(double &a, double &v, int &idx)
{
    const double amx = wave_max_key(a);
    const int key = (a == amx && idx != INT_MAX) ? ((idx << 1) | (signbit(v) ? 1 : 0)) : INT_MAX;
    const int kmin = wave_min_i(key);
    a = amx;
    if (kmin == INT_MAX) { idx = INT_MAX; v = 0.0; }
    else { idx = kmin >> 1; v = (kmin & 1) ? -amx : amx; }
}

// TTX_ARITH=fast for Ising C: the two running sums of test_crs_ising.f90:197-204 are affine in their start state, so with the
// prefix states of the pivot rows (pv, pvk after the right row; pw, pwk after the left row), the sums SL / SR of the partial
// products that start at the bond and the weight products WL / WR an element is a closed form of its two free nodes:
//   v = pv + pvk xk (1 + xj (1 + SL)),   w = pw + pwk xj (1 + xk (1 + SR)),   f = 2 / (v w) * WL wj wk WR
// -- fifteen operations instead of a dependent chain of 2 m fed from LDS; equal to the exact value to rounding.
__device__ __forceinline__ double f_ising_cfast(double xj, double wj, double xk, double wk, double pv, double pvk, double pw, double pwk,
                                                double SL, double WL, double SR, double WR)
{
    const double v = pv + pvk * xk * (1.0 + xj * (1.0 + SL));
    const double w = pw + pwk * xj * (1.0 + xk * (1.0 + SR));
    return 2.0 / (v * w) * ((WL * wj) * (wk * WR));
}

// 16-byte records exchanged between the blocks of a cluster: one store / one load instruction each, agent scope
// (sc1: the store goes through to the point of coherence, the load does not hit in the vector L1)
typedef unsigned int u4 __attribute__((ext_vector_type(4)));
struct ClRec { u4 a, b; };
static_assert(sizeof(ClRec) == sizeof(ClPart), "record buffers are sized as ClPart: [2][G][TTX_CLREC] u4 arg-max records, then as many running-maximum records");
__device__ __forceinline__ void st16(void *p, u4 v) { asm volatile("global_store_dwordx4 %0, %1, off sc1" :: "v"(p), "v"(v) : "memory"); }
__device__ __forceinline__ u4 ld16(const void *p)
{
    u4 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
    return v;
}

// XCC_ID hardware register (id 20, 4 bits): the XCD this wave runs on
__device__ __forceinline__ int xcc_id() { return (int)__builtin_amdgcn_s_getreg(((4 - 1) << 11) | 20) & 15; }

// Barrier across the workgroups of one cluster with release/acquire semantics for ordinary global data; false: timed
// out / aborted (every thread of the block gets the same answer).  Every wave first waits for its own stores to be
// acknowledged by the L2; after the block barrier ONE wave performs the agent-scope release (L2 write-back), the
// counter increment, the bounded spin and the agent-scope acquire: cache maintenance acts on the CU's L1 and the XCD's
// L2, not on a wave, so repeating it per wave only multiplies its cost (measured: 12.0 -> 9.0 ms per C_64 run).
__device__ __forceinline__ bool cluster_sync(unsigned *ctr, unsigned target, int *abortflag, int *s_ok)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        int ok = 1;
        unsigned spins = 0;
        __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > (1u << 22)) { ok = 0; __hip_atomic_store(abortflag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
            if ((spins & 1023u) == 0 && __hip_atomic_load(abortflag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) { ok = 0; break; }
        }
        __atomic_thread_fence(__ATOMIC_ACQUIRE);
        *s_ok = ok;
    }
    __syncthreads();
    return *s_ok != 0;
}

#ifdef TTX_STAMPS
#define CST_DECL const bool t_me = (threadIdx.x == 0 && g == 0 && cb == 0); long long t_prev = wall_clock64()
#define CST(k) do { if (t_me) { long long t_now = wall_clock64(); gs.stamp[0][k] += t_now - t_prev; t_prev = t_now; } } while (0)
#define CST_END() do { if (t_me) gs.nstamp[0]++; } while (0)
// the entry and the exit of a launch, thread 0 of blocks 0 and 1 of group 0: GroupState::stamp[1][8 cb + k] of group 0 -- k = 0 kernel
// start to behind the staging of par, the start of the sweep and their barrier, 1 the pivot lists (rebuilt or loaded), 2 the generator powers and the
// state loads (top of the first bond step), 3 (block 0) from behind the last cluster_sync to behind exch_pack_group
#define CSE_DECL const int t_eb = (threadIdx.x == 0 && g == 0 && cb <= 1) ? cb : -1; long long t_eprev = wall_clock64()
#define CSE_MARK() do { if (t_eb >= 0) t_eprev = wall_clock64(); } while (0)
#define CSE(k) do { if (t_eb >= 0) { long long t_now = wall_clock64(); P.gs[0].stamp[1][8 * t_eb + (k)] += t_now - t_eprev; t_eprev = t_now; } } while (0)
#define CSE_END() do { if (t_eb == 0) P.gs[0].nstamp[1]++; } while (0)
// per-wave timeline of ONE bond step (launch 8, step 4, group 0): slot k of half-step h of wave (cb, wv)
#define WST(k) do { if (P.dbg && g == 0 && epoch == 8 && pp == 4 && lane == 0 && h < 8) P.dbg[((size_t)(h * 64 + cb * 4 + wv)) * 8 + (k)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define WST(k)
#define CST_DECL
#define CST(k)
#define CST_END()
#define CSE_DECL
#define CSE_MARK()
#define CSE(k)
#define CSE_END()
#endif

// The forms of the launch entry, bits of the kernel's argument `zkeep` (the host sets them: launch_sweep_kernel):
#define CL_ZKEEP 1      // the sorted distinct pivot lists of every own bond stay in LDS for the whole launch
#define CL_ZCARRY 2     // ... and travel from launch to launch through the group's image in global memory (TTX_CL_LISTS=0: rebuilt per launch)
#define CL_WORD 4       // the generator word is taken from the launch before (TTX_CL_WORD=0: raised from rngpos per launch)
#define CL_POWTAB 8     // the generator's jump powers come from cl_powtab (TTX_CL_POWTAB=0: three square-and-multiply loops per launch)
#define CL_PACK2 16     // exit: block 1 packs the left-going boundary message beside block 0 (TTX_CL_PACK2=0: block 0 packs both)
static_assert(CL_POWTAB_N == CB, "one table entry per thread of a workgroup");
__device__ const ClPowTab cl_powtab = cl_make_powtab();
// the kernel's argument block as the launch lays it out (k_sweep_cluster's parameter list): the exit reads it afresh
struct ClArgs { DevProb P; int dir, nsteps, NB, ldsinv, epoch, zkeep; };
// Image of a group's pivot lists, the LDS layout word for word ([nsteps][2][RM] keys, [nsteps][2] counts): behind the record buffers
// of cl_part, so that the kernel takes no further argument and DevProb no further field (its scalar registers are short as it is)
__device__ __forceinline__ int *cl_zimage(const DevProb &P, int g, int nsteps)
{ return (int *)(P.cl_part + (size_t)2 * P.G * TTX_CLREC) + (size_t)g * cl_zimage_ints(nsteps, P.RM); }

// CFAST: the closed form of TTX_ARITH=fast (f_ising_cfast) instead of the chains; CPAD: rows padded to whole chunks with neutral
// elements and f_ising_c4w instead of f_ising_c4p.  Both are fixed for the life of an engine, so they are compiled in: the exact
// kernels hold no closed-form arm and no fSL .. fWR, the fast kernel no chains in its hot loops.
template <bool CFAST, bool CPAD>
__global__ __launch_bounds__(CB) void k_sweep_cluster(DevProb P, int dir, int nsteps, int NB, int ldsinv, int epoch, int zkeep)
{
    extern __shared__ __align__(16) double dyn[];
    __shared__ int zc[128], zr[128], zcs[128], zrs[128], keepc[128], keepr[128];
    __shared__ int nzc, nzr, nsc, nsr, s_ok;
    __shared__ int slt[2][TTX_CLMAX + 1], wtab[TTX_CLMAX];   // slice bounds of the two modes of a bond step; waves at work per workgroup
    __shared__ ttx_cdfseg segc[TTX_TABSEG], segr[TTX_TABSEG];
    __shared__ double sha[8], shv[8], shm[8]; __shared__ int shi[8];
    __shared__ double pLw[64], pLk[64], pRv[64], pRk[64];   // prefix states of the two running sums per left / right row
    // TTX_ARITH=fast: per pivot row the sum of the partial products that start at the bond (left: descending, right: ascending) and
    // the product of its weights -- with them the integrand is a closed form of the two free nodes (f_ising_cfast)
    static_assert(!(CFAST && CPAD), "the closed form reads the rows in dimension order");
    constexpr int NFT = CFAST ? 64 : 1;
    __shared__ double fSL[NFT], fWL[NFT], fSR[NFT], fWR[NFT];
    // results of the rook loop, handed from wave 0 to the waves of the workgroup that own no fiber element at the current ranks
    __shared__ struct { int ii, jj, kk, qq, hcount, rc_k, rc_q, rr_i, rr_j; double pivot, amax, bytes_half; long long neval, n_resid; } s_rook;
    const int bid = blockIdx.x;
    const int g = (bid & 7) + 8 * (bid / (8 * NB)), cb = (bid >> 3) % NB;     // cluster of group g lives on XCD g % 8
    CSE_DECL;
    if (g >= P.G || P.ctl[0]) return;
    // Summary on the side stream (ttx_dev.h: tail_side): the rule of sweep epoch-1 has not been written to ctl[0] for certain yet, so
    // every block applies it itself to the same records -- the job-wide maxima of group 0's record with its corner maximum, and the
    // strike count after sweep epoch-2 -- and all decide alike, without a word to each other.  (ctl[0] above: an abort, or a stop
    // the summary has already recorded.)  Sweep 1 follows the initial cross: nothing to decide.
    const int bpar = (epoch - 1) & 1;
    if (P.tail_side && epoch >= 2) {
        const TailRec &t0 = P.tailrec[(size_t)bpar * P.G];
        if (stop_rule(epoch - 1, P.maxrank, P.accuracy, t0.pivotmax, max_pos(t0.amax, P.gs[0].amax_bnd[bpar]), P.strk[epoch & 1]).ready) return;
    }
    if (P.cl_test_abort && P.cl_test_abort == epoch && g == 0 && cb == 0) {    // test hook (TTX_CLUSTER_TEST_ABORT): a block that never arrives
        if (threadIdx.x == 0) { __hip_atomic_store(P.cl_abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); P.ctl[0] = 1; }
        return;
    }
    const int tid = threadIdx.x, m = P.d, RM = P.RM, NM = P.NM;
    const int lane = tid & 63, wv = tid >> 6;
    GroupState &gs = P.gs[g];
    const int first = gs.first, last = gs.last, nbonds = last - first + 1;
    int *r = P.r + (size_t)g * (m + 2);
    const int VS = ((m + 7) & ~7) + 8;
    // row stride of the value tables: 2*VS doubles would put every row on the same LDS banks (a multiple of 128 bytes), and
    // a column half-step reads 32 DIFFERENT rows with one 16-byte load per lane -- a 32-way bank conflict on every load
    // of the integrand chain.  Two extra doubles shift consecutive rows by 16 bytes: 8 rows tile the 32 banks.
    const int RS = 2 * VS + 2;
    const int n1m = P.n[1];
    const int SL = RM * ((NM + NB - 1) / NB + 1);       // most fiber entries one block owns
    unsigned *ctr = P.cl_ctr + g;
    // the barrier counter and the record tags are never reset: launch number `epoch` (1, 2, ...) of a run starts from
    // where launch epoch-1 stopped (every launch passes exactly one counter barrier per own bond)
    unsigned nbar = (unsigned)(epoch - 1) * (unsigned)min(nsteps, nbonds);
    ClPart *part = P.cl_part;
    // LDS carve-up
    double *par = dyn;
    double *XL = par + ((P.npar + 1) & ~1);            // RM rows x (VS node values, VS weight values)
    double *XR = XL + (size_t)RM * RS;
    double *acol = XR + (size_t)RM * RS;           // own slice of the column fiber
    double *arow = acol + SL;                          // own slice of the row fiber
    double *resc = arow + SL;                          // residuals of the own column / row slice at the last half-step
    double *resr = resc + SL;                          // that computed them (reused by the append, roles A and B)
    double *xsc = resr + SL;                           // RM: row-factor entries at the pivot column (kk, qq) ...
    double *xsr = xsc + ((RM + 1) & ~1);               // RM: column-factor entries at the pivot row (ii, jj)
    int *lot = (int *)(xsr + ((RM + 1) & ~1));         // 4 * nlotmax
    double *GL = (double *)(lot + 4 * ((2 * RM + 2 * NM + 4 + 1) & ~1));   // packed LU of bonds p-1 and p+1 (ldsinv only)
    double *GU = GL + (size_t)RM * RM;
    // zkeep: the sorted distinct pivot rows / columns of EVERY own bond stay in LDS for the whole launch as keys
    // (j << 16 | i), (q << 16 | k): built once, extended by insertion when a pivot is accepted.  Their order does not
    // depend on the ranks, only the flattened positions do (recomputed per bond step).
    int *ZK = (int *)(ldsinv ? GU + (size_t)RM * RM : GL);   // [nsteps][2][RM]
    int *ZN = ZK + (size_t)nsteps * 2 * RM;                  // [nsteps][2]
    for (int x = tid; x < P.npar; x += CB) par[x] = P.par[x];
    // (sweep_start also puts -1 into gs.pivotmax / gs.pivotmin, which this kernel keeps in registers and writes at its end: they
    // differ from before only after an aborted launch, whose run is replayed from k_reset on the chain path)
    // The start of the sweep (sweep_start of ttx_bondstep.h) by the whole of block 0, one rank per thread: one thread's loop over the
    // d + 1 ranks held block 0 -- and with it every block of the cluster at the first record exchange -- for about 6.5 us per launch
    // at d = 63.  r[] is first rewritten behind further barriers of this block (append_scalars).
    if (cb == 0) {
        if (tid == 0) { gs.pivotmax = -1.0; gs.pivotmin = -1.0; }
        int *rr = P.rr + (size_t)g * (m + 2);
        for (int s = tid; s <= m; s += CB) rr[s] = r[s];
    }
    __syncthreads();
    CSE(0);
    // The lists are exactly what this workgroup held when the launch before ended (built once, extended at every accepted pivot; nobody
    // else writes the pivot sets of own bonds between two launches of a run), and block 0 left them in the group's image with its launch
    // number: taken from there, one round trip.  The first launch of a run, a launch behind one that did not end regularly, and
    // TTX_CL_LISTS=0 rebuild them from vip.  (Block 0 rewrites image and tag at its END, behind a cluster_sync every block has passed.)
    if ((zkeep & CL_ZCARRY) && cl_lists_valid(gs.zk_epoch, epoch)) {
        const int *img = cl_zimage(P, g, nsteps);
        for (int x = tid; x < nbonds * 2 * RM; x += CB) ZK[x] = img[x];
        for (int x = tid; x < 2 * nbonds; x += CB) ZN[x] = img[(size_t)nsteps * 2 * RM + x];
        if (cb == 0 && tid == 0) gs.n_zload++;
        __syncthreads();
    } else if (zkeep & CL_ZKEEP) {
        int *TMP = (int *)XL;                          // XL is staged later; free scratch for now: [nsteps][2][RM]
        const int E = nbonds * 2 * RM;
        for (int x = tid; x < E; x += CB) {            // raw keys
            const int b = x / (2 * RM), side = (x / RM) & 1, u = x % RM, pb = first + b;
            if (u < r[pb]) { const int *vp = vip_ptr(P, g, pb, first) + 4 * u; TMP[x] = (vp[2 * side + 1] << 16) | vp[2 * side]; }
        }
        __syncthreads();
        for (int x = tid; x < E; x += CB) {            // rank among the bond's keys (ties by position), scatter
            const int b = x / (2 * RM), u = x % RM, nb_ = r[first + b];
            if (u < nb_) {
                const int *src = TMP + (x - u); const int a = src[u]; int ra = 0;
                for (int t = 0; t < nb_; t++) ra += (src[t] < a) || (src[t] == a && t < u);
                ZK[(x - u) + ra] = a;
            }
        }
        __syncthreads();
        for (int x = tid; x < E; x += CB) {            // drop repeats: position among the kept ones
            const int b = x / (2 * RM), u = x % RM, nb_ = r[first + b];
            if (u < nb_) {
                const int *src = ZK + (x - u); int pc = 0;
                for (int t = 1; t <= u; t++) pc += (src[t] != src[t - 1]);
                const bool keep = (u == 0) || (src[u] != src[u - 1]);
                TMP[x] = keep ? pc : -1;
                if (u == nb_ - 1) ZN[x / RM] = pc + 1;
            }
        }
        __syncthreads();
        int mykey = 0, mypos = -1;
        for (int x0 = 0; x0 < E; x0 += CB) {
            const int x = x0 + tid;
            mypos = -1;
            if (x < E) { const int b = x / (2 * RM), u = x % RM; if (u < r[first + b]) { mypos = TMP[x]; mykey = ZK[x]; } }
            __syncthreads();
            if (mypos >= 0) ZK[(x - x % RM) + mypos] = mykey;
            __syncthreads();
        }
    }
    double amax = gs.amax, pivotmax = -1.0, pivotmin = -1.0;
    if (P.tail_side && epoch >= 2) amax = max_pos(amax, gs.amax_bnd[bpar]);     // the corner maxima of the last tail launch
    const double pivotmax_prev = gs.pivotmax_prev;
    long long neval = gs.neval;
    unsigned long long rngpos = gs.rngpos;
    double bytes_half = gs.bytes_half; long long n_resid = gs.n_resid;
    int hcount = 0;                                    // half-steps exchanged so far (selects the record buffer)
    CSE(1);
    // The generator's powers: 48271^(2 t) from the compile-time table (cl_powtab), and the running word 48271^(2 rngpos + 1) from the
    // launch before, which held it in a register when it wrote gs.rngpos (cl_word_valid).  Else by square-and-multiply, as before.
    const bool ptab = (zkeep & CL_POWTAB) != 0;
    const unsigned long long bil0 = ptab ? cl_powtab.v[tid] : ttx_minstd_pow(2ull * tid);     // RNG jump of this thread's first lottery candidate
    unsigned long long sA0;
    {
        const unsigned long long cw = gs.rngword, cwpos = gs.rngword_pos;
        if ((zkeep & CL_WORD) && cl_word_valid(cw, cwpos, rngpos)) { sA0 = cw; if (cb == 0 && tid == 0) gs.n_wload++; }
        else sA0 = ttx_minstd_pow(2 * rngpos + 1);
    }
    // the generator step of a bond step, 48271^(2 nlot), without the square-and-multiply loop per step (8 rounds of two 64-bit
    // products on every lane): lane l keeps 48271^(2 l), and 48271^(2 (64 a + b)) = 48271^(2 b) * (48271^128)^a -- one lane
    // exchange and a <= 7 products below 512 candidates (the same residue: modular products are exact).  The bound 512 is
    // reasoned, not measured: the loop runs about ten rounds of two products for such nlot, so seven products are still fewer.
    const int bl0 = ptab ? (int)cl_powtab.v[lane] : (int)ttx_minstd_pow(2ull * lane);
    constexpr unsigned long long c64 = cl_minstd_pow_c(128);        // entry 64 of the table, a literal in every form
    CSE(2);
    CST_DECL;

    for (int pp = 1; pp <= nsteps; pp++) {
        if (pp > nbonds) break;
        const int p = (dir == 1) ? first + pp - 1 : last + 1 - pp;          // :330-331
        const int r0 = r[p - 1], r1 = r[p], r2 = r[p + 1], n1 = P.n[p], n2 = P.n[p + 1];
        const int nlot = r0 + n1 + n2 + r2;
        double *Cp = core_ptr(P, P.col, g, p, first), *Wq = core_ptr(P, P.row, g, p + 1, first);
        double *Ap = core_ptr(P, P.arg, g, p, first), *Aq = core_ptr(P, P.arg, g, p + 1, first);
        const short *Lt = L_ptr(P, g, p - 1, first), *Rt = R_ptr(P, g, p + 1, first);
        const int cA = (p - 1 + 7) >> 3, cB = (m - p - 1 + 7) >> 3;      // chunks of the left / right rows (f_ising_c4w)
        // The lottery's CDF segments are fetched by the two waves that have no prefix chain to run (waves 2, 3: column / row lottery),
        // count and segment in ONE round trip: the row of the table is read at full width (rows are TTX_TABSEG long, zero behind
        // the count) and only the valid part is stored.  Held in plain registers until the lists are built.
        const int sside = (tid >> 6) & 1, sseg = tid & 63;
        double sg_a0 = 0.0, sg_al = 0.0, sg_de = 0.0; int sg_k0 = 0, sg_cn = 0, myns = 0;
        auto seg_issue = [&](int Kc_, int Kr_) {
            if (tid >= 128) {
                const int K = sside ? Kr_ : Kc_; const ttx_cdfseg *sp = P.cdf_tab + (size_t)K * TTX_TABSEG + sseg;
                myns = P.cdf_ns[K]; sg_a0 = sp->a0; sg_al = sp->alast; sg_de = sp->delta; sg_k0 = sp->k0; sg_cn = sp->cnt;
            }
        };
        // ---- stage the value tables of both pivot sets (only the dimensions that exist on either side, rounded up to
        //      the 8-wide chunks the integrand reads; the walk over (row, dim) needs no division) ----
        {
            const int AL = min(VS, (p - 1 + 7) & ~7), AR = min(VS, (m - p - 1 + 7) & ~7);
            if (AL > 0) {
                int c = tid / AL, o = tid - c * AL;
                const int dc = CB / AL, dO = CB - dc * AL;
                while (c < r0) {
                    if constexpr (CPAD) {          // nodes in the order the hot chain walks them (dimension p-1 first), neutral tails
                        if (o < p - 1) {
                            const int ix = (int)Lt[(size_t)o * RM + c];
                            XL[(size_t)c * RS + (p - 2 - o)] = par[ix - 1]; XL[(size_t)c * RS + VS + o] = par[n1m + ix - 1];
                        } else { XL[(size_t)c * RS + o] = 0.0; XL[(size_t)c * RS + VS + o] = 1.0; }
                    } else {
                        const int ix = (o < p - 1) ? (int)Lt[(size_t)o * RM + c] : 1;
                        XL[(size_t)c * RS + o] = par[ix - 1]; XL[(size_t)c * RS + VS + o] = par[n1m + ix - 1];
                    }
                    c += dc; o += dO; if (o >= AL) { o -= AL; c++; }
                }
            }
            if (AR > 0) {
                int c = tid / AR, o = tid - c * AR;
                const int dc = CB / AR, dO = CB - dc * AR;
                while (c < r2) {
                    if (CPAD && o >= m - p - 1) { XR[(size_t)c * RS + o] = 0.0; XR[(size_t)c * RS + VS + o] = 1.0; }
                    else {
                        const int ix = (o < m - p - 1) ? (int)Rt[(size_t)o * RM + c] : 1;
                        XR[(size_t)c * RS + o] = par[ix - 1]; XR[(size_t)c * RS + VS + o] = par[n1m + ix - 1];
                    }
                    c += dc; o += dO; if (o >= AR) { o -= AR; c++; }
                }
            }
        }
        if (ldsinv) {                                  // neighbour LU factors for the fix-ups of the append (roles C, D)
            if (p > first) { const double *gL = inv_ptr(P, g, p - 1, first); for (int x = tid; x < r0 * r0; x += CB) GL[x] = gL[x]; }
            if (p < last)  { const double *gU = inv_ptr(P, g, p + 1, first); for (int x = tid; x < r2 * r2; x += CB) GU[x] = gU[x]; }
        }
        CST(0);
        if (zkeep & CL_ZKEEP) seg_issue(r0 * n1 - ZN[2 * (p - first)], n2 * r2 - ZN[2 * (p - first) + 1]);
        // The slice bounds of this bond step as a table, one division each, on a wave that has no prefix chain to run: lanes
        // 0..16 of wave 3 hold floor(c n1 / NB), lanes 17..33 floor(c n2 / NB), c = min(lane, NB) (slices behind the last are
        // empty); lane c then takes the participating waves of workgroup c from the widths of its two slices.  Read behind the
        // next barrier; the last reader of the step before is its append, in front of the closing cluster_sync.
        static_assert(2 * (TTX_CLMAX + 1) <= 64 && TTX_CLMAX + TTX_CLMAX + 2 < 64, "the two slice rows and the shuffles of the fill fit one wave");
        if (wv == CB / 64 - 1) {
            const int side = lane > TTX_CLMAX ? 1 : 0, c = lane - side * (TTX_CLMAX + 1);
            const int s = cl_slice(min(c, NB), side ? n2 : n1, NB);
            const int s1 = __shfl(s, lane + 1), t0 = __shfl(s, lane + TTX_CLMAX + 1), t1 = __shfl(s, lane + TTX_CLMAX + 2);
            if (lane < 2 * (TTX_CLMAX + 1)) slt[side][c] = s;
            if (lane < TTX_CLMAX) wtab[lane] = cl_wact(s1 - s, t1 - t0, r0, r2, CB / 64);
        }
        // ---- lottery (:410-484): every block draws and scores all candidates (identical results, no traffic) ----
        // generator words of the two draw columns: 48271^(2*rngpos+1) and 48271^(2*(rngpos+nlot)+1), advanced from
        // step to step by the small power 48271^(2*nlot) (every thread keeps them; no shared state, no barrier)
        if (tid == 0) s_ok = 1;                            // (read behind the rook loop; several barriers lie in between)
        const unsigned long long stepmul = cl_stepmul(nlot, [&](int b) { return (unsigned long long)(unsigned)__shfl(bl0, b); }, c64);
        const unsigned long long sA1 = ttx_mulmod31(sA0, stepmul);
        if (zkeep & CL_ZKEEP) {
            const int b = p - first;
            const int *kc = ZK + (size_t)b * 2 * RM, *kr = kc + RM;
            if (tid == 0) { nzc = ZN[2 * b]; nzr = ZN[2 * b + 1]; }
            if (tid < ZN[2 * b]) zc[tid] = ((kc[tid] & 0xffff) - 1) + r0 * ((kc[tid] >> 16) - 1) + 1;
            if (tid < ZN[2 * b + 1]) zr[tid] = ((kr[tid] & 0xffff) - 1) + n2 * ((kr[tid] >> 16) - 1) + 1;
            __syncthreads();
        } else bond_zero_lists(vip_ptr(P, g, p, first), r1, r0, n2, tid, zc, zr, zcs, zrs, keepc, keepr, &nzc, &nzr);
        CST(1);
        const int Kc = r0 * n1 - nzc, Kr = n2 * r2 - nzr;
        // (waves 2 and 3 store their segment while waves 0 and 1 run the prefix chains; without zkeep the lengths are known only
        // here, so nothing is hidden, but count and row still come in one round trip instead of two)
        if (!(zkeep & CL_ZKEEP)) seg_issue(Kc, Kr);
        if (tid >= 128) {
            ttx_cdfseg *dst = sside ? segr : segc;
            if (sseg < myns) { dst[sseg].a0 = sg_a0; dst[sseg].alast = sg_al; dst[sseg].delta = sg_de; dst[sseg].k0 = sg_k0; dst[sseg].cnt = sg_cn; }
            if (sseg == 0) { if (sside) nsr = myns; else nsc = myns; }
        }
        if (tid < r0) {                                // ascending sum over the left row (dims 1..p-1)
            double w = 1.0, wk = 1.0;
            auto wstep = [&](double xv) { wk = wk * xv; w = w + wk; };
            // (exact length: the final wk is kept.  Padded rows hold the nodes reversed: descending storage = ascending dimensions)
            if constexpr (CPAD) chain8v<true>(XL + (size_t)tid * RS, p - 1, wstep);
            else chain8v<false>(XL + (size_t)tid * RS, p - 1, wstep);
            pLw[tid] = w; pLk[tid] = wk;
            if constexpr (CFAST) {
                double sk = 1.0, ss = 0.0, ww = 1.0;
                auto sstep = [&](double xv) { sk = sk * xv; ss = ss + sk; };
                auto pstep = [&](double xv) { ww = ww * xv; };
                chain8v<true>(XL + (size_t)tid * RS, p - 1, sstep);
                chain8v<false>(XL + (size_t)tid * RS + VS, p - 1, pstep);
                fSL[tid] = ss; fWL[tid] = ww;
            }
        } else if (tid >= 64 && tid < 64 + r2) {       // descending sum over the right row (dims p+2..m)
            const int c = tid - 64;
            double v = 1.0, vk = 1.0;
            auto vstep = [&](double xv) { vk = vk * xv; v = v + vk; };
            chain8v<true>(XR + (size_t)c * RS, m - p - 1, vstep);
            pRv[c] = v; pRk[c] = vk;
            if constexpr (CFAST) {
                double sk = 1.0, ss = 0.0, ww = 1.0;
                auto sstep = [&](double xv) { sk = sk * xv; ss = ss + sk; };
                auto pstep = [&](double xv) { ww = ww * xv; };
                chain8v<false>(XR + (size_t)c * RS, m - p - 1, sstep);
                chain8v<false>(XR + (size_t)c * RS + VS, m - p - 1, pstep);
                fSR[c] = ss; fWR[c] = ww;
            }
        }
        __syncthreads();
        CST(2);
        const int jlo = __builtin_amdgcn_readfirstlane(slt[0][cb]), jhi = __builtin_amdgcn_readfirstlane(slt[0][cb + 1]);   // own columns j of acol1
        const int klo = __builtin_amdgcn_readfirstlane(slt[1][cb]), khi = __builtin_amdgcn_readfirstlane(slt[1][cb + 1]);   // own rows k of arow1
        const int nj = jhi - jlo, nk = khi - klo;
        double ma = 0.0, ba = -1.0, bv = 0.0; int bi = INT_MAX;
        // list lengths as wave-uniform values: the two searches of ttx_lottery_index2 then run a uniform number of steps
        const int nscu = __builtin_amdgcn_readfirstlane(nsc), nsru = __builtin_amdgcn_readfirstlane(nsr);
        const int nzcu = __builtin_amdgcn_readfirstlane(nzc), nzru = __builtin_amdgcn_readfirstlane(nzr);
        const int r1u = __builtin_amdgcn_readfirstlane(r1);
        for (int il = tid; il < nlot; il += CB) {
            const unsigned long long bil = (il == tid) ? bil0 : ttx_minstd_pow(2ull * il);
            const double d1 = ttx_flang_from_word(ttx_mulmod31(sA0, bil)), d2 = ttx_flang_from_word(ttx_mulmod31(sA1, bil));
            // (the lists hold at most r1 <= RM <= 64 entries on this path)
            const ttx_pair xy = ttx_lottery_index2<TTX_TABSEG, 64>(segc, nscu, Kc, r0 * n1, zc, nzcu, d1, segr, nsru, Kr, n2 * r2, zr, nzru, d2);
            const int x = xy.x, y = xy.y;
            CST(3);
            const int i = (x - 1) % r0 + 1, j = (x - 1) / r0 + 1, k = (y - 1) % n2 + 1, q = (y - 1) / n2 + 1;
            lot[4 * il] = i; lot[4 * il + 1] = j; lot[4 * il + 2] = k; lot[4 * il + 3] = q;
            const double *rl = XL + (size_t)(i - 1) * RS, *rq = XR + (size_t)(q - 1) * RS;
            double f;
            if constexpr (CFAST) f = f_ising_cfast(par[j - 1], par[n1m + j - 1], par[k - 1], par[n1m + k - 1], pRv[q - 1], pRk[q - 1], pLw[i - 1], pLk[i - 1], fSL[i - 1], fWL[i - 1], fSR[q - 1], fWR[q - 1]);
            else if constexpr (CPAD) f = f_ising_c4w(cA, cB, rl, rl + VS, par[j - 1], par[n1m + j - 1], par[k - 1], par[n1m + k - 1], rq, rq + VS, pRv[q - 1], pRk[q - 1], pLw[i - 1], pLk[i - 1]);
            else f = f_ising_c4p(m, p - 1, rl, rl + VS, par[j - 1], par[n1m + j - 1], par[k - 1], par[n1m + k - 1], rq, rq + VS, pRv[q - 1], pRk[q - 1], pLw[i - 1], pLk[i - 1]);
            ma = fmax(ma, fabs(f));
            CST(4);
            ClStrided lc(Cp, (i - 1) + (size_t)RM * (j - 1), P.SS), lw(Wq, (k - 1) + (size_t)NM * (q - 1), P.SW);
            double t = 0.0;
            cl_ordered_sum<8>(r1u, [&] { const double cv = lc(); return ClD2{cv, lw()}; }, [&](int, ClD2 e) { t = t + e.a * e.b; });
            const double b = f - t, aa = fabs(b);
            if (aa > ba || (aa == ba && il < bi)) { ba = aa; bv = b; bi = il; }
        }
        ma = wave_max_key(ma);
        wave_argmax2(ba, bv, bi);                      // (ba is |bv| or the start value, never a NaN: the same first maximum as wave_argmax)
        if (lane == 0) { shm[wv] = ma; sha[wv] = ba; shv[wv] = bv; shi[wv] = bi; }
        __syncthreads();
        ma = shm[0]; ba = sha[0]; bv = shv[0]; bi = shi[0];
        for (int x = 1; x < CB / 64; x++) {
            ma = fmax(ma, shm[x]);
            if (sha[x] > ba || (sha[x] == ba && shi[x] < bi)) { ba = sha[x]; bv = shv[x]; bi = shi[x]; }
        }
        amax = fmax(amax, ma);
        neval += nlot; rngpos += 2ull * nlot;
        sA0 = ttx_mulmod31(sA1, stepmul);
        if (bi == INT_MAX) bi = 0;                       // every residual a NaN: the first candidate, as idamax
        int ii = lot[4 * bi], jj = lot[4 * bi + 1], kk = lot[4 * bi + 2], qq = lot[4 * bi + 3];
        double pivot = bv;
        CST(5);
        // ---- rook half-steps (:516-582) / piv = 0 (:492-513): own slice, then one record per block ----
        int havecol = 0, haverow = 0, crs = 0, done = 0;
        int rc_k = -1, rc_q = -1, rr_i = -1, rr_j = -1;     // pivot at which resc / resr were computed (-1: not valid)
        const int H = (P.piv == 0) ? 2 : 2 * P.piv;
        double mxrun = 0.0;                                 // this wave's largest |value| over the half-steps of this bond step
        // Only the waves that own fiber elements at the current ranks (and wave 0 of every workgroup) take part in the rook loop and
        // its record exchange: at low ranks that is one wave per workgroup, and 24 idle waves polling the same four cache lines for
        // the whole evaluation delayed the records of the working ones (2900 cycles from the last store to the end of the poll,
        // against ~1000 in isolation: profiles/probes/probe_exchange.hip).  The others wait at the barrier behind the loop and take
        // the results from LDS.  wtab[c]: participating waves of workgroup c (cl_wact) -- the same number on every wave of the cluster.
        const bool rook_active = wv < wtab[cb];
        const bool slot_on = (lane < NB * (CB / 64)) && ((lane & (CB / 64 - 1)) < wtab[lane / (CB / 64)]);      // lane = record slot
        if (rook_active) {
        for (int h = 0; h < H && !done; h++) {
            // (the rook turn, the traffic count and the pivot taking below are this kernel's own copies of rook_turn,
            // halfstep_traffic and take_pivot of ttx_bondstep.h: through the shared functions the <false, false> instance
            // needs 262 registers instead of the 256 it has room for.  A change of those rules is made here as well.)
            const bool iscol = (P.piv == 0) ? (h == 0) : (((h + (dir == 2 ? 1 : 0)) & 1) == 0);
            const int nf = iscol ? r0 * n1 : n2 * r2;
            const int nsl = iscol ? r0 * nj : nk * r2;
            double *fib = iscol ? acol : arow;
            // The r1 factor entries at the current pivot, ONE PER LANE of every wave (r1 <= 64): requested here, consumed after the
            // evaluation (lane s of the wave supplies entry s to the ordered residual sum through v_readlane).  No LDS, no
            // workgroup barrier: the waves of a cluster run the rook loop independently and meet only in the record exchange.
            double xsv = 0.0;
            if (lane < r1) xsv = iscol ? Wq[(kk - 1) + (size_t)NM * (qq - 1) + P.SW * lane] : Cp[(ii - 1) + (size_t)RM * (jj - 1) + P.SS * lane];
            crs++;
            if (iscol) havecol = 1; else haverow = 1;
            const int dn = (P.piv == 0) ? (h == 1) : (havecol && haverow && (crs >= 2 * P.piv));
            const bool resid = (P.piv != 0) && !dn;
            if (iscol) { rc_k = resid ? kk : -1; rc_q = qq; } else { rr_i = resid ? ii : -1; rr_j = jj; }
            CST(6);
            WST(0);
            double mx = 0.0, ab = -1.0, bb = 0.0; int ix = INT_MAX;
            for (int u = tid; u < nsl; u += CB) {
                double a;
                if (iscol) {
                    const int i = u % r0, j = jlo + u / r0, t = i + r0 * j;
                    const double *rl = XL + (size_t)i * RS, *rq = XR + (size_t)(qq - 1) * RS;
                    if constexpr (CFAST) a = f_ising_cfast(par[j], par[n1m + j], par[kk - 1], par[n1m + kk - 1], pRv[qq - 1], pRk[qq - 1], pLw[i], pLk[i], fSL[i], fWL[i], fSR[qq - 1], fWR[qq - 1]);
                    else if constexpr (CPAD) a = f_ising_c4w(cA, cB, rl, rl + VS, par[j], par[n1m + j], par[kk - 1], par[n1m + kk - 1], rq, rq + VS, pRv[qq - 1], pRk[qq - 1], pLw[i], pLk[i]);
                    else a = f_ising_c4p(m, p - 1, rl, rl + VS, par[j], par[n1m + j], par[kk - 1], par[n1m + kk - 1], rq, rq + VS, pRv[qq - 1], pRk[qq - 1], pLw[i], pLk[i]);
                    fib[u] = a;
                    if (resid) {
                        double b = a;
                        cl_ordered_sum<16>(r1u, ClStrided(Cp, i + (size_t)RM * j, P.SS), [&](int s, double cv) { b = b + (-lane_get(xsv, s)) * cv; });
                        resc[u] = b;
                        const double aa = fabs(b);
                        if (aa > ab || (aa == ab && t < ix)) { ab = aa; bb = b; ix = t; }
                    }
                } else {
                    const int k = klo + u % nk, q = u / nk, t = k + n2 * q;
                    const double *rl = XL + (size_t)(ii - 1) * RS, *rq = XR + (size_t)q * RS;
                    if constexpr (CFAST) a = f_ising_cfast(par[jj - 1], par[n1m + jj - 1], par[k], par[n1m + k], pRv[q], pRk[q], pLw[ii - 1], pLk[ii - 1], fSL[ii - 1], fWL[ii - 1], fSR[q], fWR[q]);
                    else if constexpr (CPAD) a = f_ising_c4w(cA, cB, rl, rl + VS, par[jj - 1], par[n1m + jj - 1], par[k], par[n1m + k], rq, rq + VS, pRv[q], pRk[q], pLw[ii - 1], pLk[ii - 1]);
                    else a = f_ising_c4p(m, p - 1, rl, rl + VS, par[jj - 1], par[n1m + jj - 1], par[k], par[n1m + k], rq, rq + VS, pRv[q], pRk[q], pLw[ii - 1], pLk[ii - 1]);
                    fib[u] = a;
                    if (resid) {
                        double tt = 0.0;
                        cl_ordered_sum<16>(r1u, ClStrided(Wq, k + (size_t)NM * q, P.SW), [&](int s, double wv_) { tt = tt + wv_ * lane_get(xsv, s); });
                        const double b = a + (-1.0) * tt;
                        resr[u] = b;
                        const double aa = fabs(b);
                        if (aa > ab || (aa == ab && t < ix)) { ab = aa; bb = b; ix = t; }
                    }
                }
                mx = fmax(mx, fabs(a));
            }
            CST(7);
            WST(1);
            mx = wave_max_key(mx);
            if (resid) wave_argmax2(ab, bb, ix);         // (without a residual there is no arg-max: ix is not read)
            WST(2);
            // exchange: every WAVE publishes ONE tagged 16-byte record {|b|max, position, tag | sign} of its own elements and then
            // polls the 4 NB records of this half-step itself (L1-bypassing 16-byte loads, one per lane) and reduces them -- every
            // wave of the cluster arrives at the same result without a workgroup barrier.  A second record per exchange doubles its
            // cost (profiles/probes/probe_exchange.hip: 1.33 us per round with two records, 0.63 us with one, 0.49 us without the
            // sleep between polls), so the fiber maximum -- needed only by the acceptance test after the rook loop -- travels as a
            // RUNNING maximum in a record of its own that is stored here but read once, after the loop.  No fence: nothing but the
            // records crosses blocks here (fibers stay in LDS, factors were published at the end of earlier bond steps).  Records
            // are double-buffered by half-step parity (a wave cannot be two exchanges ahead of another: it needs that wave's record
            // of the exchange in between); the tag carries the launch number.
            // The turn that ends a full rook search (piv != 0, dn already true: evaluation only, no residual) has no arg-max to
            // agree on and stores ONLY its running-maximum record; it neither stores nor polls an arg-max record.  The poll of the
            // running maxima behind the loop waits for that very record of every participating wave, so it orders the waves as the
            // skipped poll did: a wave that has stored its running maximum of exchange L has finished polling exchange L-1, so
            // the parity buffers of exchange L+1 are free, and the closing cluster_sync separates the bond steps in any case.  The
            // exchange still counts (hcount): tags and parities go on as if it had taken place.  piv = 0 has no poll behind the
            // loop and keeps the stores and polls of both of its exchanges; like every turn without a residual it runs no arg-max
            // reduction around them (ab, ix keep their start values and nothing reads them).
            const bool xchg = resid || P.piv == 0;
            u4 *bufA = (u4 *)part + ((size_t)(hcount & 1) * P.G + g) * TTX_CLREC;
            u4 *bufB = bufA + (size_t)2 * P.G * TTX_CLREC;
            const unsigned gen = ((unsigned)epoch << 20) | (unsigned)(hcount + 1);
            mxrun = fmax(mxrun, mx);
            if (lane == 0) {
                const unsigned long long ua = (unsigned long long)__double_as_longlong(ab), um = (unsigned long long)__double_as_longlong(mxrun);
                u4 ra, rb;
                rb.x = (unsigned)um; rb.y = (unsigned)(um >> 32); rb.z = gen; rb.w = 0;
                st16(&bufB[cb * (CB / 64) + wv], rb);
                if (xchg) {
                    ra.x = (unsigned)ua; ra.y = (unsigned)(ua >> 32); ra.z = (unsigned)ix; ra.w = gen | (signbit(bb) ? 0x80000000u : 0u);
                    st16(&bufA[cb * (CB / 64) + wv], ra);
                }
            }
            CST(8);
            WST(3);
            int ok = 1;
            ab = -1.0; bb = 0.0; ix = INT_MAX;
            if (xchg && slot_on) {
                unsigned spins = 0;
                for (;;) {
                    const u4 ra = ld16(&bufA[lane]);
                    if ((ra.w & 0x7fffffffu) == gen) {
                        ab = __longlong_as_double((long long)(((unsigned long long)ra.y << 32) | ra.x));
                        ix = (int)ra.z;
                        bb = (ra.w & 0x80000000u) ? -ab : ab;
                        break;
                    }
                    if (++spins > 64u) __builtin_amdgcn_s_sleep(1);
                    if (spins > (1u << 22)) { ok = 0; break; }
                    if ((spins & 1023u) == 0 && __hip_atomic_load(P.cl_abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) { ok = 0; break; }
                }
            }
            WST(4);
            ok = __all(ok);
            if (resid) wave_argmax2(ab, bb, ix);
            WST(5);
            if (!ok) {                                   // aborted: the tail kernels of this sweep do nothing
                if (lane == 0) { __hip_atomic_store(P.cl_abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); P.ctl[0] = 1; *(volatile int *)&s_ok = 0; }
                return;
            }
            CST(9);
            hcount++;
            neval += nf;
            bytes_half += resid ? 8.0 * ((double)nf * r1 + r1 + 2.0 * nf) : 8.0 * nf;
            n_resid += resid ? 1 : 0;
            done = dn;
            if (resid) {
                if (ix == INT_MAX) ix = 0;
                if (iscol) { const int i = ix % r0 + 1, j = ix / r0 + 1; done = havecol && haverow && (i == ii && j == jj); ii = i; jj = j; }
                else       { const int k = ix % n2 + 1, q = ix / n2 + 1; done = havecol && haverow && (k == kk && q == qq); kk = k; qq = q; }
                pivot = bb;
            }
        }
        if (P.piv != 0) {            // the fiber maxima of the bond step (:531 / :564; the piv = 0 branch :492-513 does not touch amax):
            // the running maxima that every wave stored next to its record of the LAST exchange
            u4 *bufB = (u4 *)part + ((size_t)((hcount - 1) & 1) * P.G + g) * TTX_CLREC + (size_t)2 * P.G * TTX_CLREC;
            const unsigned gen = ((unsigned)epoch << 20) | (unsigned)hcount;
            double mx = 0.0; int ok = 1;
            if (slot_on) {
                unsigned spins = 0;
                for (;;) {
                    const u4 rb = ld16(&bufB[lane]);
                    if (rb.z == gen) { mx = __longlong_as_double((long long)(((unsigned long long)rb.y << 32) | rb.x)); break; }
                    if (++spins > 64u) __builtin_amdgcn_s_sleep(1);
                    if (spins > (1u << 22)) { ok = 0; break; }
                    if ((spins & 1023u) == 0 && __hip_atomic_load(P.cl_abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)) { ok = 0; break; }
                }
            }
            ok = __all(ok);
            if (!ok) {
                if (lane == 0) { __hip_atomic_store(P.cl_abort, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); P.ctl[0] = 1; *(volatile int *)&s_ok = 0; }
                return;
            }
            amax = fmax(amax, wave_max_key(mx));
        }
        if (tid == 0) {
            s_rook.ii = ii; s_rook.jj = jj; s_rook.kk = kk; s_rook.qq = qq; s_rook.hcount = hcount; s_rook.rc_k = rc_k; s_rook.rc_q = rc_q;
            s_rook.rr_i = rr_i; s_rook.rr_j = rr_j; s_rook.pivot = pivot; s_rook.amax = amax; s_rook.bytes_half = bytes_half; s_rook.neval = neval; s_rook.n_resid = n_resid;
        }
        }   // rook_active
        __syncthreads();
        if (!*(volatile int *)&s_ok) return;                // the working waves gave up (bounded wait expired) and have left
        if (!rook_active) {
            ii = s_rook.ii; jj = s_rook.jj; kk = s_rook.kk; qq = s_rook.qq; hcount = s_rook.hcount; rc_k = s_rook.rc_k; rc_q = s_rook.rc_q;
            rr_i = s_rook.rr_i; rr_j = s_rook.rr_j; pivot = s_rook.pivot; amax = s_rook.amax; bytes_half = s_rook.bytes_half; neval = s_rook.neval; n_resid = s_rook.n_resid;
        }
        CST(10);
        // ---- acceptance and in-place append (:598-758): every block appends its own slice ----
        int *tape = P.tape + ((size_t)g * (m + 2) + p) * 4;
        const bool upd = accept_pivot(pivot, amax, pivotmax_prev, P.small_element, P.small_pivot);
        if (!upd) {
            if (cb == 0 && tid == 0) { tape[0] = tape[1] = tape[2] = tape[3] = -1; P.upd[(size_t)g * (m + 2) + p] = 0; }
        } else {
            const int i0 = ii - 1, j0 = jj - 1, k0 = kk - 1, q0 = qq - 1;
            double *gI = inv_ptr(P, g, p, first);
            const bool reuseA = (rc_k == kk && rc_q == qq), reuseB = (rr_i == ii && rr_j == jj);    // block-uniform (s_rook)
            // role E, tables: the entries of the new pivot's column are requested here and stored behind role D, so that block 0
            // does not end its bond step with a dependent load (nobody reads the column before the closing cluster_sync)
            AppendTab tab{0, 0};
            if (cb == 0) tab = append_tables_fetch(P, g, p, first, ii, qq, tid);
            // The factor entries at the final pivot (the half-steps keep theirs in registers) go through LDS only where the
            // fall-back sums of roles A and B read them; where both residuals are reused, block 0's packed-LU copy is their one
            // reader and takes them from global memory -- no staging and no barrier in any block.
            // role E first part: packed LU from the OLD factors (:649-660)
            if (reuseA && reuseB) {
                if (cb == 0)
                    for (int s = tid; s < r1; s += CB) {
                        const double c = Wq[k0 + (size_t)NM * q0 + P.SW * s], w = Cp[i0 + (size_t)RM * j0 + P.SS * s];
                        gI[r1 * r1 + s] = w; gI[r1 * r1 + r1 + s] = c;
                    }
            } else {
                for (int s = tid; s < r1; s += CB) { xsc[s] = Wq[k0 + (size_t)NM * q0 + P.SW * s]; xsr[s] = Cp[i0 + (size_t)RM * j0 + P.SS * s]; }
                __syncthreads();
                if (cb == 0)
                    for (int s = tid; s < r1; s += CB) { gI[r1 * r1 + s] = xsr[s]; gI[r1 * r1 + r1 + s] = xsc[s]; }
            }
            // role A: arg(p), col(p) new slab (:662-668, :701)
            for (int u = tid; u < r0 * nj; u += CB) {
                const int i = u % r0, j = jlo + u / r0; const size_t o = i + (size_t)RM * j;
                const double a = acol[u];
                Ap[o + P.SS * r1] = a;
                double y;
                if (reuseA) y = resc[u];             // the same sum, in the same order, as the last column half-step
                else {
                    y = a;
                    ClStrided lc(Cp, o, P.SS); const double *xp = xsc;
                    cl_ordered_sum<16>(r1u, [&] { const double xv = *xp++; return ClD2{xv, lc()}; }, [&](int, ClD2 e) { y = y + (-e.a) * e.b; });
                }
                Cp[o + P.SS * r1] = (1.0 / pivot) * y;
            }
            // role B: arg(p+1), row(p+1) new row (:669-674, :702)
            for (int u = tid; u < nk * r2; u += CB) {
                const int k = klo + u % nk, q = u / nk;
                const double a = arow[u];
                Aq[r1 + (size_t)RM * k + P.SS * q] = a;
                const size_t o = k + (size_t)NM * q;
                if (reuseB) Wq[o + P.SW * r1] = resr[u];
                else {
                    double tt = 0.0;
                    ClStrided lw(Wq, o, P.SW); const double *xp = xsr;
                    cl_ordered_sum<16>(r1u, [&] { const double xv = *xp++; return ClD2{lw(), xv}; }, [&](int, ClD2 e) { tt = tt + e.a * e.b; });
                    Wq[o + P.SW * r1] = a + (-1.0) * tt;
                }
            }
            CST(11);
            // roles C and D are triangular solves along the rank index, one per own column j / row k.  A solve occupies
            // r0 (r2) lanes: with ranks up to 32 two of them share a wave (ttx_wave_solve.h, PK = 2).
            // role C: row(p)(:, j, r1+1) = L(p-1)^-1 acol1(:, j)  (:715-728)
            if (p > first) {
                const double *gL = ldsinv ? GL : inv_ptr(P, g, p - 1, first);
                double *Wp = core_ptr(P, P.row, g, p, first);
                const int pk = (r0 <= 32) ? 2 : 1, lw = 64 / pk, l = lane & (lw - 1), sub = lane / lw;
                for (int base = wv * pk; base < nj; base += (CB / 64) * pk) {
                    const int jl = base + sub, j = jlo + jl;
                    const bool on = (jl < nj) && (l < r0);
                    const double a = on ? acol[l + r0 * jl] : 0.0;
                    const double xf = (pk == 2) ? dev_solve_L<2>(gL, r0, a, l, sub) : dev_solve_L<1>(gL, r0, a, l, 0);
                    if (on) Wp[j + (size_t)NM * r1 + P.SW * l] = xf;
                }
            }
            CST(12);
            // role D: col(p+1)(r1+1, k, :) = arow1(k, :) U(p+1)^-1  (:730-749)
            if (p < last) {
                const double *gU = ldsinv ? GU : inv_ptr(P, g, p + 1, first);
                double *Cq = core_ptr(P, P.col, g, p + 1, first);
                const int pk = (r2 <= 32) ? 2 : 1, lw = 64 / pk, l = lane & (lw - 1), sub = lane / lw;
                const double rdg = dev_solve_rdg(gU, r2, l);
                for (int base = wv * pk; base < nk; base += (CB / 64) * pk) {
                    const int kl = base + sub, k = klo + kl;
                    const bool on = (kl < nk) && (l < r2);
                    const double y0 = on ? arow[kl + nk * l] : 0.0;
                    const double y = (pk == 2) ? dev_solve_U<2>(gU, r2, y0, rdg, l, sub) : dev_solve_U<1>(gU, r2, y0, rdg, l, 0);
                    if (on) Cq[r1 + (size_t)RM * k + P.SS * l] = y;
                }
            }
            CST(13);
            // role E: index tables, pivot set, scalars (:604-635)
            if (cb == 0) {
                append_tables_store(P, g, p, first, r1, ii, jj, kk, qq, tid, CB, tab);
                if (tid == 0) append_scalars(P, g, p, first, r1, ii, jj, kk, qq, pivot);
            }
            if ((zkeep & CL_ZKEEP) && wv < 2) {                     // keep the sorted distinct lists of this bond current:
                const int b = p - first;               // wave 0 inserts the pivot row, wave 1 the pivot column (RM <= 64)
                int *kl = ZK + (size_t)b * 2 * RM + (size_t)wv * RM;
                const int nl = ZN[2 * b + wv];
                const int key = wv == 0 ? ((jj << 16) | ii) : ((qq << 16) | kk);
                const int v = (lane < nl) ? kl[lane] : INT_MAX;
                const bool dup = __ballot(v == key) != 0ull;
                const int pos = __popcll(__ballot(v < key));
                if (!dup) {
                    if (lane < nl && v > key) kl[lane + 1] = v;      // every lane has read its entry before any lane writes
                    if (lane == 0) { kl[pos] = key; ZN[2 * b + wv] = nl + 1; }
                }
            }
            pivot_range(pivotmax, pivotmin, fabs(pivot));
        }
        CST(14);
        // end of the bond step: appends and the new rank become visible to the whole cluster (every block read r[] of
        // this step before its first half-step barrier, so block 0 may already have overwritten r[p])
        if (!cluster_sync(ctr, (++nbar) * (unsigned)NB, P.cl_abort, &s_ok)) { if (tid == 0) P.ctl[0] = 1; return; }
        CST(15);
        CST_END();
    }
    CSE_MARK();
    if (cb == 1) {
        // the left-going boundary message, beside block 0's list image, scalars and right-going message (cl_pack_block): all it reads lies
        // in front of the closing cluster_sync.  Reached, like block 0's exit, only by a launch that ran all its bond steps.
        const ClArgs *K = (const ClArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(K));
        if (cl_pack_block(CL_PACK_LEFT, K->NB, (K->zkeep & CL_PACK2) != 0) == 1) exch_pack_left(K->P, g);
        CSE(3);
    }
    if (cb == 0) {
        // what the next launch's entry takes instead of recomputing it: the pivot lists as they stand (the last insertion lies in front of
        // the closing cluster_sync) with this launch's number, and the generator word of the position written below.  Reached only by a
        // launch that ran all its bond steps: an abort, the stopping rule and ctl[0] return above.
        // (The arguments are read afresh from the kernel's argument block here: taken from the registers of the bond loop they lengthen
        // live ranges across it, and every instantiation spills 10 scalar registers more: profiles/cluster_entry_mi355x.txt.)
        const ClArgs *K = (const ClArgs *)__builtin_amdgcn_kernarg_segment_ptr();
        asm volatile("" : "+s"(K));
        if (K->zkeep & CL_ZCARRY) {
            const int ns = K->nsteps, rm = K->P.RM;
            int *img = cl_zimage(K->P, g, ns);
            for (int x = tid; x < nbonds * 2 * rm; x += CB) img[x] = ZK[x];
            for (int x = tid; x < 2 * nbonds; x += CB) img[(size_t)ns * 2 * rm + x] = ZN[x];
        }
        if (tid == 0) {
            gs.amax = amax; gs.pivotmax = pivotmax; gs.pivotmin = pivotmin; gs.neval = neval; gs.rngpos = rngpos;
            gs.bytes_half = bytes_half; gs.n_resid = n_resid;
            if (K->zkeep & CL_WORD) { gs.rngword = sA0; gs.rngword_pos = rngpos; }
            if (K->zkeep & CL_ZCARRY) gs.zk_epoch = K->epoch;
            if (P.tail_side) gs.amax_bnd[epoch & 1] = 0.0;      // the slot this sweep's tail launch raises (ttx_dev.h)
        }
        __syncthreads();
        // the group's outgoing boundary messages (saves the separate k_exch_pack launch): the left-going one only where block 1 does not
        exch_pack_right(P, g);
        if (cl_pack_block(CL_PACK_LEFT, K->NB, (K->zkeep & CL_PACK2) != 0) == 0) exch_pack_left(P, g);
        CSE(3);
        CSE_END();
    }
}
