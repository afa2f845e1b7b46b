// ttx_create_plan.h -- what an engine is made of, decided before anything is allocated (host only, no HIP in here).
//
// create_plan() is a pure function of the configuration, of the environment switches (CreateEnv) and of two figures of the
// device (DevCaps): the derived sizes, which kernel variants the engine may use, the dynamic LDS of each, or the refusal.  The
// cluster sweep kernel needs one more figure that only the runtime has, the occupancy of the chosen instantiation with the
// chosen LDS: the plan names a candidate, create_impl in ttx_engine.hip asks the runtime, and create_admit() takes or drops it
// and applies TTX_SWEEP.  The engine keeps the plan (ttx_engine::sel); chain_plan, run_impl and the accessors read it.
// tests/create_plan_main.cpp prints and checks plans on the CPU.
//
// The LDS formulas of the Ising D/E kernels (ttx_de.h includes this header) live here, one definition for both sides.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/ttx.h"
#include "ttx_dev.h"
#include "ttx_qr_plan.h"

#if defined(__HIPCC__)
#define TTX_PLAN_HD __host__ __device__ inline
#else
#define TTX_PLAN_HD inline
#endif

// ---- dynamic LDS of the Ising D/E kernels (ttx_de.h), in doubles, for m dimensions -------------------------------------------
#define DE5_W 4                  // waves of a k_halfstep_de5 relay
#define DE5_SEG 16               // columns of a row's body per wave and round
TTX_PLAN_HD size_t de5_lds_doubles(int m) { const int VS = ((m + 7) & ~7) + 8 + DE5_SEG; return (size_t)5 * VS + 128 + (size_t)DE5_W * 64; }
TTX_PLAN_HD bool de5_fits(int m) { return m >= 3; }
TTX_PLAN_HD int de_rows_stride(int m) { const int s = m + 56; return ((s + 31) & ~31) + 16; }
TTX_PLAN_HD size_t de_rows_lds_doubles(int m) { return (size_t)12 * de_rows_stride(m); }
TTX_PLAN_HD int det_vs(int m) { return ((m + 7) & ~7) + 8; }
TTX_PLAN_HD size_t det_lds_doubles(int m, int nbk) { return (size_t)4 * det_vs(m) + 256 + (det_vs(m) + 48) + (size_t)3 * nbk * 16 * 64; }

// figures of kernel headers that have HIP in them, restated; ttx_engine.hip holds them against the originals (static_assert)
constexpr int TTX_PLAN_FB = 1024;       // FB (ttx_fused.h): threads of the fused kernel
constexpr int TTX_PLAN_FNR = 24;        // TTX_FNR (ttx_fast.h)
constexpr int TTX_PLAN_MVN_MAXQ = 8;    // MVN_MAXQ (ttx_mvn.h)

// ---- what creation reads from outside -------------------------------------------------------------------------------------------
struct EnvText { bool set = false; std::string v; };        // a switch that is a word: kept as given, the plan words the refusal
// every environment switch of engine creation, parsed, with the defaults of an empty environment; create_env() of ttx_engine.hip,
// the one place of the create path that calls getenv, fills it through create_env_from
struct CreateEnv {
    EnvText arith;                  // TTX_ARITH = exact | fast
    EnvText sweep;                  // TTX_SWEEP = auto | chain | fused | cluster
    EnvText cl_pad;                 // TTX_CL_PAD = 0 | 1
    bool fullpiv_mfma = false;      // TTX_FULLPIV=mfma
    bool fast_persist_off = false;  // TTX_FAST_PERSIST=0
    bool de_lane = false;           // TTX_DE_LANE=1
    bool de_tables_off = false, de_fastdiv_off = false, de_cut_off = false, de_v2_off = false, de_team_off = false;   // TTX_DE_*=0
    bool de_lot_point_set = false; int de_lot_point = 0;    // TTX_DE_LOT_POINT (unset: on up to d = 160)
    int de_team_units = 256, de_team6_units = 1024;         // TTX_DE_TEAM_UNITS, TTX_DE_TEAM6_UNITS
    int de_test_fault = 0;          // TTX_DE_TEST_FAULT
    bool de_v5 = false;             // TTX_DE_V5=1
    int cluster_nb = 8;             // TTX_CLUSTER_NB
    bool cluster_coop = false;      // TTX_CLUSTER_COOP=1
    int cluster_test_abort = 0;     // TTX_CLUSTER_TEST_ABORT
    bool dbg_waves = false;         // TTX_DBG_WAVES (read by -DTTX_STAMPS builds only)
    bool lottery_one_block = false; // TTX_LOTTERY_NB=1
    bool lottery_wave_off = false;  // TTX_LOTTERY_WAVE=0
    bool lottery_rows2 = false;     // TTX_LOTTERY_ROWS=2
    bool mvn_v2_off = false;        // TTX_MVN_V2=0
    bool tail_off = false;          // TTX_TAIL=0
    bool tail_side_off = false;     // TTX_TAIL_SIDE=0
    bool head_direct_off = false;   // TTX_HEAD_DIRECT=0
    bool init_wave_off = false;     // TTX_INIT_WAVE=0
    bool fin_early_off = false;     // TTX_FIN_EARLY=0
    bool fin_skip_exch_off = false; // TTX_FIN_SKIP_EXCH=0
    bool init_wide_off = false;     // TTX_INIT_WIDE=0
    bool quad_lds_off = false;      // TTX_QUAD_LDS=0
    bool cl_powtab_off = false;     // TTX_CL_POWTAB=0
    bool cl_word_off = false;       // TTX_CL_WORD=0
    bool cl_lists_off = false;      // TTX_CL_LISTS=0
    EnvText tail_event;             // TTX_TAIL_EVENT = marker | kernel
    bool tail_lean_off = false;     // TTX_TAIL_LEAN=0
    bool cl_pack2_off = false;      // TTX_CL_PACK2=0
};
// the switches as `get` finds them (get(name): the value, or nullptr where unset): an integer as atoi reads it, "=0" as atoi(value) == 0
template <class Get>
CreateEnv create_env_from(Get get)
{
    auto text = [&](const char *name) { EnvText t; if (const char *e = get(name)) { t.set = true; t.v = e; } return t; };
    auto num = [&](const char *name, int dflt) { const char *e = get(name); return e ? atoi(e) : dflt; };
    auto off = [&](const char *name) { const char *e = get(name); return e && atoi(e) == 0; };
    CreateEnv v;
    v.arith = text("TTX_ARITH"); v.sweep = text("TTX_SWEEP"); v.cl_pad = text("TTX_CL_PAD");
    v.fullpiv_mfma = text("TTX_FULLPIV").v == "mfma";
    v.fast_persist_off = off("TTX_FAST_PERSIST");
    v.de_lane = num("TTX_DE_LANE", 0) == 1;
    v.de_tables_off = off("TTX_DE_TABLES"); v.de_fastdiv_off = off("TTX_DE_FASTDIV"); v.de_cut_off = off("TTX_DE_CUT");
    v.de_v2_off = off("TTX_DE_V2"); v.de_team_off = off("TTX_DE_TEAM");
    v.de_lot_point_set = get("TTX_DE_LOT_POINT") != nullptr; v.de_lot_point = num("TTX_DE_LOT_POINT", 0);
    v.de_team_units = num("TTX_DE_TEAM_UNITS", v.de_team_units); v.de_team6_units = num("TTX_DE_TEAM6_UNITS", v.de_team6_units);
    v.de_test_fault = num("TTX_DE_TEST_FAULT", 0);
    v.de_v5 = num("TTX_DE_V5", 0) == 1;
    v.cluster_nb = num("TTX_CLUSTER_NB", v.cluster_nb);
    v.cluster_coop = num("TTX_CLUSTER_COOP", 0) == 1;
    v.cluster_test_abort = num("TTX_CLUSTER_TEST_ABORT", 0);
    v.dbg_waves = get("TTX_DBG_WAVES") != nullptr;
    v.lottery_one_block = num("TTX_LOTTERY_NB", 0) == 1;
    v.lottery_wave_off = off("TTX_LOTTERY_WAVE");
    v.lottery_rows2 = num("TTX_LOTTERY_ROWS", 0) == 2;
    v.mvn_v2_off = off("TTX_MVN_V2");
    v.tail_off = off("TTX_TAIL"); v.tail_side_off = off("TTX_TAIL_SIDE");
    v.head_direct_off = off("TTX_HEAD_DIRECT"); v.init_wave_off = off("TTX_INIT_WAVE");
    v.fin_early_off = off("TTX_FIN_EARLY"); v.fin_skip_exch_off = off("TTX_FIN_SKIP_EXCH");
    v.init_wide_off = off("TTX_INIT_WIDE"); v.quad_lds_off = off("TTX_QUAD_LDS");
    v.cl_powtab_off = off("TTX_CL_POWTAB"); v.cl_word_off = off("TTX_CL_WORD"); v.cl_lists_off = off("TTX_CL_LISTS");
    v.tail_event = text("TTX_TAIL_EVENT"); v.tail_lean_off = off("TTX_TAIL_LEAN");
    v.cl_pack2_off = off("TTX_CL_PACK2");
    return v;
}
struct DevCaps { int ncu = 0; bool coop = false; };          // multiProcessorCount, hipDeviceAttributeCooperativeLaunch

enum SweepWant { SWEEP_AUTO, SWEEP_CHAIN, SWEEP_FUSED, SWEEP_CLUSTER };
enum SlotKind { SLOTS_NONE, SLOTS_HOST, SLOTS_DEVICE };      // two-pass integrands: no slots, pinned host slots, device slots

// the lottery's CDF segment tables for every K in 1..kmax (ttx_cdf.h), as DevProb::cdf_tab / cdf_ns take them
struct CdfTables { std::vector<ttx_cdfseg> tab; std::vector<int> ns; };

struct CreatePlan {
    int err = TTX_OK; std::string errtext;          // a refusal: nothing below it is meant to be used
    // ---- derived sizes ----
    int d = 0, RM = 0, NM = 0, W = 1, wrank = 0, nproc = 1, g0 = 0, G = 0, nbmax = 0, NC = 0, mode = 0, H = 0;
    std::vector<int32_t> own;                       // own[0..nproc]: first bond of every global group
    int ising_id = 0; bool isDE = false;            // Ising D or E: the long dependent chains of ttx_de.h
    double mvn_norm = 1.0;
    size_t SS = 0, SW = 0, CS = 0, XD = 0, IOFF = 0, MSZ = 0, QB = 0, SB = 0, VS = 0;
    int nfb = 0, nlotmax = 0;
    int nn = 0, snum = 0;                           // the initial cross: smallest mode size, samples
    SlotKind slots = SLOTS_NONE; size_t HS = 0;     // slots of one group of a two-pass integrand
    int cdf_kmax = -1;                              // the lottery's CDF tables reach up to this K (cdf_tables); -1: none, the kernels build the segments
    bool pfull = false, qscr = false;               // full pivoting's partial records; quadrature chain matrices in HBM
    // ---- arithmetic ----
    bool want_fast = false;                         // fast arithmetic was asked for (ttx_config.arith / TTX_ARITH); arith says where it is effective
    bool unit_nodes = false;                        // Ising: every node the integrand can read lies in [0,1]
    // DevProb's, as created.  arith of Ising C follows the cluster path (create_admit); where ttx_run retires that path it clears
    // DevProb::arith, which is what the kernels and ttx_arith read: ttx_engine::arith() gives the value in force
    int arith = 0, FD = 0, fpersist = 0;
    bool fast_tables = false;                       // the tables of a re-associated evaluator (fNear, fPiv, mvn: fDv, auxS)
    // ---- Ising D/E (ttx_de.h) ----
    int de_npair = 0;                               // > 0: pair-factor tables (deTL, deTR, deUL)
    int de_unit = 0, de_cut = 0;
    int de_slots = 0;                               // units of a wave-per-pivot half-step (also mvn_v2's)
    int de_v2 = 0;                                  // wave-per-pivot half-step k_halfstep_de / k_halfstep_dec
    int de_team = 0, de_team_units = 256, de_team6_units = 1024;    // teams of 14 waves (k_halfstep_det) up to de_team_units units, of 6 up to de_team6_units
    int de_v5 = 0;                                  // a relay of four waves (k_halfstep_de5)
    int de_test_fault = 0;                          // test hook: the team half-steps of that sweep get a grid of one unit
    int de_lot_point = 0;                           // unit-cut path: lottery candidates row-parallel without tables (k_lottery_eval_decp)
    int lot_wave = 0, lot_rows = 0;                 // lottery candidates by the row-wise wave evaluator; four per wave, 2: with factor tables
    size_t lds_de = 0, lds_det = 0, lds_det6 = 0, lds_de5 = 0, lds_der = 0;
    // ---- mvn (ttx_mvn.h) ----
    int mvn_v2 = 0; size_t lds_mvn = 0;             // wave-per-pivot half-step and wave-per-candidate lottery
    // ---- lottery ----
    int lot_nb = 1, bnd_wave = 0;
    bool lot_cand = false;                          // candidate lists lotc / lotf: the lottery runs as pick / evaluate / fold
    // ---- full pivoting ----
    int fp_mfma = 0, fp_tiles = 0;
    // ---- staging of the generic kernels ----
    size_t lds_par = 0, lds_half = 0, lds_lot = 0;
    int half_vals = 0, lot_vals = 0, fast_cap = 0;
    // ---- whole-sweep kernels (Ising C) ----
    size_t lds_fused = 0, lds_cluster = 0;
    bool fused_ok = false;
    int cluster_cand = 0;                           // workgroups per bond group the cluster kernel would run with; 0: not eligible
    int cluster_var = 0;                            // its instantiation: 0 exact, remainders predicated; 1 exact, rows padded to whole chunks; 2 closed form
    int cluster_ldsinv = 0, cluster_zkeep = 0, cluster_coop = 0;
    // the entry of a cluster launch (ttx_cluster.h): the generator's jump powers from a compile-time table (TTX_CL_POWTAB=0: three
    // square-and-multiply loops per launch), the generator word carried from the launch before (TTX_CL_WORD=0: raised from rngpos),
    // the sorted pivot lists carried through a global image (TTX_CL_LISTS=0, or no cluster_zkeep: rebuilt from vip per launch)
    bool cl_powtab = true, cl_word = true, cl_lists = false;
    int cl_test_abort = 0; bool dbg_waves = false;
    bool sweep_tail = true;                         // the pipelined cluster loop ends a sweep with k_exch_tail (TTX_TAIL=0: max/apply and boundary launches)
    bool sweep_tail_side = true;                    // ... and its summary runs on the quadrature's stream (TTX_TAIL_SIDE=0: k_sweep_end on the main stream)
    // the stretch between the last bond step of one sweep and the first of the next (profiles/sweep_gap_mi355x.txt)
    bool tail_event_kernel = true;                  // ev_tail is the tail launch's own completion signal (TTX_TAIL_EVENT=marker: an event recorded behind it)
    bool tail_lean = true;                          // boundary blocks request their header words together and the LU ahead of the corner (TTX_TAIL_LEAN=0: one by one)
    bool cl_pack2 = true;                           // the cluster kernel's exit packs the left-going message on block 1 (TTX_CL_PACK2=0: block 0 packs both)
    // the two ends of a run around its sweeps (ttx_loop_plan.h says where each applies)
    bool head_direct = true;                        // the initial summary goes from k_init_final into the pinned slot (TTX_HEAD_DIRECT=0: k_collect and a copy in front of sweep kernel 1)
    size_t lds_qtree = 0;                           // k_quad_tree multiplies in LDS: the bytes of its two regions of nproc matrices (quad_tree_lds); 0 (also TTX_QUAD_LDS=0): in the global scratch
    bool init_wide = true;                          // k_init_samples stages the mode sizes in LDS and takes the samples in one pass (TTX_INIT_WIDE=0: 256 threads, two passes)
    bool init_wave = true;                          // k_init_final runs one wave per core (TTX_INIT_WAVE=0: one thread per core)
    bool fin_early = true;                          // the finalisation waits for the last quadrature's k_quad_build only, its collect and copy go out before the host waits for the value (TTX_FIN_EARLY=0: behind the value's copy)
    bool fin_skip_exch = true;                      // no final exchange behind a sweep of one process, whose end has made it already (TTX_FIN_SKIP_EXCH=0: always)
    SweepWant sweep_want = SWEEP_AUTO; int ncu = 0;
    // decided by create_admit
    int fused = 0;                                  // whole-sweep kernel (ttx_fused.h) in use
    int cluster = 0;                                // workgroups per bond group of the cluster sweep kernel (ttx_cluster.h); 0: not used
};

// The launch of k_init_samples (ttx_init.h).  rows 0: the index rows of 256 threads do not fit the LDS, the generic accessor runs.
// rows 1: one row of VS shorts per thread behind the staged parameters, 256 threads -- the samples beyond 256 (408 with 8 groups at
// n = 51) take a second, part-empty pass, and every thread reads the mode sizes from global memory.  rows 2, where `wide` allows it
// and the kernel walks its own rows (own_rows: not the wave-per-sample evaluator of the fast Ising D/E, not the host's two passes):
// whole waves for all samples up to 512 threads, so one pass, and the d mode sizes staged once behind the rows.
// k_quad_tree in LDS: two regions of nproc RM x RM matrices, where they fit the working-set ceiling; one group has no tree
inline size_t quad_tree_lds(int nproc, size_t RM, bool on)
{
    const size_t need = sizeof(double) * 2 * (size_t)nproc * RM * RM;
    return on && nproc > 1 && need <= TTX_LDS_WORK ? need : 0;
}
struct InitSamplesPlan { int threads = 256, rows = 0; size_t lds = 0; };
inline InitSamplesPlan init_samples_plan(size_t lds_par, size_t VS, int d, long nsamples, bool own_rows, bool wide)
{
    InitSamplesPlan p;
    const size_t lds1 = lds_par + 16 + sizeof(short) * 256 * VS;
    p.rows = lds1 <= TTX_LDS_WORK ? 1 : 0;
    p.lds = p.rows ? lds1 : lds_par;
    if (!p.rows || !wide || !own_rows) return p;
    const int threads = (int)std::min<long>(512, std::max<long>(256, (nsamples + 63) / 64 * 64));
    const size_t lds2 = lds_par + 16 + sizeof(short) * (size_t)threads * VS + 16 + sizeof(int) * (size_t)(d + 1);
    if (lds2 <= TTX_LDS_WORK) { p.threads = threads; p.rows = 2; p.lds = lds2; }
    return p;
}

// lib/default.f90:78-97 share(): own(p) = first + int(dble(last-first+1)*dble(p)/nproc)
inline void share(int first, int last, int nproc, std::vector<int32_t> &own)
{
    own.assign(nproc + 1, 0);
    own[0] = first;
    for (int p = 1; p < nproc; p++) own[p] = first + (int)((double)(last - first + 1) * (double)p / nproc);
    own[nproc] = last + 1;
}
inline double powi(double a, int b)
{
    double r = 1.0;
    for (;;) { if (b & 1) r *= a; b /= 2; if (b == 0) break; a *= a; }
    return r;
}
// lottery CDF segment tables for every K that can occur (K <= kmax): pure function of K, see ttx_cdf.h; false: some K needs more
// than TTX_TABSEG segments
inline bool cdf_tables(int kmax, CdfTables &out)
{
    out.tab.assign((size_t)(kmax + 1) * TTX_TABSEG, ttx_cdfseg());
    out.ns.assign(kmax + 1, 0);
    std::vector<ttx_cdfseg> tmp(TTX_MAXSEG);
    for (int K = 1; K <= kmax; K++) {
        const int n_ = ttx_cdf_build(K, tmp.data());
        if (n_ > TTX_TABSEG) { out = CdfTables(); return false; }
        out.ns[K] = n_;
        memcpy(&out.tab[(size_t)K * TTX_TABSEG], tmp.data(), sizeof(ttx_cdfseg) * n_);
    }
    return true;
}
// whether cdf_tables serves kmax: a table is made for kmax <= 16384 where no K needs more than TTX_TABSEG segments.  A pure function
// of kmax that remembers how far it has looked, so that a process pays for each K once
inline bool cdf_table_fits(int kmax)
{
    static std::mutex mu;
    static int looked = 0, first_over = -1;             // K = 1..looked are known; the first K over TTX_TABSEG, if one was met
    if (kmax > 16384) return false;
    std::lock_guard<std::mutex> lk(mu);
    std::vector<ttx_cdfseg> tmp(TTX_MAXSEG);
    while (looked < kmax && first_over < 0) { looked++; if (ttx_cdf_build(looked, tmp.data()) > TTX_TABSEG) first_over = looked; }
    return first_over < 0 || kmax < first_over;
}

#if defined(__GNUC__)
__attribute__((format(printf, 3, 4)))
#endif
inline CreatePlan &plan_refuse(CreatePlan &p, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    p.err = code; p.errtext = buf;
    return p;
}

// cfg has passed the argument checks of create_impl (pointers, d, maxrank, pivoting, fun_id, par, nproc against d and world_size)
inline CreatePlan create_plan(const ttx_config &cfg, bool nofun, const CreateEnv &env, const DevCaps &caps)
{
    CreatePlan p;
    const int d = cfg.d, fun = cfg.fun_id, nproc = std::max(cfg.nproc, 1);
    p.d = d; p.RM = cfg.maxrank; p.nproc = nproc; p.ncu = caps.ncu;
    p.W = cfg.world_size < 1 ? 1 : cfg.world_size; p.wrank = cfg.world_rank;
    int NM = 1;
    for (int k = 0; k < d; k++) { if (cfg.n[k] < 1 || cfg.n[k] > 32000) return plan_refuse(p, TTX_EINVAL, "bad mode size"); NM = std::max(NM, cfg.n[k]); }
    p.NM = NM;
    if ((long long)p.RM * NM > (long long)TTX_MAXPART * TTX_BLK) return plan_refuse(p, TTX_EINVAL, "maxrank*n too large");
    if (cfg.mybonds) p.own.assign(cfg.mybonds, cfg.mybonds + nproc + 1);
    else share(1, d - 1, nproc, p.own);                                 // lib/dmrgg.f90:126-130
    for (int g = 0; g < nproc; g++) if (p.own[g + 1] <= p.own[g]) return plan_refuse(p, TTX_EINVAL, "mybonds: empty group %d", g);
    // the groups must tile the bonds 1 .. d-1 (own(0) = 1, own(nproc) = d, lib/default.f90:78-97): anything else would address
    // cores that do not exist or leave bonds without an owner
    if (p.own[0] != 1 || p.own[nproc] != d) return plan_refuse(p, TTX_EINVAL, "mybonds: must run from 1 to d = %d (got %d .. %d)", d, p.own[0], p.own[nproc]);
    // bond groups are dealt contiguously to the GPUs of the job
    p.g0 = (int)((long long)nproc * p.wrank / p.W);
    p.G = (int)((long long)nproc * (p.wrank + 1) / p.W) - p.g0;
    for (int g = 0; g < nproc; g++) p.nbmax = std::max(p.nbmax, p.own[g + 1] - p.own[g]);     // same launch shape on every GPU
    p.NC = p.nbmax + 1;
    p.mode = (cfg.pivoting == 0) ? 1 : (cfg.pivoting < 0) ? 2 : 0;
    p.H = (cfg.pivoting <= 0) ? 2 : 2 * cfg.pivoting;
    p.ising_id = (fun == TTX_FUN_ISING) ? (int)cfg.par[2 * cfg.n[0]] : 0;
    p.isDE = fun == TTX_FUN_ISING && p.ising_id != 1;
    if (fun == TTX_FUN_MVN) {
        if (cfg.naux < d + d * d + 1) return plan_refuse(p, TTX_EINVAL, "mvn: aux too short");
        p.mvn_norm = std::sqrt(powi(2.0 * 3.141592653589793, d) * cfg.aux[d + (size_t)d * d]);   // lib/mvn_pdf.f90:82
        if (!(p.mvn_norm > 0.0) || !std::isfinite(p.mvn_norm))
            return plan_refuse(p, TTX_EINVAL, "ttx_create: mvn normalisation sqrt((2 pi)^d det) = %g is not a positive finite number (det = %g under- or overflows at d = %d)",
                               p.mvn_norm, cfg.aux[d + (size_t)d * d], d);
    }
    const size_t RM = p.RM;
    const size_t VS = ((d + 7) & ~7) + 8;                               // doubles (or shorts) of a staged index row
    const int nlotmax = 2 * p.RM + 2 * NM;                              // most candidates of one lottery
    p.VS = VS; p.nlotmax = nlotmax;
    p.SS = RM * NM; p.SW = (size_t)NM * RM; p.CS = RM * NM * RM;
    p.nfb = (int)((RM * NM + TTX_BLK - 1) / TTX_BLK);
    p.XD = RM * NM + RM * RM;
    p.IOFF = (sizeof(int) * (XH + d + 2) + 15) & ~(size_t)15;
    p.MSZ = (p.IOFF + sizeof(double) * p.XD + 15) & ~(size_t)15;
    p.QB = (size_t)nproc * RM * RM + 2 * nproc;
    p.lds_qtree = quad_tree_lds(nproc, RM, !env.quad_lds_off);
    p.SB = SUM_HDR + nproc + 5 * (size_t)(d + 1);
    p.qscr = 2 * sizeof(double) * (RM * RM + 2) > TTX_LDS_WORK;
    p.nn = cfg.n[0];
    for (int k = 1; k < d; k++) p.nn = std::min(p.nn, cfg.n[k]);
    p.snum = std::max(8, nproc);

    // TTX_ARITH: exact (default) or fast; fast is effective where a re-associated evaluator exists (ttx_fast.h)
    bool want = cfg.arith == TTX_ARITH_FAST;
    if (cfg.arith != TTX_ARITH_EXACT && cfg.arith != TTX_ARITH_FAST) return plan_refuse(p, TTX_EINVAL, "ttx_create: arith must be TTX_ARITH_EXACT or TTX_ARITH_FAST (got %d)", cfg.arith);
    if (env.arith.set) {
        if (env.arith.v == "fast") want = true;
        else if (env.arith.v != "exact") return plan_refuse(p, TTX_EINVAL, "TTX_ARITH must be exact or fast (got %s)", env.arith.v.c_str());
    }
    p.want_fast = want && !nofun;
    // Ising: all nodes in [0,1] (every running product stays in [0,1] and is non-increasing: the cut at 2^-54 is valid, fdiv_unit
    // is exact).  The integrand reads node par[ind - 1] for ind up to the LARGEST mode size (lib: nodes + ind), whatever n(1) is
    bool unit = fun == TTX_FUN_ISING;
    for (int j = 0; unit && j < std::min(NM, (int)cfg.npar); j++) unit = cfg.par[j] >= 0.0 && cfg.par[j] <= 1.0;
    p.unit_nodes = unit;
    p.arith = (p.want_fast && ((p.isDE && unit) || fun == TTX_FUN_MVN)) ? 1 : 0;
    if (p.arith) {
        p.fast_tables = true;
        p.FD = d + 1;
        // tables per bond, kept for the whole run and extended incrementally (ttx_fast.h); TTX_FAST_PERSIST=0: mvn rebuilds the
        // tables of a bond step's two pivot sets with k_fast_tables instead (the first version, kept as a cross-check)
        p.fpersist = (fun == TTX_FUN_MVN && env.fast_persist_off) ? 0 : 1;
    }
    // Ising D/E, TTX_DE_LANE=1: one fiber element per lane, every pair by division, rows ended at the unit cut (f_ising_de with
    // `unit`): no tables, no teams
    if (p.isDE && !p.arith && env.de_lane) p.de_unit = unit;
    if (p.isDE && !p.arith && !env.de_lane && !env.de_tables_off) {
        p.de_npair = d * (d + 1) / 2;
        p.de_unit = unit && !env.de_fastdiv_off;
        // nodes in [0,1]: compact tables, every row of the pair triangle ends at the unit cut (k_de_ctables, k_halfstep_dec; same bits).
        // TTX_DE_CUT=0: the full tables and the kernels of round 2 (wave teams, row-wise lottery)
        p.de_cut = (p.de_unit && !env.de_cut_off) ? 1 : 0;
        p.de_lot_point = (env.de_lot_point_set ? env.de_lot_point : (int)(d <= 160)) != 0;
        p.de_slots = (int)RM * ((NM + 63) / 64);
        p.lds_de = sizeof(double) * (5 * VS + 256) + (p.de_cut ? sizeof(int) * VS : 0);
        p.de_v2 = cfg.pivoting >= 0 && p.de_slots <= TTX_MAXPART && p.lds_de <= TTX_LDS_WORK && !env.de_v2_off;
        p.lds_det = sizeof(double) * det_lds_doubles(d, 3);
        p.lds_det6 = sizeof(double) * det_lds_doubles(d, 1);
        p.de_team = p.de_v2 && !p.de_cut && p.lds_det <= TTX_LDS_WORK && !env.de_team_off;
        p.de_team_units = env.de_team_units;
        p.de_team6_units = env.de_team6_units;
        p.de_test_fault = env.de_test_fault;
        p.lds_de5 = sizeof(double) * de5_lds_doubles(d);
        p.de_v5 = p.de_v2 && !p.de_cut && de5_fits(d) && p.lds_de5 <= TTX_LDS_WORK && env.de_v5;
    }
    p.pfull = cfg.pivoting < 0;
    if (cfg.pivoting < 0 && env.fullpiv_mfma && RM <= 64 && (long long)(RM * NM) * (long long)(RM * NM) < (1LL << 31)) {
        // dense full pivoting: the whole superblock resident (8 (RM NM)^2 bytes per group: 21 MB at r=32, n=51; 334 MB at r=64, n=101)
        const size_t side = RM * NM;
        p.fp_mfma = 1; p.fp_tiles = (int)(((side + 63) / 64) * ((side + 63) / 64));
    }
    if (cdf_table_fits(p.RM * NM)) p.cdf_kmax = p.RM * NM;

    p.lds_par = sizeof(double) * (cfg.npar + 2);
    {   // half-step LDS: index rows always fit the limit checked below; value rows (Ising C fast path) where they fit
        const size_t base = sizeof(double) * (cfg.npar + RM + 4);
        const size_t idx_bytes = sizeof(short) * ((RM + 1) * VS + 16), val_bytes = sizeof(double) * ((RM + 1) * 2 * VS + 4);
        p.half_vals = (fun == TTX_FUN_ISING && p.ising_id == 1 && base + val_bytes <= TTX_LDS_VALUES) ? 1 : 0;
        p.lds_half = base + (p.half_vals ? val_bytes : idx_bytes);
        const size_t dif_bytes = sizeof(double) * ((RM + 1) * VS + 4);          // mvn: rows of differences x - mu
        if (fun == TTX_FUN_MVN && base + dif_bytes <= TTX_LDS_HALF_DIFF) { p.half_vals = 1; p.lds_half = base + dif_bytes; }
        if (p.arith) p.lds_half = std::max(p.lds_half, base + sizeof(double) * ((size_t)std::max(p.FD, TTX_PLAN_FNR) + 4 + RM + 2));   // far[] + cross terms
    }
    const size_t lot_hdr = sizeof(double) * (cfg.npar + 4) + sizeof(int) * 4 * (nlotmax + 4);
    {
        p.lds_lot = lot_hdr + sizeof(short) * (2 * RM * VS + 16);
        const size_t lot_dif = lot_hdr + sizeof(double) * (2 * RM * VS + 4);
        if (fun == TTX_FUN_MVN && lot_dif <= TTX_LDS_LOTTERY) { p.lot_vals = 1; p.lds_lot = lot_dif; }
        if (p.arith && fun == TTX_FUN_ISING) {
            // fast mode: the leading rows of the two decay tables ([row][RM] doubles each) instead of the index rows
            const size_t hdr = lot_hdr + 32;
            const size_t rowb = 2 * sizeof(double) * RM;
            p.fast_cap = (int)std::min<size_t>(std::min<size_t>(40, (size_t)d + 1), hdr < TTX_LDS_VALUES ? (TTX_LDS_VALUES - hdr) / rowb : 0);
            p.lds_lot = std::max(p.lds_lot, hdr + rowb * p.fast_cap);
        }
    }
    {   // whole-sweep kernels (Ising C): TTX_SWEEP = auto | chain | fused | cluster
        const bool fastc = fun == TTX_FUN_ISING && p.ising_id == 1 && cfg.pivoting >= 0 && p.cdf_kmax >= 0;
        // one 1024-thread workgroup per group: everything of a bond step in one CU's LDS
        p.lds_fused = sizeof(double) * (cfg.npar + 4 + 4 * RM * VS + 2 * RM * NM + RM + 4) + sizeof(int) * 4 * (nlotmax + 4);
        p.fused_ok = fastc && p.RM <= 64 && nlotmax <= TTX_PLAN_FB && p.lds_fused <= TTX_LDS_WORK;
        // a cluster of NB 256-thread workgroups per group, all resident at once (G*NB <= number of CUs)
        int NB = std::max(1, std::min(env.cluster_nb, TTX_CLMAX));
        while (NB > 1 && p.G * NB > caps.ncu / 2) NB--;                         // leave room for other processes on the card
        const size_t SL = RM * ((NM + NB - 1) / NB + 1);
        p.lds_cluster = sizeof(double) * (cfg.npar + 4 + 2 * RM * (2 * VS + 2) + 4 * SL + 2 * RM + 8) + sizeof(int) * 4 * (nlotmax + 4);
        if (p.lds_cluster + sizeof(double) * 2 * RM * RM <= TTX_LDS_WORK) { p.cluster_ldsinv = 1; p.lds_cluster += sizeof(double) * 2 * RM * RM; }
        const size_t zk = sizeof(int) * ((size_t)p.nbmax * 2 * RM + 2 * p.nbmax + 4);
        if (p.lds_cluster + zk <= TTX_LDS_WORK) { p.cluster_zkeep = 1; p.lds_cluster += zk; }
        p.cl_powtab = !env.cl_powtab_off; p.cl_word = !env.cl_word_off; p.cl_lists = p.cluster_zkeep && !env.cl_lists_off;
        // instantiation of the cluster kernel: the closed form where fast arithmetic was asked for; else rows padded to whole chunks
        // (f_ising_c4w) where the pad is neutral -- every node in [0,1], so that no running product overflows (inf * 0.0 is NaN) --
        // unless TTX_CL_PAD=0 asks for the predicated remainders (f_ising_c4p), which hold for any node (ttx_cluster_eval tells)
        const bool cfastc = p.want_fast && fun == TTX_FUN_ISING && p.ising_id == 1;
        if (env.cl_pad.set && env.cl_pad.v != "0" && env.cl_pad.v != "1") return plan_refuse(p, TTX_EINVAL, "TTX_CL_PAD must be 0 or 1 (got %s)", env.cl_pad.v.c_str());
        p.cluster_var = cfastc ? 2 : (unit && !(env.cl_pad.set && env.cl_pad.v == "0")) ? 1 : 0;
        // the candidate; its residency is create_admit's business
        if (fastc && p.RM <= 64 && NB >= 2 && p.G * NB <= caps.ncu && p.lds_cluster <= TTX_LDS_WORK) {
            p.cluster_cand = NB;
            // plain launch by default: with the occupancy gate every workgroup is placed as soon as the launch starts;
            // the cooperative launch (TTX_CLUSTER_COOP=1) adds the runtime's own refusal of oversized grids but costs
            // ~30 us per launch on this stack (C_64: 5.28 -> 5.80 ms per run, measured)
            p.cluster_coop = caps.coop && env.cluster_coop;
        }
        p.cl_test_abort = env.cluster_test_abort; p.dbg_waves = env.dbg_waves;
        p.sweep_tail = !env.tail_off; p.sweep_tail_side = !env.tail_side_off;
        if (env.tail_event.set && env.tail_event.v != "marker" && env.tail_event.v != "kernel")
            return plan_refuse(p, TTX_EINVAL, "TTX_TAIL_EVENT must be marker or kernel (got %s)", env.tail_event.v.c_str());
        p.tail_event_kernel = !(env.tail_event.set && env.tail_event.v == "marker");
        p.tail_lean = !env.tail_lean_off; p.cl_pack2 = !env.cl_pack2_off;
        p.head_direct = !env.head_direct_off; p.init_wave = !env.init_wave_off; p.init_wide = !env.init_wide_off;
        p.fin_early = !env.fin_early_off; p.fin_skip_exch = !env.fin_skip_exch_off;
        const std::string want_sweep = env.sweep.set ? env.sweep.v : "auto";
        if (want_sweep == "cluster") p.sweep_want = SWEEP_CLUSTER;
        else if (want_sweep == "fused") p.sweep_want = SWEEP_FUSED;
        else if (want_sweep == "auto") p.sweep_want = SWEEP_AUTO;
        else if (want_sweep == "chain") p.sweep_want = SWEEP_CHAIN;
        else return plan_refuse(p, TTX_EINVAL, "TTX_SWEEP must be auto, chain, fused or cluster (got %s)", want_sweep.c_str());
    }
    // an engine that only holds a train (nofun) never launches the half-step or the lottery: their staging does not bound its modes
    // (the lottery's header alone, 16 (2 RM + 2 NM) bytes, would refuse every train with a mode above about 3800)
    if (!nofun && (p.lds_half > TTX_LDS_DEVICE || p.lds_lot > TTX_LDS_LOTTERY)) return plan_refuse(p, TTX_EINVAL, "problem too large for LDS staging (d*maxrank)");
    {   // lottery: one wave of candidates per workgroup where one evaluation is a long dependent chain (Ising D/E, mvn)
        const bool heavy = p.isDE || fun == TTX_FUN_MVN;
        if (heavy && !env.lottery_one_block) p.lot_nb = std::min((nlotmax + 63) / 64, 64);
        if (p.lot_nb > 1 && (nlotmax + p.lot_nb - 1) / p.lot_nb > 64) p.lot_nb = 1;      // more candidates than 64 blocks x 64: keep one block
        if (fun == TTX_FUN_MVN && d <= 64 * TTX_PLAN_MVN_MAXQ && cfg.pivoting >= 0 && (int)RM * ((NM + 63) / 64) <= TTX_MAXPART && !env.mvn_v2_off) {
            p.lot_cand = true;
            p.mvn_v2 = 1; p.de_slots = (int)RM * ((NM + 63) / 64);
            p.bnd_wave = 1;
            p.lds_mvn = sizeof(double) * (3 * (size_t)d + 8);
        }
        if (p.isDE && p.arith) p.bnd_wave = 1;      // boundary corners by de_fast_point_wave
        if (p.isDE && p.de_npair) {
            p.lot_cand = true;
            // candidates and boundary corners by the row-wise wave evaluator (ttx_de.h); TTX_LOTTERY_WAVE=0: one lane per element
            p.lds_der = sizeof(double) * de_rows_lds_doubles(d);
            p.lot_wave = p.de_v2 && !p.de_cut && p.lds_der <= TTX_LDS_WORK && !env.lottery_wave_off;
            p.bnd_wave = p.lot_wave || (p.de_cut && p.de_v2 && p.lds_der <= TTX_LDS_WORK);      // boundary corners by one wave per corner
            p.lot_rows = p.lot_wave ? (env.lottery_rows2 ? 2 : 1) : 0;
        }
    }
    if (fun == TTX_FUN_HOST || fun == TTX_FUN_COSCOEFF || fun == TTX_FUN_DEVICE || fun == TTX_FUN_TRAINS || fun == TTX_FUN_PULLBACK) {
        // slots of one group: the largest point set any evaluating kernel asks for in one launch.  The host's `fun` reads pinned
        // slots; the others are evaluated on the stream between the two passes, from device slots
        p.HS = std::max<size_t>({RM * NM, (size_t)p.nn * p.snum, (size_t)p.NC * NM, (size_t)nlotmax, (size_t)2 * NM, (size_t)256});
        p.slots = fun == TTX_FUN_HOST ? SLOTS_HOST : SLOTS_DEVICE;
    }
    return p;
}

// The cluster candidate against what the device can hold of its kernel with its dynamic LDS (occ workgroups per CU, from
// hipOccupancyMaxActiveBlocksPerMultiprocessor; not read without a candidate): the grid may use half of it.  Then TTX_SWEEP.
inline void create_admit(CreatePlan &p, int occ)
{
    bool cluster_ok = p.cluster_cand != 0;
    if (cluster_ok) {
        const long long cap = (long long)occ * p.ncu;
        const long long grid = 8LL * p.cluster_cand * ((p.G + 7) / 8);
        if (grid * 2 > cap) cluster_ok = false;
    }
    if (p.sweep_want == SWEEP_CLUSTER) { if (cluster_ok) p.cluster = p.cluster_cand; }
    else if (p.sweep_want == SWEEP_FUSED) { if (p.fused_ok) p.fused = 1; }
    else if (p.sweep_want == SWEEP_AUTO) { if (cluster_ok) p.cluster = p.cluster_cand; else if (p.fused_ok && p.G == 1) p.fused = 1; }
    // TTX_ARITH=fast for Ising C: a closed form inside the cluster kernel (f_ising_cfast); the other paths evaluate C exactly
    if (p.cluster && p.cluster_var == 2) p.arith = 1;
}
