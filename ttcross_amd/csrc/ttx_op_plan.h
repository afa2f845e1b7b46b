// ttx_op_plan.h -- what a call of an operation on the resident train reserves and launches, decided before anything is launched
// (host only: no HIP in here beyond the qualifiers of the formulas the kernels share).
//
// Every plan is a pure function of the train's shape (d, the mode sizes, the ranks, RM), of the device's CU count, of the call's
// arguments and of the chunk the engine read from the call's TTX_*_CHUNK variable.  The host functions of ttx_engine.hip check their
// arguments, build the plan, reserve its byte counts, upload tables and launch in its order; device pointers are theirs to fill in.
// tests/op_plan_main.cpp prints and checks plans on the CPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <math.h>
#include <algorithm>
#include <vector>

#include "../../include/ttx.h"      // TTX_EVAL_*
#include "ttx_contract.h"           // CtCore, CtTile (the kernels of these three are behind __HIPCC__)
#include "ttx_modeapply.h"          // MaCore, TTX_MA_*
#include "ttx_roundsum.h"           // RsBlk, TTX_RS_*
#include "ttx_qr_plan.h"            // TTX_LDS_DEVICE
#include "ttx_sq_norm.h"            // SqnCore, TTX_SQN_*
#include "ttx_sq_moments.h"         // TTX_SQM_*

#if defined(__HIPCC__)
#define TTX_OP_HD __host__ __device__ inline
#else
#define TTX_OP_HD inline
#endif

// ---- rules every operation shares ------------------------------------------------------------------------------------------------
inline bool op_mode_known(int mode) { return mode == TTX_EVAL_EXACT || mode == TTX_EVAL_MFMA || mode == TTX_EVAL_AUTO; }
// TTX_EVAL_AUTO takes the matrix cores where the call's work reaches the operation's break-even
inline int op_mode_eff(int mode, double work, double threshold) { return mode != TTX_EVAL_AUTO ? mode : work >= threshold ? TTX_EVAL_MFMA : TTX_EVAL_EXACT; }
// row tiles of 16 of the kernels instantiated for 1, 2, 4 and 8 (k_ev_gemm, k_tk_score_mfma; the squared samplers' quads are four times that)
inline int rank_tier(int r) { return r <= 16 ? 1 : r <= 32 ? 2 : r <= 64 ? 4 : 8; }
// one wave per item, 4 waves per workgroup, at most 8 workgroups per CU: the kernels stride over the rest
inline int wave_grid(long long items, int ncu) { return (int)std::min<long long>((items + 3) / 4, (long long)ncu * 8); }
// dynamic LDS of a launch; above the default ceiling of 64 KB the kernel's attribute has to be raised first
struct OpLds { size_t bytes = 0; bool raise = false; };
inline OpLds op_lds(size_t bytes) { OpLds l; l.bytes = bytes; l.raise = bytes > 64 * 1024; return l; }
// doubles of a point's state: the largest rank rounded up to four
inline int op_ldx(int d, const int *r) { return (std::max(1, *std::max_element(r, r + d + 1)) + 3) & ~3; }
// points per chunk of the batched evaluations where the environment names none
inline size_t op_chunk_default(int RM) { return RM <= 64 ? (size_t)1 << 18 : (size_t)1 << 17; }

// ---- ttx_ijk_batch, ttx_ijk_batch_dev, ttx_value_batch (ttx_eval.h) ----------------------------------------------------------------
#define TTX_EV_TP 256               // points per work item of k_ev_gemm: 4 waves x 4 column tiles of 16
#define TTX_EV_LDSHIST 8192         // modes up to this size are histogrammed in LDS
// leading dimension (doubles) of k_ev_gemm's slice image in LDS: rows rounded up to 16, and = 16 mod 32 so that the two k columns a
// half-wave reads (A[row l&15][k l>>4]) fall into different banks
TTX_OP_HD int ev_lda(int q0) { const int m = (q0 + 15) & ~15; return (m & 31) == 16 ? m : m + 16; }
TTX_OP_HD size_t ev_gemm_lds(int q0, int q1) { return sizeof(double) * (size_t)ev_lda(q0) * ((q1 + 3) & ~3); }

// TTX_EVAL_AUTO, a cost model fitted to the measurement in DESIGN.md 4.5, with w = sum r(k-1) r(k) (slice elements a point touches).
// The MFMA path pays a fixed cost whatever the batch (four launches per mode and the staging of the slices): 1.46 / 1.47 / 9.2 ms at
// (d, w) = (63, 6.8 k) / (63, 62 k) / (255, 1.04 M), modelled as 23 us d + 3.2 ns w.  Per point it saves 27.7 / 106 / 1317 ns against
// the exact kernel, modelled as 1.25 ps w + 0.286 ns d.  MFMA is taken where the saving covers the fixed cost; the model's break-evens
// are 55 k / 17 k / 6.7 k points on the three trains, the measured ones 52 k / 14 k / 7 k.
inline int ev_mode_eff(int mode, int d, const int *r, int64_t npts)
{
    double w = 0.0;
    for (int k = 1; k <= d; k++) w += (double)r[k - 1] * r[k];
    return op_mode_eff(mode, (double)npts * (1.25e-12 * w + 0.286e-9 * d), 23.0e-6 * d + 3.2e-9 * w);
}
enum EvStage { EV_ON_DEVICE, EV_HOST_INDEX, EV_HOST_COORD };   // caller's device pointers; host rows staged; host coordinates -> k_ev_digits
struct EvStep { int nmode = 0, q0 = 0, q1 = 0, tier = 1; size_t hist_lds = 0; OpLds lds; };    // 0-based mode i of the MFMA path: sort by index, k_ev_gemm<tier>
struct EvPlan {
    int eff = TTX_EVAL_EXACT, ldx = 4, ncu = 0;
    size_t chunk = 0;
    size_t b_ind = 0, b_out = 0, b_flag = 0, b_x = 0, b_xa = 0, b_xb = 0, b_sort = 0;   // bytes of SC_*; 0: the call does not use the slot
    size_t exact_lds = 0;                   // k_ev_exact: per wave x, z and the index row
    std::vector<EvStep> step;               // modes 0 .. d-2, walked from the last to the first
    // the grids of a chunk of c points
    int g_wave(int c) const { return wave_grid(c, ncu); }                                       // k_ev_exact, k_ev_init
    int g_sort(int c) const { return std::max(1, std::min((c + 1023) / 1024, 1024)); }          // k_ev_hist, k_ev_scatter
    int g_gemm(int i, int c) const { return c / TTX_EV_TP + std::min(step[i].nmode, c); }       // a work item per index and TTX_EV_TP of its points
    int g_final(int c) const { return std::max(1, std::min((c + 255) / 256, 1024)); }
};
// n[0 .. d-1], r[0 .. d]; NM: the engine's largest mode; dd: coordinates per point of EV_HOST_COORD; chunk: TTX_IJK_CHUNK or the default
inline EvPlan ev_plan(int d, const int *n, const int *r, int NM, int ncu, EvStage st, int64_t npts, int dd, int mode, size_t chunk)
{
    EvPlan p;
    p.eff = ev_mode_eff(mode, d, r, npts); p.ldx = op_ldx(d, r); p.ncu = ncu;
    p.chunk = std::min<size_t>(chunk, (size_t)std::max<int64_t>(npts, 0));
    if (!p.chunk) return p;                                                     // an empty call reserves and launches nothing
    // the chunk bounds the work space: the staging blocks of the host entries, two state buffers of chunk x ldx doubles and the sort on the MFMA path
    if (st != EV_ON_DEVICE) { p.b_ind = sizeof(int) * p.chunk * d; p.b_out = sizeof(double) * p.chunk; }
    if (st == EV_HOST_COORD) { p.b_flag = sizeof(int) * p.chunk; p.b_x = sizeof(double) * p.chunk * dd; }
    p.exact_lds = 4 * sizeof(double) * (2 * (size_t)p.ldx + (((size_t)d + 1) >> 1));
    if (p.eff != TTX_EVAL_MFMA) return p;
    p.b_xa = p.b_xb = sizeof(double) * p.chunk * p.ldx;
    p.b_sort = sizeof(int) * (2 * p.chunk + 4 * (size_t)NM + 8);                // valid, perm [chunk]; cnt [NM]; off, tile [NM + 1]; cur [NM]
    p.step.resize(d > 1 ? d - 1 : 0);
    for (int i = 0; i + 1 < d; i++) {
        EvStep &s = p.step[i];
        s.nmode = n[i]; s.q0 = r[i]; s.q1 = r[i + 1]; s.tier = rank_tier(s.q0);
        s.hist_lds = s.nmode <= TTX_EV_LDSHIST ? sizeof(int) * s.nmode : 0;
        s.lds = op_lds(ev_gemm_lds(s.q0, s.q1));
    }
    return p;
}

// ---- ttx_basis_batch, ttx_basis_tab and their _dev forms (ttx_basis.h) -------------------------------------------------------------
// break-even of TTX_EVAL_AUTO in flops per call (2 npts sum r0 n r1).  Measured (profiles/basis_mi355x.txt): on the coscoeff6 train
// (d = 6) exact wins at 2.1e8 flops and MFMA at 2.1e9; on the D_64 train (d = 63) MFMA wins at 6.3e8 already.  The value lies inside
// the first bracket and below the second figure.  Provisional for long chains: below 6.3e8 flops the D_64 crossover is not measured
// (both modes are then bound by their 2 d launches, not by the flops).
#define TTX_BS_AUTO_FLOPS 4.0e8
#define TTX_BS_KPAN 16              // columns k of a panel of k_bs_gemm
TTX_OP_HD constexpr int bs_ct(int MR) { return MR <= 2 ? 4 : MR <= 4 ? 2 : 1; }                // column tiles of 16 per wave
TTX_OP_HD size_t bs_gemm_lds(int q0) { return sizeof(double) * 2 * (size_t)ev_lda(q0) * TTX_BS_KPAN; }

enum BsSrc { BS_X_HOST, BS_X_DEV, BS_TAB_HOST, BS_TAB_DEV };
enum BsRefusal { BS_OK, BS_RANK, BS_BOUNDARY };                // ranks above 128; boundary ranks not 1
struct BsStep { int tier = 1, tp = 256; size_t lds = 0; };      // k_bs_gemm<tier> of a 0-based mode: 16 tier >= max(r0, r1), tp points per workgroup
struct BsPlan {
    BsRefusal refusal = BS_OK;
    int rmax = 1, eff = TTX_EVAL_EXACT, ldx = 4, ncu = 0;
    std::vector<size_t> off;                // where a mode's rows start in a point's row of the caller's table
    size_t sumn = 0, nmax = 1, chunk = 0, row = 0;                              // row: doubles per point of the input
    double flops = 0.0;
    size_t b_xa = 0, b_xb = 0, b_btab = 0, b_x = 0, b_out = 0;                  // bytes of SC_*; 0: the call does not use the slot
    size_t exact_lds = 0;                   // k_bs_exact: per wave x
    std::vector<BsStep> step;
    int g_exact(int c) const { return wave_grid(c, ncu); }
    int g_gemm(int i, int c) const { return (c + step[i].tp - 1) / step[i].tp; }
};
// n[0 .. d-1], r[0 .. d]; chunk: TTX_BASIS_CHUNK or the default
inline BsPlan bs_plan(int d, const int *n, const int *r, int ncu, BsSrc src, int64_t npts, int mode, size_t chunk)
{
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    BsPlan p;
    p.rmax = *std::max_element(r, r + d + 1); p.ncu = ncu;
    if (p.rmax > 128) { p.refusal = BS_RANK; return p; }
    if (r[0] != 1 || r[d] != 1) { p.refusal = BS_BOUNDARY; return p; }
    double w = 0.0;
    p.off.resize(d); p.step.resize(d);
    for (int k = 0; k < d; k++) {
        w += (double)r[k] * n[k] * r[k + 1];
        p.off[k] = p.sumn; p.sumn += (size_t)n[k]; p.nmax = std::max(p.nmax, (size_t)n[k]);
        BsStep &s = p.step[k];
        s.tier = (std::max(r[k], r[k + 1]) + 15) / 16; s.tp = 64 * bs_ct(s.tier); s.lds = bs_gemm_lds(r[k]);
    }
    p.flops = 2.0 * (double)npts * w;
    p.eff = op_mode_eff(mode, p.flops, TTX_BS_AUTO_FLOPS);
    p.ldx = op_ldx(d, r);
    p.chunk = std::min<size_t>(chunk, (size_t)std::max<int64_t>(npts, 0));
    if (src == BS_TAB_HOST) p.chunk = std::min(p.chunk, std::max<size_t>(1, ((size_t)1 << 25) / p.sumn));     // the staged rows of the caller's table
    p.row = tab ? p.sumn : (size_t)d;
    p.b_xa = p.b_xb = sizeof(double) * p.chunk * p.ldx;
    if (!tab) p.b_btab = sizeof(double) * p.chunk * p.nmax;
    if (!dev) { p.b_x = sizeof(double) * p.chunk * p.row; p.b_out = sizeof(double) * p.chunk; }
    p.exact_lds = 4 * sizeof(double) * (size_t)p.ldx;
    return p;
}

// ---- ttx_basis_grad_batch, ttx_basis_grad_tab and their _dev forms (ttx_basis_grad.h) ---------------------------------------------
// break-even of TTX_EVAL_AUTO in flops per call (6 npts sum r0 n r1).  PROVISIONAL: equal to TTX_BS_AUTO_FLOPS until the break-even of
// the gradient call itself is measured (profiles/basis_grad_mi355x.txt says what was and what was not).
#define TTX_BG_AUTO_FLOPS TTX_BS_AUTO_FLOPS
#define TTX_BG_LDT 20               // leading dimension of the forward step's panel image, (k, ac) at TTX_BG_LDT k + ac: 16 columns, and
                                    // 20 col + kq (col < 8, kq < 4) meets every residue mod 32 once
#define TTX_BG_STORE_DEFAULT ((size_t)1 << 32)      // bytes of the state store where TTX_BASIS_GRAD_STORE names none (provisional: 32768 points per chunk at S = 16 k)
// column tiles of 16 per wave of the backward step, whose accumulators are two sets (states 8 MR CT registers, accumulators 16 MR CT):
// chosen per tier from the compiler's resource report (profiles/basis_grad_mi355x.txt) so that no tier has scratch.  An a fragment from
// LDS already feeds two MFMAs per column tile, so the narrower tiles cost no LDS bandwidth that the matrix cores would wait for.  No tier
// needs a second pass for the dphi operand.  bg_waves: the waves per SIMD the register allocator is held to -- two wherever the kernel
// then still has no scratch.  The backward step of MR = 4 is the exception: with one column tile and two waves it spills (956 bytes per
// lane), so it keeps two column tiles and one wave (299 registers); MR >= 6 (forward: 7) needs more than 256 registers in any case.
TTX_OP_HD constexpr int bg_ct(int MR) { return MR <= 1 ? 4 : MR <= 4 ? 2 : 1; }
TTX_OP_HD constexpr int bg_waves(int MR, bool fwd) { return fwd ? (MR <= 6 ? 2 : 1) : (MR <= 3 || MR == 5) ? 2 : 1; }
TTX_OP_HD size_t bg_fwd_lds(int q1) { return sizeof(double) * 2 * (size_t)TTX_BG_LDT * ((q1 + 15) & ~15); }

// k_bg_gemm<tier, *> of a 0-based mode: 16 tier >= max(r0, r1); points per workgroup and LDS of the backward and of the forward step
struct BgStep { int tier = 1, tp_back = 256, tp_fwd = 256; size_t lds_back = 0, lds_fwd = 0; };
struct BgPlan {
    BsRefusal refusal = BS_OK;
    int rmax = 1, eff = TTX_EVAL_EXACT, ldx = 4, ncu = 0;
    std::vector<size_t> off;                // where a mode's rows start in a point's row of the caller's tables
    std::vector<size_t> soff;               // where a mode's row D_i starts among the S doubles of a point in the state store
    size_t sumn = 0, nmax = 1, S = 0, chunk = 0, row = 0;                       // row: doubles per point of the input (of each table)
    double flops = 0.0;
    size_t b_xa = 0, b_xb = 0, b_btab = 0, b_x = 0, b_out = 0, b_gst = 0;       // bytes of SC_*; 0: the call does not use the slot
    size_t lds_back = 0, lds_fwd = 0;       // k_bg_exact_back: per wave x; k_bg_exact_fwd: per wave l and D_i's row
    std::vector<BgStep> step;
    int g_exact(int c) const { return wave_grid(c, ncu); }
    int g_back(int i, int c) const { return (c + step[i].tp_back - 1) / step[i].tp_back; }
    int g_fwd(int i, int c) const { return (c + step[i].tp_fwd - 1) / step[i].tp_fwd; }
};
// n[0 .. d-1], r[0 .. d]; chunk: TTX_BASIS_CHUNK or the default; store: TTX_BASIS_GRAD_STORE or the default, bytes
inline BgPlan bg_plan(int d, const int *n, const int *r, int ncu, BsSrc src, int64_t npts, int mode, size_t chunk, size_t store)
{
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    BgPlan p;
    p.rmax = *std::max_element(r, r + d + 1); p.ncu = ncu;
    if (p.rmax > 128) { p.refusal = BS_RANK; return p; }
    if (r[0] != 1 || r[d] != 1) { p.refusal = BS_BOUNDARY; return p; }
    double w = 0.0;
    p.off.resize(d); p.soff.resize(d); p.step.resize(d);
    for (int k = 0; k < d; k++) {
        w += (double)r[k] * n[k] * r[k + 1];
        p.off[k] = p.sumn; p.sumn += (size_t)n[k]; p.nmax = std::max(p.nmax, (size_t)n[k]);
        p.soff[k] = p.S; p.S += (size_t)r[k];
        BgStep &s = p.step[k];
        s.tier = (std::max(r[k], r[k + 1]) + 15) / 16;
        s.tp_back = 64 * bg_ct(s.tier); s.tp_fwd = 64 * bs_ct(s.tier);
        s.lds_back = bs_gemm_lds(r[k]); s.lds_fwd = bg_fwd_lds(r[k + 1]);
    }
    p.flops = 6.0 * (double)npts * w;
    p.eff = op_mode_eff(mode, p.flops, TTX_BG_AUTO_FLOPS);
    p.ldx = op_ldx(d, r);
    // the store holds S doubles per point: the largest multiple of 256 points under the budget, at least one tile of 256
    const size_t fit = std::max<size_t>(256, store / (sizeof(double) * p.S) / 256 * 256);
    p.chunk = std::min<size_t>(std::min(chunk, fit), (size_t)std::max<int64_t>(npts, 0));
    if (src == BS_TAB_HOST) p.chunk = std::min(p.chunk, std::max<size_t>(1, ((size_t)1 << 25) / p.sumn));     // the staged rows of each of the caller's tables
    p.row = tab ? p.sumn : (size_t)d;
    p.b_xa = p.b_xb = sizeof(double) * p.chunk * p.ldx;
    p.b_gst = sizeof(double) * p.chunk * p.S;
    if (!tab) p.b_btab = sizeof(double) * 2 * p.chunk * p.nmax;                 // phi, then dphi
    if (!dev) { p.b_x = sizeof(double) * (tab ? 2 : 1) * p.chunk * p.row; p.b_out = sizeof(double) * p.chunk * ((size_t)d + 1); }    // val, then grad
    p.lds_back = 4 * sizeof(double) * (size_t)p.ldx; p.lds_fwd = 2 * p.lds_back;
    return p;
}

// ---- ttx_basis_core_grad_batch, ttx_basis_core_grad_tab and their _dev forms (ttx_basis_core_grad.h) -----------------------------
// break-even of TTX_EVAL_AUTO in flops per call (6 npts sum r0 n r1).  PROVISIONAL, NOT MEASURED: equal to TTX_BS_AUTO_FLOPS until the
// break-even of the core-gradient call itself is measured (profiles/basis_core_grad_mi355x.txt says what was and what was not).
#define TTX_CG_AUTO_FLOPS TTX_BS_AUTO_FLOPS
#define TTX_CG_PB 16                // points of a staged block of k_cg_gemm: four MFMA steps of four points
#define TTX_CG_WG 512               // workgroups a core's accumulation launch aims at (a constant, not the device's CU count: the
                                    // summation order of MFMA mode must not depend on the device)
#define TTX_CG_SEGMIN 256           // fewest points of a workgroup's segment of a chunk
// column tiles of 16 per wave of k_cg_gemm<MR> (the accumulators are 8 MR CT registers, nothing else is held across the point loop)
// and the waves per SIMD its register allocator is held to, from the compiler's resource report (profiles/basis_core_grad_mi355x.txt):
// no tier has scratch
TTX_OP_HD constexpr int cg_ct(int MR) { return MR <= 2 ? 4 : 2; }
TTX_OP_HD constexpr int cg_waves(int MR) { return MR <= 8 ? 2 : 1; }
// leading dimensions (doubles) of the staged rows: c L (= 16 mod 32, ev_lda), the table window of the workgroup's 64 CT columns
// (= 16 mod 32: the two point rows a half-wave reads fall into different banks) and the state X (odd: a half-wave's two broadcasts differ)
TTX_OP_HD constexpr int cg_lda(int MR) { return (16 * MR & 31) == 16 ? 16 * MR : 16 * MR + 16; }
TTX_OP_HD constexpr int cg_ldw(int MR) { return 64 * cg_ct(MR) + 16; }
TTX_OP_HD int cg_ldq(int q1) { return ((q1 + 3) & ~3) + 1; }
inline size_t cg_gemm_lds(int MR, int q1) { return sizeof(double) * TTX_CG_PB * ((size_t)cg_lda(MR) + cg_ldw(MR) + cg_ldq(q1)); }

// a 0-based mode's accumulation: k_cg_gemm<tier> on (ngrp, nsplit(c)) workgroups, 16 tier >= r0; seg points per workgroup
struct CgStep { int tier = 1, ngrp = 1, seg = TTX_CG_SEGMIN; size_t lds = 0, size = 0, goff = 0; };
struct CgPlan {
    BsRefusal refusal = BS_OK;
    int rmax = 1, eff = TTX_EVAL_EXACT, ldx = 4, ncu = 0;
    std::vector<size_t> off;                // where a mode's rows start in a point's row of the caller's table
    size_t sumn = 0, nmax = 1, S = 0, cap = 0, chunk = 0, row = 0;              // S: doubles per point of the state store; cap: the chunk before npts bounds it; chunk: the points per chunk
    size_t gsize = 0;                       // doubles of the packed gradient
    double flops = 0.0;
    size_t b_xa = 0, b_xb = 0, b_btab = 0, b_x = 0, b_out = 0, b_gst = 0, b_cgg = 0, b_part = 0;     // bytes of SC_*; 0: the call does not use the slot
    size_t lds_back = 0, lds_fwd = 0;       // k_bs_exact: per wave x; k_bg_exact_fwd: per wave l and a row it does not use here
    std::vector<BsStep> back;               // k_bs_gemm<tier> of the backward chain (bs_plan's)
    std::vector<BgStep> fwd;                // k_bg_gemm<tier, true> of the forward advance (bg_plan's)
    std::vector<CgStep> step;
    int g_exact(int c) const { return wave_grid(c, ncu); }
    int g_back(int i, int c) const { return (c + back[i].tp - 1) / back[i].tp; }
    int g_fwd(int i, int c) const { return (c + fwd[i].tp_fwd - 1) / fwd[i].tp_fwd; }
    int nsplit(int i, int c) const { return (c + step[i].seg - 1) / step[i].seg; }
    size_t soff(int i) const { return (size_t)(i - 1) * ldx; }                  // bond i = 1 .. d-1: X_i's block starts at soff(i) chunk doubles
};
// n[0 .. d-1], r[0 .. d]; chunk: TTX_BASIS_CHUNK or the default; store: TTX_BASIS_GRAD_STORE or the default, bytes; host_g: the
// gradient is the caller's host array.  The segments depend on the shapes and on the points per chunk only, never on the device.
inline CgPlan cg_plan(int d, const int *n, const int *r, int ncu, BsSrc src, bool host_g, int64_t npts, int mode, size_t chunk, size_t store)
{
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    CgPlan p;
    p.rmax = *std::max_element(r, r + d + 1); p.ncu = ncu;
    if (p.rmax > 128) { p.refusal = BS_RANK; return p; }
    if (r[0] != 1 || r[d] != 1) { p.refusal = BS_BOUNDARY; return p; }
    double w = 0.0;
    p.off.resize(d); p.back.resize(d); p.fwd.resize(d); p.step.resize(d);
    p.ldx = op_ldx(d, r);
    // the store holds X_1 .. X_(d-1) at the row stride of the value chain's kernels: the largest multiple of 256 points under the budget, at least 256
    p.S = (size_t)(d - 1) * p.ldx;
    const size_t fit = p.S ? std::max<size_t>(256, store / (sizeof(double) * p.S) / 256 * 256) : chunk;
    p.cap = std::max<size_t>(1, std::min(chunk, fit));
    for (int k = 0; k < d; k++) p.sumn += (size_t)n[k];
    p.chunk = std::min<size_t>(p.cap, (size_t)std::max<int64_t>(npts, 0));
    if (src == BS_TAB_HOST) p.chunk = std::min(p.chunk, std::max<size_t>(1, ((size_t)1 << 25) / p.sumn));     // the staged rows of the caller's table
    p.sumn = 0;
    for (int k = 0; k < d; k++) {
        w += (double)r[k] * n[k] * r[k + 1];
        p.off[k] = p.sumn; p.sumn += (size_t)n[k]; p.nmax = std::max(p.nmax, (size_t)n[k]);
        const int tb = (std::max(r[k], r[k + 1]) + 15) / 16;
        p.back[k].tier = tb; p.back[k].tp = 64 * bs_ct(tb); p.back[k].lds = bs_gemm_lds(r[k]);
        p.fwd[k].tier = tb; p.fwd[k].tp_fwd = 64 * bs_ct(tb); p.fwd[k].lds_fwd = bg_fwd_lds(r[k + 1]);
        CgStep &s = p.step[k];
        s.tier = (r[k] + 15) / 16;
        s.size = (size_t)r[k] * n[k] * r[k + 1]; s.goff = p.gsize; p.gsize += s.size;
        const size_t ncol = (size_t)n[k] * r[k + 1], wcol = (size_t)64 * cg_ct(s.tier);
        s.ngrp = (int)((ncol + wcol - 1) / wcol);
        const size_t want = std::max<size_t>(1, (size_t)TTX_CG_WG / (size_t)s.ngrp);
        s.seg = (int)std::max<size_t>(TTX_CG_SEGMIN, ((p.chunk + want - 1) / want + TTX_CG_PB - 1) / TTX_CG_PB * TTX_CG_PB);
        s.lds = cg_gemm_lds(s.tier, r[k + 1]);
    }
    p.flops = 6.0 * (double)npts * w;
    p.eff = op_mode_eff(mode, p.flops, TTX_CG_AUTO_FLOPS);
    p.row = tab ? p.sumn : (size_t)d;
    if (host_g) p.b_cgg = sizeof(double) * p.gsize;
    if (!p.chunk) return p;                                                     // an empty call launches no chain
    p.b_xa = p.b_xb = sizeof(double) * p.chunk * p.ldx;
    p.b_gst = sizeof(double) * p.chunk * p.S;
    if (!tab) p.b_btab = sizeof(double) * p.chunk * p.nmax;
    if (!dev) { p.b_x = sizeof(double) * p.chunk * (p.row + 1); p.b_out = sizeof(double) * p.chunk; }      // the rows, then c; val
    if (p.eff == TTX_EVAL_MFMA)
        for (int k = 0; k < d; k++) p.b_part = std::max(p.b_part, sizeof(double) * p.step[k].size * (size_t)p.nsplit(k, (int)p.chunk));
    p.lds_back = 4 * sizeof(double) * (size_t)p.ldx; p.lds_fwd = 2 * p.lds_back;
    return p;
}

// ---- ttx_basis_jvp_batch, ttx_basis_jvp_tab and their _dev forms, the vector operations (ttx_basis_jvp.h) -------------------------
// break-even of TTX_EVAL_AUTO in flops per call (6 npts sum r0 n r1).  PROVISIONAL, NOT MEASURED: equal to TTX_BS_AUTO_FLOPS until the
// break-even of the JVP itself is bracketed (profiles/basis_fit_mi355x.txt says what was and what was not measured).
#define TTX_JV_AUTO_FLOPS TTX_BS_AUTO_FLOPS
// column tiles of 16 per wave of k_jv_gemm<MR>, the row tiles a workgroup owns and the waves per SIMD its register allocator is held
// to, from the compiler's resource report (profiles/basis_fit_mi355x.txt): no tier has scratch.  A lane holds two states (16 MR CT
// registers) and two accumulator sets (16 MH CT).  An a fragment pair from LDS feeds 3 CT MFMAs, so CT = 2 is kept wherever it fits
// into the 512 registers of one wave per SIMD (MR <= 6; MR = 6 with its rows split over two workgroups); at MR = 7 and 8 the states
// alone are 224 / 256 registers per column tile pair, two column tiles spill (120 / 324 bytes per lane), and CT = 1 is taken
TTX_OP_HD constexpr int jv_ct(int MR) { return MR <= 1 ? 4 : MR <= 6 ? 2 : 1; }
TTX_OP_HD constexpr int jv_waves(int MR) { return MR <= 2 ? 2 : 1; }
// row tiles of 16 a workgroup owns: all MR up to 5; above, all rows spill even with one column tile, so the rows go to two workgroups
TTX_OP_HD constexpr int jv_mh(int MR) { return MR <= 5 ? MR : MR == 6 ? 3 : 4; }
// two buffers of two panel images (U's and V's) of a workgroup's rows
TTX_OP_HD size_t jv_gemm_lds(int q0, int MR) { return 2 * bs_gemm_lds(std::min(q0, 16 * jv_mh(MR))); }
// ttx_cores_dot: the buffer is cut into TTX_DOT_SEGS segments of dot_seg(tot) elements, a multiple of 256
#define TTX_DOT_SEGS 256
inline long long dot_seg(long long tot) { return 256 * ((tot + 65535) / 65536); }

struct JvStep { int tier = 1, tp = 256, gy = 1; OpLds lds; };           // k_jv_gemm<tier> of a 0-based mode: 16 tier >= max(r0, r1), tp points per workgroup, gy row groups
struct JvPlan {
    BsRefusal refusal = BS_OK;
    int rmax = 1, eff = TTX_EVAL_EXACT, ldx = 4, ncu = 0;
    std::vector<size_t> off;                // where a mode's rows start in a point's row of the caller's table
    std::vector<size_t> voff;               // where a mode's block starts in the packed direction
    size_t sumn = 0, nmax = 1, chunk = 0, row = 0, vsize = 0;                   // row: doubles per point of the input; vsize: doubles of the packed direction
    double flops = 0.0;
    size_t ystr = 0;                        // from a point's X row to its Y row in a state buffer: chunk ldx doubles
    size_t b_xa = 0, b_xb = 0, b_btab = 0, b_x = 0, b_out = 0, b_v = 0;         // bytes of SC_*; 0: the call does not use the slot
    size_t exact_lds = 0;                   // k_jv_exact: per wave x and y
    std::vector<JvStep> step;
    int g_exact(int c) const { return wave_grid(c, ncu); }
    int g_gemm(int i, int c) const { return (c + step[i].tp - 1) / step[i].tp; }
};
// n[0 .. d-1], r[0 .. d]; chunk: TTX_BASIS_CHUNK or the default; host_v: the direction is the caller's host array
inline JvPlan jv_plan(int d, const int *n, const int *r, int ncu, BsSrc src, bool host_v, int64_t npts, int mode, size_t chunk)
{
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    JvPlan p;
    p.rmax = *std::max_element(r, r + d + 1); p.ncu = ncu;
    if (p.rmax > 128) { p.refusal = BS_RANK; return p; }
    if (r[0] != 1 || r[d] != 1) { p.refusal = BS_BOUNDARY; return p; }
    double w = 0.0;
    p.off.resize(d); p.voff.resize(d); p.step.resize(d);
    for (int k = 0; k < d; k++) {
        w += (double)r[k] * n[k] * r[k + 1];
        p.off[k] = p.sumn; p.sumn += (size_t)n[k]; p.nmax = std::max(p.nmax, (size_t)n[k]);
        p.voff[k] = p.vsize; p.vsize += (size_t)r[k] * n[k] * r[k + 1];
        JvStep &s = p.step[k];
        s.tier = (std::max(r[k], r[k + 1]) + 15) / 16; s.tp = 64 * jv_ct(s.tier); s.lds = op_lds(jv_gemm_lds(r[k], s.tier));
        s.gy = (std::min((r[k] + 15) / 16, s.tier) + jv_mh(s.tier) - 1) / jv_mh(s.tier);                // row groups that hold rows of this mode
    }
    p.flops = 6.0 * (double)npts * w;
    p.eff = op_mode_eff(mode, p.flops, TTX_JV_AUTO_FLOPS);
    p.ldx = op_ldx(d, r);
    p.chunk = std::min<size_t>(chunk, (size_t)std::max<int64_t>(npts, 0));
    if (src == BS_TAB_HOST) p.chunk = std::min(p.chunk, std::max<size_t>(1, ((size_t)1 << 25) / p.sumn));     // the staged rows of the caller's table
    p.row = tab ? p.sumn : (size_t)d;
    p.ystr = p.chunk * p.ldx;
    if (!p.chunk) return p;                                                     // an empty call reserves and launches nothing
    p.b_xa = p.b_xb = sizeof(double) * 2 * p.ystr;
    if (!tab) p.b_btab = sizeof(double) * p.chunk * p.nmax;
    if (!dev) { p.b_x = sizeof(double) * p.chunk * p.row; p.b_out = sizeof(double) * 2 * p.chunk; }         // val, then dval
    if (host_v) p.b_v = sizeof(double) * p.vsize;
    p.exact_lds = 4 * sizeof(double) * 2 * (size_t)p.ldx;
    return p;
}

// ---- ttx_basis_enrich_batch, ttx_basis_enrich_tab and their _dev forms (ttx_basis_enrich.h) ----------------------------------------
// break-even of TTX_EVAL_AUTO in flops per call (EnPlan::flops).  PROVISIONAL, NOT MEASURED: equal to TTX_BS_AUTO_FLOPS until the two
// modes of the enrichment itself have been timed against each other (profiles/basis_enrich_mi355x.txt has the commands that give the
// crossing); TTX_ENRICH_AUTO_FLOPS in the environment replaces it
#define TTX_EN_AUTO_FLOPS TTX_BS_AUTO_FLOPS
#define TTX_EN_STORAGE (512 * 256)  // what maxrank * n of a new engine may reach: TTX_MAXPART * TTX_BLK of ttx_create_plan.h (ttx_engine.hip asserts it)
// point tiles of 16 per wave of k_en_z_gemm<QT> (the accumulators are 8 PT QT registers; a hashed b operand feeds PT MFMAs)
TTX_OP_HD constexpr int en_pt(int QT) { return QT <= 4 ? 4 : 2; }
// directions a bond takes: add, the complement of the left unfolding, the rows of the right unfolding, the engine's rank cap
inline int en_k(int add, int r0, int n, int r1, int n2, int r2)
{
    const long long comp = (long long)r0 * n - r1, right = (long long)n2 * r2;
    return (int)std::max<long long>(0, std::min(std::min<long long>(add, comp), std::min<long long>(right, 128 - r1)));
}
// bond b = 1 .. d-1 (between the 0-based modes b-1 and b): k_en_z_gemm<qt> on tp points per workgroup, then the accumulation launch of
// ttx_basis_core_grad.h with r1 = k (acc.goff: Y_b's start in the packed sketches); the QR of [U^L | Y] is rows x cols
struct EnStep { int k = 0, qt = 1, tp = 256, rows = 0, cols = 0; CgStep acc; };
struct EnPlan {
    BsRefusal refusal = BS_OK;
    int storage_bond = 0, storage_rank = 0; // a bond whose new rank times the largest mode is more than a new engine stores (0: none)
    CgPlan cg;                              // the pass structure: tables, backward and forward chain; ldx, S, chunk and the bytes are this call's
    int kmax = 0, eff = TTX_EVAL_EXACT;
    std::vector<EnStep> step;               // [d], entry b for bond b (entry 0 is not used)
    size_t ysize = 0;                       // doubles of the packed sketches Y_1 .. Y_(d-1)
    size_t b_y = 0, b_stat = 0, b_part = 0; // bytes: the sketches (then the new directions), the segment sums and maxima, the partial blocks
    double flops = 0.0;
    bool sketch = false;                    // any bond takes a direction and npts > 0: the passes run
    int g_z(int b, int c) const { return (c + step[b].tp - 1) / step[b].tp; }
    int nsplit(int b, int c) const { return (c + step[b].acc.seg - 1) / step[b].acc.seg; }
    size_t zoff() const { return (size_t)(cg.ldx) * (size_t)(step.size() - 1); }   // the chunk's z block starts at zoff chunk doubles of the state store
};
// n[0 .. d-1], r[0 .. d], add[0 .. d-2]; NM: the largest mode; chunk, store: as cg_plan's; auto_flops: the break-even in force
inline EnPlan en_plan(int d, const int *n, const int *r, const int32_t *add, int ncu, BsSrc src, int64_t npts, int mode, size_t chunk, size_t store,
                      double auto_flops = TTX_EN_AUTO_FLOPS)
{
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    EnPlan p;
    p.cg = cg_plan(d, n, r, ncu, src, false, npts, mode, chunk, store);
    p.refusal = p.cg.refusal;
    if (p.refusal != BS_OK) return p;
    CgPlan &g = p.cg;
    p.step.resize(d);
    int NM = 1;
    for (int k = 0; k < d; k++) NM = std::max(NM, n[k]);
    double w = 0.0, ws = 0.0;
    for (int k = 0; k < d; k++) w += (double)r[k] * n[k] * r[k + 1];
    for (int b = 1; b < d; b++) {
        EnStep &s = p.step[b];
        s.k = en_k(add[b - 1], r[b - 1], n[b - 1], r[b], n[b], r[b + 1]);
        if (!p.storage_bond && (long long)(r[b] + s.k) * NM > (long long)TTX_EN_STORAGE) { p.storage_bond = b; p.storage_rank = r[b] + s.k; }
        p.kmax = std::max(p.kmax, s.k);
        s.qt = rank_tier(std::max(s.k, 1)); s.tp = 64 * en_pt(s.qt);
        s.rows = r[b - 1] * n[b - 1]; s.cols = r[b] + s.k;
        s.acc.tier = (r[b - 1] + 15) / 16;
        s.acc.size = (size_t)s.rows * s.k; s.acc.goff = p.ysize; p.ysize += s.acc.size;
        ws += (double)s.k * ((double)n[b] * r[b + 1] + (double)s.rows);
    }
    if (p.storage_bond) return p;
    p.flops = (double)npts * (4.0 * w + 2.0 * ws);                              // the two chains; z and Y of every bond
    p.eff = op_mode_eff(mode, p.flops, auto_flops);
    g.eff = p.eff; g.flops = p.flops; g.b_cgg = 0; g.b_part = 0;
    p.b_y = sizeof(double) * std::max<size_t>(p.ysize, 1);
    p.b_stat = sizeof(double) * 2 * 256 * (size_t)(d - 1);
    p.sketch = p.kmax > 0 && npts > 0;
    // every state row -- X, L, z -- at one stride that also holds the k_i; the store takes X_1 .. X_(d-1) and the chunk's z block
    g.ldx = (std::max(g.rmax, p.kmax) + 3) & ~3;
    g.S = (size_t)d * g.ldx;
    const size_t fit = std::max<size_t>(256, store / (sizeof(double) * g.S) / 256 * 256);
    g.cap = std::max<size_t>(1, std::min(chunk, fit));
    g.chunk = std::min<size_t>(g.cap, (size_t)std::max<int64_t>(npts, 0));
    if (src == BS_TAB_HOST) g.chunk = std::min(g.chunk, std::max<size_t>(1, ((size_t)1 << 25) / g.sumn));
    if (!p.sketch) { g.chunk = 0; g.b_xa = g.b_xb = g.b_gst = g.b_btab = g.b_x = g.b_out = 0; return p; }
    g.b_xa = g.b_xb = sizeof(double) * g.chunk * g.ldx;
    g.b_gst = sizeof(double) * g.chunk * g.S;
    g.b_btab = tab ? 0 : sizeof(double) * g.chunk * g.nmax;
    g.b_x = dev ? 0 : sizeof(double) * g.chunk * (g.row + 1);                   // the rows, then c
    g.b_out = 0;
    g.lds_back = 4 * sizeof(double) * (size_t)g.ldx; g.lds_fwd = 2 * g.lds_back;
    for (int b = 1; b < d; b++) {
        EnStep &s = p.step[b];
        if (!s.k) continue;
        const size_t ncol = (size_t)n[b - 1] * s.k, wcol = (size_t)64 * cg_ct(s.acc.tier);
        s.acc.ngrp = (int)((ncol + wcol - 1) / wcol);
        const size_t want = std::max<size_t>(1, (size_t)TTX_CG_WG / (size_t)s.acc.ngrp);
        s.acc.seg = (int)std::max<size_t>(TTX_CG_SEGMIN, ((g.chunk + want - 1) / want + TTX_CG_PB - 1) / TTX_CG_PB * TTX_CG_PB);
        s.acc.lds = cg_gemm_lds(s.acc.tier, s.k);
        if (p.eff == TTX_EVAL_MFMA) p.b_part = std::max(p.b_part, sizeof(double) * s.acc.size * (size_t)p.nsplit(b, (int)g.chunk));
    }
    return p;
}

// ---- ttx_topk (ttx_topk.h) -----------------------------------------------------------------------------------------------------------
#define TTX_TK_KMAX 4096            // largest K
#define TTX_TK_SHEET (1 << 24)      // largest sheet K max n_k
#define TTX_TK_BINS 2048            // bins of a radix pass (11 bits)
#define TTX_TK_CHUNK 4096           // positions per workgroup of the compaction kernels: 1024 threads x 4
// TTX_EVAL_AUTO scores on the matrix cores from this many flops per call on.  Measured on the D_64 trains (profiles/topk_mi355x.txt):
// EXACT is faster at 2.0e8 and 8.1e8 flops per call, MFMA at 3.2e9 and 1.3e10; the break-even lies between 8.1e8 and 3.2e9
#define TTX_TK_AUTO_FLOPS 3.0e9
// the selection's state on the device, 64-bit words
enum { TKS_PREFIX, TKS_KREM, TKS_T, TKS_NEED, TKS_BOUND, TKS_NAN, TKS_WORDS = 8 };
typedef unsigned long long tk_u64;
TTX_OP_HD int tk_ldy(int r0) { return ((r0 + 15) & ~15) + 2; }     // = 2 or 18 mod 32: a half-wave's 16 columns x 2 rows meet 32 different bank pairs

struct TkStep {                             // 0-based mode k: the sheet of cnt[k + 1] x nI[k] pairs is scored, cnt[k] of them are kept
    int gx = 1, gy = 1, niper = 1, tier = 1;                                    // k_tk_score_mfma<tier> on (gx, gy), niper indices per workgroup
    OpLds lds;
    int g_exact = 1;                        // k_tk_score_exact
    bool radix = false;                     // more pairs than K: the six radix passes run, k_tk_hist on hg workgroups
    int hg = 0, nblk = 1, g_adv = 1;        // the compaction kernels, k_tk_advance
};
struct TkPlan {
    bool refused = false;                   // K times the largest mode is more than the score sheet holds
    int nmax = 1, eff = TTX_EVAL_EXACT, ldx = 4;
    // per mode (0-based): searched indices, the fixed index or -1, the sheet and the pairs kept; cnt[d] = 1, the empty suffix
    std::vector<int> nI, ifx, cnt;
    std::vector<long long> sheet;
    double flops = 0.0;
    size_t wmax = 1, smax = 1;
    size_t obytes = 0, b_kp = 0, b_kw = 0, b_ks = 0, b_kx = 0, b_krec = 0, b_ksel = 0, b_kout = 0;     // K rows of output; bytes of SC_K*
    std::vector<TkStep> step;
};
// n[0 .. d-1], r[0 .. d]; fixed (may be null): 0 or the 1-based index a mode is held at
inline TkPlan tk_plan(int d, const int *n, const int *r, int ncu, int K, const int32_t *fixed, int mode)
{
    TkPlan p;
    for (int k = 0; k < d; k++) p.nmax = std::max(p.nmax, n[k]);
    if ((long long)K * p.nmax > (long long)TTX_TK_SHEET) { p.refused = true; return p; }
    p.nI.resize(d); p.ifx.resize(d); p.cnt.assign(d + 1, 1); p.sheet.resize(d); p.step.resize(d);
    for (int k = d - 1; k >= 0; k--) {
        const int f = fixed ? fixed[k] : 0, r0 = r[k], r1 = r[k + 1];
        p.nI[k] = f ? 1 : n[k]; p.ifx[k] = f - 1;
        p.sheet[k] = (long long)p.cnt[k + 1] * p.nI[k];
        p.cnt[k] = (int)std::min<long long>(K, p.sheet[k]);
        p.flops += 2.0 * p.cnt[k + 1] * p.nI[k] * r0 * ((double)r1 + r0);
        p.wmax = std::max(p.wmax, (size_t)r0 * p.nI[k] * r1); p.smax = std::max(p.smax, (size_t)p.sheet[k]);
    }
    p.eff = op_mode_eff(mode, p.flops, TTX_TK_AUTO_FLOPS);
    p.ldx = op_ldx(d, r);
    for (int k = 0; k < d; k++) {
        TkStep &s = p.step[k];
        const long long M = p.sheet[k];
        s.gy = (p.cnt[k + 1] + 63) / 64;
        s.niper = (int)std::max<long long>(1, (long long)p.nI[k] * s.gy / (4ll * ncu));
        s.gx = (p.nI[k] + s.niper - 1) / s.niper;
        s.tier = rank_tier(r[k]);
        s.lds = op_lds(sizeof(double) * 64 * (size_t)tk_ldy(r[k]));
        s.g_exact = wave_grid(M, ncu);
        s.radix = M > K;
        s.hg = (int)std::min<long long>((M + 255) / 256, (long long)ncu * 4);
        s.nblk = (int)((M + TTX_TK_CHUNK - 1) / TTX_TK_CHUNK);
        s.g_adv = wave_grid(p.cnt[k], ncu);
    }
    p.obytes = (sizeof(int) * d + sizeof(double)) * (size_t)K;
    p.b_kp = sizeof(double) * (size_t)d * p.ldx * p.ldx; p.b_kw = sizeof(double) * p.wmax; p.b_ks = sizeof(tk_u64) * p.smax;
    p.b_kx = sizeof(double) * 2 * (size_t)K * p.ldx; p.b_krec = sizeof(int) * (size_t)d * K;
    p.b_ksel = sizeof(tk_u64) * (TKS_WORDS + TTX_TK_SHEET / TTX_TK_CHUNK) + sizeof(unsigned) * TTX_TK_BINS;
    p.b_kout = 2 * p.obytes;                                                    // [tval K][oval K][tind K d][oind K d]
    return p;
}

// ---- ttx_contract, ttx_marginals and the prefix vectors of the samplers (ttx_contract.h) -------------------------------------------
struct CtPlan {
    std::vector<CtCore> cores;          // every source core; src is the engine's to fill in
    std::vector<CtTile> tiles;          // mode-sum tiles of the contracted ones
    std::vector<int> r;                 // r(0:d)
    std::vector<size_t> moff;
    size_t msize = 0, wsize = 0;
    double bytes = 0.0;                 // 8 sum r0 n r1 over the contracted cores
};
// n[0 .. d-1], r[0 .. d]
inline void ct_plan(int d, const int *n, const int *r, const std::vector<char> &contracted, CtPlan &pl)
{
    pl.r.assign(r, r + d + 1);
    pl.cores.resize(d); pl.moff.assign(d, 0);
    for (int k = 0; k < d; k++) {
        CtCore &c = pl.cores[k];
        c.src = nullptr; c.r0 = r[k]; c.n = n[k]; c.r1 = r[k + 1];
        c.ta = 1; while (c.ta < 64 && c.ta < c.r0) c.ta <<= 1;
        c.woff = pl.wsize; pl.wsize += c.n;
        c.moff = 0;
        if (!contracted[k]) continue;
        c.moff = pl.moff[k] = pl.msize; pl.msize += (size_t)c.r0 * c.r1;
        pl.bytes += 8.0 * c.r0 * c.n * c.r1;
        const int tb = 256 / c.ta;
        for (int b0 = 0; b0 < c.r1; b0 += tb) for (int a0 = 0; a0 < c.r0; a0 += c.ta) pl.tiles.push_back(CtTile{k, a0, b0, 0});
    }
}

// ---- ttx_mode_apply, ttx_mode_apply_dev (ttx_modeapply.h) ---------------------------------------------------------------------------
struct MaPlan {
    std::vector<MaCore> app, cpy;       // the applied and the copied cores; src, dst and A are the engine's to fill in
    std::vector<int> app_k, cpy_k;      // the 0-based mode of every entry
    std::vector<size_t> aoff;           // of every applied mode's block in the matrices
    size_t asize = 0;
    long long tapp = 0, tcpy = 0;       // workgroups of k_ma_apply, k_ma_copy
    double rd = 0.0, wr = 0.0, fl = 0.0;
    int eff = TTX_EVAL_EXACT;
    bool refused = false;               // more workgroups than a launch takes
};
// n[0 .. d-1], r[0 .. d]; m[k]: 0 = mode k is left alone, or the rows of its matrix
inline MaPlan ma_plan(int d, const int *n, const int *r, const int32_t *m, int mode)
{
    MaPlan p;
    for (int k = 0; k < d; k++) {
        const bool applied = m[k] > 0;
        MaCore c{};
        c.r0 = r[k]; c.n = n[k]; c.r1 = r[k + 1]; c.m = applied ? m[k] : c.n;
        c.nab = (c.r0 + 15) / 16; c.npan = (c.m + TTX_MA_JP - 1) / TTX_MA_JP;
        c.ngrp = (int)(((long long)c.nab * c.r1 + TTX_MA_UNITS - 1) / TTX_MA_UNITS);
        long long &tiles = applied ? p.tapp : p.tcpy;
        c.first = tiles; tiles += (long long)c.ngrp * c.npan;
        if (applied) {
            p.aoff.push_back(p.asize); p.asize += (size_t)c.m * c.n;
            p.rd += 8.0 * c.r0 * c.n * c.r1 + 8.0 * c.m * c.n; p.wr += 8.0 * c.r0 * c.m * c.r1; p.fl += 2.0 * c.r0 * c.r1 * c.n * c.m;
        }
        (applied ? p.app : p.cpy).push_back(c); (applied ? p.app_k : p.cpy_k).push_back(k);
    }
    p.refused = p.tapp > 0x7fffffffll || p.tcpy > 0x7fffffffll;
    p.eff = op_mode_eff(mode, p.fl, TTX_MA_AUTO_FLOPS);
    return p;
}

// ---- ttx_lincomb_round (ttx_roundsum.h) ----------------------------------------------------------------------------------------------
struct RsPlan {
    std::vector<RsBlk> blks;            // [d][m], mode k at (k - 1) m; x, RM and SS -- where a term's core lies -- are the engine's to fill in
    std::vector<size_t> ooff, woff;     // Omega's cores [d + 1]; W(k) at woff[k], k = 1 .. d
    std::vector<long long> tS, tA;      // workgroups of mode k's sketch and advance launches
    size_t ymax = 1, mmax = 1, omax = 1;
    double fl = 0.0;
    int eff = TTX_EVAL_EXACT;
    long long refused = 0;              // the advance launch of a mode that has more workgroups than a launch takes, 0 if none
};
// n[0 .. d-1]; rt[t][0 .. d]: the ranks of term t; S[0 .. d]: their sums (m at both ends); l[0 .. d]: the sketch ranks
inline RsPlan rs_plan(int d, const int *n, int m, const int32_t *const *rt, const long long *S, const int32_t *l, int mode)
{
    RsPlan p;
    p.blks.resize((size_t)d * m); p.ooff.assign(d + 1, 0); p.woff.assign(d + 2, 0); p.tS.assign(d + 1, 0); p.tA.assign(d + 1, 0);
    p.mmax = (size_t)m;
    for (int k = 1; k <= d; k++) {
        const int nk = n[k - 1], l0 = l[k - 1], l1 = l[k];
        p.ooff[k] = p.ooff[k - 1] + (size_t)l0 * nk * l1;
        p.woff[k + 1] = p.woff[k] + (size_t)S[k] * l1;
        p.omax = std::max(p.omax, p.ooff[k] - p.ooff[k - 1]);
        p.ymax = std::max(p.ymax, (size_t)l0 * nk * (size_t)S[k]);
        p.mmax = std::max(p.mmax, (size_t)l1 * (size_t)S[k]);
        const int ntp = (l0 + 15) / 16;
        int o0 = 0, o1 = 0;
        for (int t = 0; t < m; t++) {
            RsBlk &B = p.blks[(size_t)(k - 1) * m + t];
            B = RsBlk{};
            B.r0 = rt[t][k - 1]; B.r1 = rt[t][k]; B.o0 = o0; B.o1 = o1;
            B.firstS = p.tS[k]; B.firstA = p.tA[k];
            p.tS[k] += (B.r0 + 15) / 16;
            p.tA[k] += (long long)ntp * (((long long)nk * B.r1 + 63) / 64);
            o0 += B.r0; o1 += B.r1;
            if (k >= 2) p.fl += 2.0 * B.r0 * nk * l1 * ((double)B.r1 + l0);     // the sketch step of mode k
            p.fl += 2.0 * l0 * B.r0 * nk * B.r1;                                // the advance into mode k
        }
        if (p.tA[k] > 0x7fffffffll) { p.refused = p.tA[k]; return p; }
        if (k < d) p.fl += 4.0 * l0 * nk * l1 * (double)S[k];                   // Z = Y W and M = Q^T Y
    }
    p.eff = op_mode_eff(mode, p.fl, TTX_RS_AUTO_FLOPS);
    return p;
}

// ---- ttx_sq_lognorm_grad (ttx_sq_norm.h) -------------------------------------------------------------------------------------------
// break-even of TTX_EVAL_AUTO in flops per call (sum 4 r0^2 n r1 + 6 r0 n r1^2).  PROVISIONAL until the two modes have been timed against
// each other on the device: profiles/sq_norm_mi355x.txt has the runs that give the crossing
#define TTX_SQN_AUTO_FLOPS 2.0e7
struct SqnPlan {
    BsRefusal refusal = BS_OK;
    int rmax = 0, eff = TTX_EVAL_EXACT, tier = 1;       // tier: rank_tier of the largest right rank, the instantiation of k_sqn_asm<true>
    size_t gsize = 0, nsum = 0;                         // doubles of g; sum n(k), the doubles of the md block (and of the mo block)
    std::vector<size_t> goff, proff, noff;              // [d + 1] core k's block in g and in W; PR_k in the PR store (k = 0 .. d; PR_0 is not formed); mode k's row in the md block
    std::vector<long long> first_e, first_wg;           // [d] SqnCore::first of the two assembly kernels
    long long tot_wg = 0;                               // workgroups of k_sqn_asm<true>
    unsigned grid_exact = 1;                            // workgroups of k_sqn_asm<false> (grid-stride)
    size_t b_w = 0, b_pr = 0, b_pl = 0, b_y = 0, b_part = 0, b_ex = 0, b_g = 0;      // bytes: the W store, the PR store, the two PL, Y, a step's partial matrices (n of them), the exponents, a host caller's g
    size_t lds_asm = sizeof(double) * TTX_SQN_KC * TTX_SQN_LDA;         // static LDS of k_sqn_asm<true>
    double flops = 0.0;
};
// n[0 .. d-1], r[0 .. d]
inline SqnPlan sqn_plan(int d, const int *n, const int *r, bool host_g, int mode)
{
    SqnPlan p;
    p.rmax = *std::max_element(r, r + d + 1);
    if (p.rmax > 128) { p.refusal = BS_RANK; return p; }
    if (r[0] != 1 || r[d] != 1) { p.refusal = BS_BOUNDARY; return p; }
    p.goff.assign(d + 1, 0); p.proff.assign(d + 2, 0); p.noff.assign(d + 1, 0); p.first_e.assign(d, 0); p.first_wg.assign(d, 0);
    size_t ymax = 1, pmax = 1;
    int r1max = 1;
    for (int k = 0; k < d; k++) {
        const size_t r0 = (size_t)r[k], nk = (size_t)n[k], r1 = (size_t)r[k + 1], sz = r0 * nk * r1;
        p.goff[k + 1] = p.goff[k] + sz;
        p.noff[k + 1] = p.noff[k] + nk;
        p.first_e[k] = (long long)p.goff[k];
        p.first_wg[k] = p.tot_wg;
        p.tot_wg += (long long)((r0 * nk + TTX_SQN_ROWS - 1) / TTX_SQN_ROWS);
        ymax = std::max(ymax, sz);
        pmax = std::max(pmax, nk * std::max(r0 * r0, r1 * r1));
        r1max = std::max(r1max, r[k + 1]);
        p.flops += 4.0 * (double)r0 * (double)r0 * (double)nk * (double)r1 + 6.0 * (double)r0 * (double)nk * (double)r1 * (double)r1;
    }
    for (int k = 0; k <= d; k++) p.proff[k + 1] = p.proff[k] + (size_t)r[k] * (size_t)r[k];
    p.gsize = p.goff[d]; p.nsum = p.noff[d];
    p.tier = rank_tier(r1max);
    p.grid_exact = (unsigned)std::min<size_t>((p.gsize + 255) / 256, 4096);
    p.b_w = sizeof(double) * p.gsize;
    p.b_pr = sizeof(double) * p.proff[d + 1];
    p.b_pl = sizeof(double) * 2 * (size_t)p.rmax * (size_t)p.rmax;
    p.b_y = sizeof(double) * ymax;
    p.b_part = sizeof(double) * pmax;
    p.b_ex = sizeof(int) * 2 * (size_t)(d + 1);
    p.b_g = host_g ? sizeof(double) * p.gsize : 0;
    p.eff = op_mode_eff(mode, p.flops, TTX_SQN_AUTO_FLOPS);
    return p;
}
// what the host forms from the chains' results (every step one double operation; numpy restates it): Z = z_mant 2^z_exp,
// den = z_mant + gvol 2^-z_exp, logz = z_exp ln 2 + log(den), s_k = ldexp((2 * coef) / den, eL(k-1) + eR(k) - z_exp)
inline int sqn_clamp_exp(long long e) { return (int)(e > 100000 ? 100000 : e < -100000 ? -100000 : e); }
inline double sqn_den(double z_mant, long long z_exp, double gvol) { return z_mant + ldexp(gvol, sqn_clamp_exp(-z_exp)); }
inline double sqn_logz(double z_mant, long long z_exp, double gvol) { return (double)z_exp * 0.6931471805599453 + log(sqn_den(z_mant, z_exp, gvol)); }
inline double sqn_scale(double z_mant, long long z_exp, double gvol, double coef, long long el, long long er)
{
    return ldexp((2.0 * coef) / sqn_den(z_mant, z_exp, gvol), sqn_clamp_exp(el + er - z_exp));
}

// ---- ttx_sq_moments (ttx_sq_moments.h) -----------------------------------------------------------------------------------------------
// break-even of TTX_EVAL_AUTO in flops per call (chains, right matrices, carried steps and band, SqmPlan::flops).  PROVISIONAL: measured
// (profiles/sq_moments_mi355x.txt), the batched exact kernels are faster than the present MFMA kernels on both trains timed, at 1.5e10 and
// at 3.6e12 flops, so no crossing has been seen and the value lies above both; TTX_SQM_AUTO_FLOPS in the environment replaces it
#define TTX_SQM_AUTO_FLOPS 1.0e13
// what the W buffer and the stored partial matrices of one batched launch may take.  An all-pairs call on d = 255, r = 64, n = 101 would
// want 0.8 GB for W alone; under the cap it is cut into batches of 38 carried matrices
#define TTX_SQM_CAP_BYTES ((size_t)256 << 20)
enum SqmRefusal { SQM_OK, SQM_RANK, SQM_BOUNDARY, SQM_NOTHING };        // SQM_NOTHING: every output null
struct SqmPlan {
    SqmRefusal refusal = SQM_OK;
    int rmax = 0, nmax = 1, eff = TTX_EVAL_EXACT;
    std::vector<int> sel;                               // the selected modes, 0-based, ascending (empty: no moments asked)
    std::vector<size_t> proff, noff;                    // [d + 2], [d + 1]: as SqnPlan's; the PL store has the PR store's layout
    size_t nsum = 0;
    long long steps = 0;                                // carried chain steps: sum over selected k below the largest of (l_max(k) - k)
    int members = 0, batch = 1;                         // the most carried matrices alive at once; members per launch
    size_t per_member = 0;                              // bytes of W and partial matrices of one member
    size_t ndots = 0;                                   // closing products: per selected l the pairs below it, m1 and the diagonal of c2
    size_t b_pr = 0, b_pl = 0, b_ex = 0, b_y = 0, b_part = 0, b_carry = 0, b_w = 0, b_cpart = 0, b_ra = 0, b_dots = 0, b_band = 0;
    double flops = 0.0;
    // members [first, first + count) of the launch number x over m alive members
    int cuts(int m) const { return (m + batch - 1) / batch; }
};
// n[0 .. d-1], r[0 .. d]; selected[k] != 0: mode k has an observable (null: no moments); want_band, want_mom: which outputs are asked;
// batch_env: TTX_SQM_BATCH (0: not set); auto_flops: the break-even in force
inline SqmPlan sqm_plan(int d, const int *n, const int *r, const unsigned char *selected, bool want_band, bool want_mom, bool want_z, int mode, long long batch_env,
                        double auto_flops = TTX_SQM_AUTO_FLOPS)
{
    SqmPlan p;
    p.rmax = *std::max_element(r, r + d + 1);
    if (p.rmax > 128) { p.refusal = SQM_RANK; return p; }
    if (r[0] != 1 || r[d] != 1) { p.refusal = SQM_BOUNDARY; return p; }
    if (!want_band && !want_mom && !want_z) { p.refusal = SQM_NOTHING; return p; }
    if (selected && want_mom) for (int k = 0; k < d; k++) if (selected[k]) p.sel.push_back(k);
    p.proff.assign(d + 2, 0); p.noff.assign(d + 1, 0);
    size_t ymax = 1, pmax = 1, p1max = 1;
    for (int k = 0; k < d; k++) {
        const size_t r0 = (size_t)r[k], nk = (size_t)n[k], r1 = (size_t)r[k + 1];
        p.noff[k + 1] = p.noff[k] + nk;
        p.nmax = std::max(p.nmax, n[k]);
        ymax = std::max(ymax, r0 * nk * r1);
        pmax = std::max(pmax, nk * std::max(r0 * r0, r1 * r1));
        p1max = std::max(p1max, r1 * r1);
        const double fw = 2.0 * (double)r0 * (double)r0 * (double)nk * (double)r1, fp = 2.0 * (double)r0 * (double)nk * (double)r1 * (double)r1;
        p.flops += 2.0 * (fw + fp);                                             // the two chains
        if (want_band) p.flops += fw + 2.0 * fp;                                // T, D0 and the band's brackets (at most)
    }
    for (int k = 0; k <= d; k++) p.proff[k + 1] = p.proff[k] + (size_t)r[k] * (size_t)r[k];
    p.nsum = p.noff[d];
    const int nsel = (int)p.sel.size(), smax = nsel ? p.sel.back() : -1;
    for (int x = 0; x < nsel; x++) {
        const int k = p.sel[x];
        const double fr = 2.0 * (double)r[k] * n[k] * r[k + 1] * ((double)r[k] + r[k + 1]);
        p.flops += 2.0 * fr;                                                    // RA and RA2
        p.ndots += 2 + (size_t)x;
        if (k == smax) continue;
        p.steps += smax - k;
        for (int j = k; j < smax; j++) p.flops += 2.0 * (double)r[j] * n[j] * r[j + 1] * ((double)r[j] + r[j + 1]);
    }
    p.members = nsel > 1 ? nsel - 1 : 0;
    p.eff = op_mode_eff(mode, p.flops, auto_flops);
    p.per_member = sizeof(double) * (ymax + (p.eff == TTX_EVAL_MFMA ? p1max : pmax));
    long long b = std::max<long long>(1, (long long)(TTX_SQM_CAP_BYTES / p.per_member));
    b = std::min<long long>(b, 65535 / p.nmax);                                 // k_sqm_p's grid: n members on the z axis
    if (batch_env >= 1) b = std::min(b, batch_env);
    p.batch = (int)std::max<long long>(1, std::min<long long>(b, std::max(1, p.members)));
    p.b_pr = p.b_pl = sizeof(double) * p.proff[d + 1];
    p.b_ex = sizeof(int) * 2 * (size_t)(d + 1);
    p.b_y = sizeof(double) * 2 * ymax;                                          // Y / W of an unbatched step; T and D0 of the band
    p.b_part = sizeof(double) * pmax;
    p.b_carry = sizeof(double) * 2 * (size_t)p.members * p.rmax * p.rmax + sizeof(int) * (size_t)std::max(1, p.members);
    p.b_w = p.members ? (size_t)p.batch * sizeof(double) * ymax : 0;
    p.b_cpart = p.members ? (size_t)p.batch * (p.per_member - sizeof(double) * ymax) : 0;
    p.b_ra = sizeof(double) * 2 * (size_t)p.rmax * p.rmax;
    p.b_dots = (sizeof(double) + sizeof(int)) * std::max<size_t>(1, p.ndots);
    p.b_band = want_band ? sizeof(double) * 2 * p.nsum : 0;
    return p;
}
// what the host forms from a product and its exponents: ldexp(dot / z_mant, e_left + e_right - z_exp), the exponent clamped
inline double sqm_ratio(double dot, double z_mant, long long el, long long er, long long z_exp) { return ldexp(dot / z_mant, sqn_clamp_exp(el + er - z_exp)); }
