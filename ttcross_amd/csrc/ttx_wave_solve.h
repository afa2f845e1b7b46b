// ttx_wave_solve.h -- the two triangular solves of the append along the rank index (lib/dmrgg.f90:715-749), one copy for every
// sweep kernel and for a host program (tests/wave_solve_main.cpp).
//
// Lane l of a solve holds entry l; lu is the packed LU of the neighbour bond (row l of L at lu[l*l + s], row l of U at
// lu[l*l + l + s], s < l; U(l,l) at lu[(l+1)*(l+1) - 1]).  Step s of the r steps takes the value of lane s and every lane l with
// s < l < r subtracts its multiple of it: r dependent steps.  PK = 1: one solve over the 64 lanes of a wave; PK = 2 (r <= 32):
// two solves of 32 lanes, `sub` = 0 / 1 names the half a lane belongs to.  Every lane of the wave calls them; lanes at or
// beyond the rank pass 0 and get nothing of use back.
//
// What a step must not wait for is taken off the chain:
//  - the value of lane s is a "value of lane k" operation lane(x, k), k wave-uniform: on the device two v_readlane_b32 into a
//    scalar pair (lane_get of ttx_wave.h; with PK = 2 one pair per half and a select), on the host an array lookup;
//  - the LU entries do not depend on the chain: a lane's WS_B entries of the next WS_B steps are requested while the current WS_B
//    steps run (lu(index, used): on the device a load, on the host a counted lookup).  A lane outside s < l < r requests a clamped
//    index inside the packed r x r block -- its own last entry, or entry 0 -- and never uses what comes back;
//  - the update is a select, not a branch: a lane outside s < l < r keeps its value, no zero product is added.
// Per lane the operations and their order are those of the plain substitution:  cand = (s == 0) ? a : a + (-1.0) * tmp,
// tmp = tmp + xs * L(l,s) in ascending s;  cand = rdg * y, y = y + (-U(l,s)) * ys.
#pragma once
#include "ttx_cdf.h"     // TTX_HD

#if defined(__clang__)      // (the host check is built by a compiler that does not know the pragma)
#define WS_UNROLL _Pragma("unroll")
#define WS_NO_UNROLL _Pragma("unroll 1")
#else
#define WS_UNROLL
#define WS_NO_UNROLL
#endif
#ifndef WS_B
#define WS_B 4            // LU entries a lane holds ahead, and steps per trip of the rolled loop; a power of two (1, 2 and 8
                          // measured the same on C_64: profiles/wave_solve_mi355x.txt)
#endif

// the lane's running request: entry s of its row (row = l*l for L, l*l + l for U), clamped into the row; lanes without a row ask for entry 0
#define WS_ROW(req, rowoff) \
    const bool inr_ = l > 0 && l < r; const int base_ = inr_ ? (rowoff) : 0, lim_ = inr_ ? l - 1 : 0; \
    auto req = [&](int s_) { return lu(base_ + (s_ < lim_ ? s_ : lim_), inr_ && s_ < l); }

// one step of either solve: the value of lane s (of this lane's half), then the update of the lanes behind it
template <int PK, class LANE>
TTX_HD double ws_lane_s(double cand, int s, int sub, LANE &lane)
{
    double v = lane(cand, s);
    if constexpr (PK == 2) { const double v1 = lane(cand, 32 + s); v = sub ? v1 : v; }
    return v;
}
template <int PK, class LANE>
TTX_HD void ws_step_L(int s, double e, double a, int upto, int sub, double &tmp, LANE &lane)
{
    const double cand = (s == 0) ? a : a + (-1.0) * tmp;
    const double xsv = ws_lane_s<PK>(cand, s, sub, lane);
    const double t = tmp + xsv * e;
    tmp = (s < upto) ? t : tmp;
}
template <int PK, class LANE>
TTX_HD void ws_step_U(int s, double e, double rdg, int upto, int sub, double &y, LANE &lane)
{
    const double cand = rdg * y;                           // only lane s's product is used: (1.0 / U(s,s)) * y_s
    const double ys = ws_lane_s<PK>(cand, s, sub, lane);
    const double t = y + (-e) * ys;
    y = (s < upto) ? t : y;
}
// The r steps: whole trips of WS_B steps while they last, the entries of the next trip requested in front of the first step;
// then pieces of WS_B/2 .. 1 steps by the bits of the wave-uniform remainder, out of the entries already held.  No test per step.
#define WS_STEPS(STEP) \
    double nx[WS_B]; \
    WS_UNROLL \
    for (int k = 0; k < WS_B; k++) nx[k] = req(k); \
    int s0 = 0; \
    WS_NO_UNROLL \
    for (; s0 + WS_B <= r; s0 += WS_B) { \
        double cur[WS_B]; \
        WS_UNROLL \
        for (int k = 0; k < WS_B; k++) { cur[k] = nx[k]; nx[k] = req(s0 + WS_B + k); } \
        WS_UNROLL \
        for (int k = 0; k < WS_B; k++) STEP(s0 + k, cur[k]); \
    } \
    const int rem = r - s0; \
    WS_UNROLL \
    for (int h = WS_B / 2; h >= 1; h >>= 1) \
        if (rem & h) {                                     /* wave-uniform */ \
            WS_UNROLL \
            for (int k = 0; k < h; k++) STEP(s0 + k, nx[k]); \
            WS_UNROLL \
            for (int k = 0; k + h < WS_B; k++) nx[k] = nx[k + h]; \
            s0 += h; \
        }

// role C, x = L^-1 a (:715-728, d2_luar)
template <int PK, class LU, class LANE>
TTX_HD double wave_solve_L(LU lu, int r, double a, int l, int sub, LANE lane)
{
    static_assert(PK == 1 || PK == 2, "one solve of 64 lanes or two of 32");
    WS_ROW(req, l * l);
    const int upto = (l < r) ? l : 0;                      // the steps s < upto change this lane's sum
    double tmp = 0.0;
#define WS_STEP_(s, e) ws_step_L<PK>(s, e, a, upto, sub, tmp, lane)
    WS_STEPS(WS_STEP_)
#undef WS_STEP_
    // x_l is the candidate of step l; the sum has not changed since (s < l only), so it is taken here and not by a select per step
    return (l == 0) ? a : a + (-1.0) * tmp;
}

// role D, y U^-1 (:730-749, d2_lual); rdg = wave_solve_rdg(lu, r, l): 1 / U(l,l) held by lane l, taken once for all solves against the same lu
template <class LU>
TTX_HD double wave_solve_rdg(LU lu, int r, int l)
{ return (l < r) ? 1.0 / lu((l + 1) * (l + 1) - 1, true) : 0.0; }
template <int PK, class LU, class LANE>
TTX_HD double wave_solve_U(LU lu, int r, double y, double rdg, int l, int sub, LANE lane)
{
    static_assert(PK == 1 || PK == 2, "one solve of 64 lanes or two of 32");
    WS_ROW(req, l * l + l);
    const int upto = (l < r) ? l : 0;
#define WS_STEP_(s, e) ws_step_U<PK>(s, e, rdg, upto, sub, y, lane)
    WS_STEPS(WS_STEP_)
#undef WS_STEP_
    // y_l is the candidate of step l, (1.0 / U(l,l)) * y; y has not changed since (s < l only)
    return (l < r) ? rdg * y : y;
}

#if defined(__HIPCC__)
#include "ttx_wave.h"    // lane_get
// the device's two operations, lane value and LU load (LDS or global), and the solves with them: dev_solve_*
struct WsLane { __device__ __forceinline__ double operator()(double x, int k) const { return lane_get(x, k); } };
struct WsLoad { const double *lu; __device__ __forceinline__ double operator()(int i, bool) const { return lu[i]; } };
template <int PK>
__device__ __forceinline__ double dev_solve_L(const double *lu, int r, double a, int l, int sub)
{ return wave_solve_L<PK>(WsLoad{lu}, r, a, l, sub, WsLane{}); }
__device__ __forceinline__ double dev_solve_rdg(const double *lu, int r, int l) { return wave_solve_rdg(WsLoad{lu}, r, l); }
template <int PK>
__device__ __forceinline__ double dev_solve_U(const double *lu, int r, double y, double rdg, int l, int sub)
{ return wave_solve_U<PK>(WsLoad{lu}, r, y, rdg, l, sub, WsLane{}); }
#endif
