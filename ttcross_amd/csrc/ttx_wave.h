// ttx_wave.h -- the wave and workgroup primitives of every kernel of the engine, one copy each (wave = 64 lanes).
//
// Two families reach a wave-wide result, and both stay because they are different instructions:
//   * the DPP tree (wave_max, wave_argmax, wave_min_i, wave_max_i, wave_max_u): cross-lane operands of the VALU itself, no LDS
//     crossbar; six steps, the result in lane 63, broadcast by v_readlane;
//   * the xor butterfly (wave_sum_xor, wave_prod_xor, wave_max_xor): __shfl_xor over the offsets 32, 16, .. 1 (ds_bpermute), the
//     result in every lane.  A floating-point sum or product keeps this pairing order wherever it is used.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>

// one double of a wave, lane k wave-uniform: two v_readlane_b32 into a scalar pair, no LDS traffic
__device__ __forceinline__ double lane_get(double x, int k)
{
    const long long b = __double_as_longlong(x);
    const int lo = __builtin_amdgcn_readlane((int)b, k), hi = __builtin_amdgcn_readlane((int)(b >> 32), k);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// ---- the DPP tree -------------------------------------------------------------------------------------------------------------
// dpp_src<CTRL, ROWMASK>(old, x): x of the lane that the control word addresses; a lane the step does not address gets `old`
template <int CTRL, int ROWMASK>
__device__ __forceinline__ int dpp_src(int old, int x) { return __builtin_amdgcn_update_dpp(old, x, CTRL, ROWMASK, 0xf, false); }
template <int CTRL, int ROWMASK>
__device__ __forceinline__ unsigned dpp_src(unsigned old, unsigned x) { return (unsigned)__builtin_amdgcn_update_dpp((int)old, (int)x, CTRL, ROWMASK, 0xf, false); }
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_src(double old, double x)
{
    const long long b = __double_as_longlong(x), o = __double_as_longlong(old);
    const int lo = dpp_src<CTRL, ROWMASK>((int)o, (int)b), hi = dpp_src<CTRL, ROWMASK>((int)(o >> 32), (int)(b >> 32));
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// The tree: butterfly inside each row of 16 lanes (quad_perm xor 1, xor 2, row_ror 4, row_ror 8), then row_bcast:15 into rows 1
// and 3 and row_bcast:31 into rows 2 and 3; lane 63 holds the result.  step(DppStep<CTRL, ROWMASK>{}) performs one step.
template <int CTRL, int ROWMASK> struct DppStep { static constexpr int ctrl = CTRL, rowmask = ROWMASK; };
template <class STEP>
__device__ __forceinline__ void dpp_tree(STEP step)
{
    step(DppStep<0xb1, 0xf>{}); step(DppStep<0x4e, 0xf>{}); step(DppStep<0x124, 0xf>{});
    step(DppStep<0x128, 0xf>{}); step(DppStep<0x142, 0xa>{}); step(DppStep<0x143, 0xc>{});
}
// A lane that a step does not address gets the `old` operand of dpp_src.  Two forms are in use, both correct, and each reduction
// keeps the one it had: its own value (wave_max, wave_argmax: the operation is idempotent) or the identity of the operation
// (dpp_reduce: the integer trees of the cluster kernel).
template <class T, class OP>
__device__ __forceinline__ T dpp_reduce(T v, OP op, T ident)
{
    dpp_tree([&](auto s) { v = op(v, dpp_src<decltype(s)::ctrl, decltype(s)::rowmask>(ident, v)); });
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
    dpp_tree([&](auto s) { v = fmax(v, dpp_src<decltype(s)::ctrl, decltype(s)::rowmask>(v, v)); });
    return lane_get(v, 63);
}
// arg-max by the first-max rule of idamax: larger |.| wins, ties go to the lower index
__device__ __forceinline__ void wave_argmax(double &a, double &v, int &idx)
{
    dpp_tree([&](auto s) {
        constexpr int C = decltype(s)::ctrl, R = decltype(s)::rowmask;
        const double a2 = dpp_src<C, R>(a, a), v2 = dpp_src<C, R>(v, v);
        const int i2 = dpp_src<C, R>(idx, idx);
        if (a2 > a || (a2 == a && i2 < idx)) { a = a2; v = v2; idx = i2; }
    });
    a = lane_get(a, 63); v = lane_get(v, 63); idx = __builtin_amdgcn_readlane(idx, 63);
}
__device__ __forceinline__ int wave_min_i(int v)
{ return __builtin_amdgcn_readlane(dpp_reduce(v, [](int x, int y) { return min(x, y); }, INT_MAX), 63); }
__device__ __forceinline__ int wave_max_i(int v)
{ return __builtin_amdgcn_readlane(dpp_reduce(v, [](int x, int y) { return max(x, y); }, INT_MIN), 63); }
__device__ __forceinline__ unsigned wave_max_u(unsigned v)
{ return (unsigned)__builtin_amdgcn_readlane((int)dpp_reduce(v, [](unsigned x, unsigned y) { return max(x, y); }, 0u), 63); }

// ---- the xor butterfly: offsets 32, 16, .. 1, the result in every lane -----------------------------------------------------------
template <class OP>
__device__ __forceinline__ double wave_xor(double v, OP op)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_xor(double v) { return wave_xor(v, [](double x, double y) { return x + y; }); }
__device__ __forceinline__ double wave_prod_xor(double v) { return wave_xor(v, [](double x, double y) { return x * y; }); }
__device__ __forceinline__ double wave_max_xor(double v) { return wave_xor(v, [](double x, double y) { return fmax(x, y); }); }

// ---- inclusive scan over the lanes by __shfl_up: lane l gets x_0 + .. + x_l, added in ascending distance 1, 2, .. 32 ---------------
template <class T>
__device__ __forceinline__ T wave_scan(T c, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const T v = __shfl_up(c, o, 64); if (lane >= o) c = c + v; }
    return c;
}

// ---- workgroup reductions through LDS; sh.. hold blockDim/64 entries ---------------------------------------------------------------
// block max to every thread, on wave_max
__device__ __forceinline__ double block_max(double v, double *sh)
{
    v = wave_max(v);
    int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    double r = sh[0];
    for (int x = 1; x < nw; x++) r = fmax(r, sh[x]);
    return r;
}
// block arg-max; result valid in thread 0
__device__ __forceinline__ void block_argmax(double &a, double &v, int &idx, double *sha, double *shv, int *shi)
{
    wave_argmax(a, v, idx);
    int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sha[w] = a; shv[w] = v; shi[w] = idx; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int x = 1; x < nw; x++)
            if (sha[x] > a || (sha[x] == a && shi[x] < idx)) { a = sha[x]; v = shv[x]; idx = shi[x]; }
}
// block sum and block max of values >= 0 to every thread, on the xor butterfly, the waves' results folded from 0.0 in wave order
__device__ __forceinline__ double block_sum_xor(double v, double *sh)
{
    v = wave_sum_xor(v);
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    double r = 0.0;
    for (int x = 0; x < nw; x++) r += sh[x];
    return r;
}
__device__ __forceinline__ double block_max_xor(double v, double *sh)
{
    v = wave_max_xor(v);
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    double r = 0.0;
    for (int x = 0; x < nw; x++) r = fmax(r, sh[x]);
    return r;
}

// ---- maximum of non-negative doubles by their bit patterns, which order like unsigned integers ------------------------------------
__device__ __forceinline__ void atomic_max_pos(double *addr, double v)
{ atomicMax((unsigned long long *)addr, (unsigned long long)__double_as_longlong(v)); }
// the same order without the atomic: what atomic_max_pos(&a, b) would leave in a (a NaN's bit pattern is above every number's)
__device__ __forceinline__ double max_pos(double a, double b)
{ return ((unsigned long long)__double_as_longlong(b) > (unsigned long long)__double_as_longlong(a)) ? b : a; }
