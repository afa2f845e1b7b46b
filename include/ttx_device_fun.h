/*
 * ttx_device_fun.h -- write your own integrand for libttx.so as a HIP __device__ function.
 *
 * The reference's dtt_dmrgg(arg, fun, par, ...) takes ANY function of a multi-index (lib/dmrgg.f90:18).  An engine created
 * with fun_id = TTX_FUN_DEVICE (include/ttx.h) evaluates such a function on the GPU: you write it against this header,
 * compile the file to a gfx950 code object and hand the code object to ttx_set_integrand_device[_file].  This header needs
 * nothing but <hip/hip_runtime.h>; it is the only file of the engine an integrand author sees.
 *
 *     #include "ttx_device_fun.h"
 *     __device__ double myfun(int d, ttx_ind ind, const int *n, const double *par)
 *     {
 *         double s = 0.0;
 *         for (int k = 0; k < d; k++) s = s + par[ind[k] - 1];     // ind[k]: 1-based index of mode k+1, as the reference's ind(k+1)
 *         return 1.0 / (1.0 + s);
 *     }
 *     TTX_DEVICE_INTEGRAND(myfun)
 *
 *     hipcc --genco --offload-arch=gfx950 -O3 -ffp-contract=off -I <include> myfun.hip -o myfun.hsaco
 *     ttx_set_integrand_device_file(h, "myfun.hsaco", "myfun", par, npar);
 *
 * BIT REPRODUCIBILITY.  The sweep makes the pivot choices of the reference only if the device function returns, bit for bit,
 * what the host function would.  Compile with -ffp-contract=off (no fused multiply-add where the host rounds twice) and keep
 * the order of operations of the host code.  fp64 + - * / and sqrt() round as on the host (IEEE, round to nearest even);
 * exp / log / sin / cos / pow of the device library do NOT match glibc bit for bit -- an integrand that uses them gives a
 * valid cross approximation, but not the pivot sequence of a host run.  par is the engine's device copy of the array handed
 * to ttx_set_integrand_device; n is n(1:d).
 *
 * ---- the slot ABI (TTX_DEVFUN_ABI), written down once -----------------------------------------------------------------------
 *
 * Every kernel of the sweep that needs values of `fun` runs twice.  Pass 1 writes the multi-index of each element it wants
 * into a slot and raises the slot's flag; the SLOT KERNEL of the loaded integrand runs behind it on the same stream; pass 2
 * reads the values.  The macros below generate, for an integrand NAME, three symbols the loader looks up:
 *
 *   ttx_devfun_info_NAME   __device__ const ttx_devfun_info {abi, kind, block, lds_per_wave}; abi must equal the engine's
 *   ttx_devfun_slots_NAME  (int d, const int *n, const double *par, long long nslot,
 *                           const short *hidx, unsigned char *hreq, double *hval)
 *                          hidx[nslot][d]: 1-based indices (d <= 2048, mode sizes <= 32000); hreq[nslot]: one byte per slot,
 *                          non-zero = raised, 16-byte aligned; hval[nslot].  CONTRACT, for every slot s with hreq[s] != 0:
 *                          write hval[s] = fun(hidx[s][:]), THEN clear hreq[s]; touch no other slot's value or flag; make no
 *                          assumption about the grid size (any number of workgroups must cover all nslot slots).
 *   ttx_devfun_list_NAME   (int d, const int *n, const double *par, long long npts, const int *ind, double *out)
 *                          ind[npts][d] 1-based ints; out[p] = fun(ind[p][:])  (ttx_eval_device)
 *
 * The ENGINE chooses the launch shape from nslot: workgroups of TTX_DEVFUN_BLOCK threads (the macros assume exactly this
 * block size), a 1-D grid (lane form: one lane per slot; wave form: one wave per slot; both capped,
 * the kernels stride), and lds_per_wave * TTX_DEVFUN_WAVES bytes of dynamic LDS (at most 64 KB per workgroup).
 */
#ifndef TTX_DEVICE_FUN_H
#define TTX_DEVICE_FUN_H
#include <hip/hip_runtime.h>

#define TTX_DEVFUN_ABI 1
#define TTX_DEVFUN_BLOCK 256                        /* threads per workgroup of every generated kernel */
#define TTX_DEVFUN_WAVES (TTX_DEVFUN_BLOCK / 64)
#define TTX_DEVFUN_STRETCH 1024                     /* -DTTX_DEVFUN_COMPACT: flags one workgroup compacts at a time (64 lanes x 16 flags) */
#define TTX_DEVFUN_KIND_LANE 0
#define TTX_DEVFUN_KIND_WAVE 1

struct ttx_devfun_info {
    int abi;            /* TTX_DEVFUN_ABI the file was compiled against */
    int kind;           /* TTX_DEVFUN_KIND_* */
    int block;          /* TTX_DEVFUN_BLOCK */
    int lds_per_wave;   /* bytes of dynamic LDS per wave (wave form; 0 for the lane form) */
};

/* A view of one multi-index where the engine keeps it -- a row of the slot array (16-bit) or of the list of ttx_eval_device
 * (32-bit): nothing is copied, an integrand of 2048 dimensions keeps no index array in scratch memory.
 * ind[k], k = 0 .. d-1 (C style) and ind(k), k = 1 .. d (the reference's ind(k)) both give the 1-based index of a mode. */
struct ttx_ind {
    const short *p16;
    const int *p32;
    __device__ __forceinline__ int operator[](int k) const { return p32 ? p32[k] : (int)p16[k]; }
    __device__ __forceinline__ int operator()(int k) const { return (*this)[k - 1]; }
};

/* wave form: this wave's share of the dynamic LDS (bytes_per_wave as given to TTX_DEVICE_INTEGRAND_WAVE).  A wave orders its own
 * LDS traffic with __builtin_amdgcn_wave_barrier(); never __syncthreads() -- the waves of a workgroup work on different elements. */
__device__ __forceinline__ void *ttx_wave_lds(int bytes_per_wave)
{
    extern __shared__ __align__(16) unsigned char ttx_devfun_dynlds[];
    return ttx_devfun_dynlds + (size_t)(threadIdx.x >> 6) * bytes_per_wave;
}

/* 16 request flags of one lane as a bit mask (bit j: flag first + j is raised); one 16-byte load where all 16 exist */
__device__ __forceinline__ unsigned ttx_devfun_flags16(const unsigned char *hreq, long long first, long long nslot)
{
    unsigned m = 0;
    if (first + 16 <= nslot) {
        const uint4 w = *reinterpret_cast<const uint4 *>(hreq + first);
        if ((w.x | w.y | w.z | w.w) == 0) return 0;
        const unsigned q[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int j = 0; j < 16; j++) m |= ((q[j >> 2] >> (8 * (j & 3))) & 0xffu) ? (1u << j) : 0u;
    } else {
        for (int j = 0; j < 16 && first + j < nslot; j++) m |= hreq[first + j] ? (1u << j) : 0u;
    }
    return m;
}

/* ---- lane form: one lane per element -------------------------------------------------------------------------------------------
 * A launch of the sweep raises one fiber batch of flags: dense runs at the start of each bond group's slots, holes where mode
 * sizes differ or a candidate was dropped, nothing behind them.  The kernel that ships is the plain grid-stride one: one lane per
 * slot; a wave over an empty stretch leaves at once, a wave inside a run is full, and a batch is spread over as many compute
 * units as it has waves.
 * -DTTX_DEVFUN_COMPACT builds the alternative that was measured against it ("Loadable device integrands"): each
 * workgroup first COMPACTS a stretch of TTX_DEVFUN_STRETCH flags -- wave 0 reads them 16 per lane in one 16-byte load, a shuffle
 * prefix sum over the per-lane counts gives each lane its place, the raised slots go to a list in LDS in slot order -- and then all
 * TTX_DEVFUN_BLOCK lanes take consecutive entries, so every wave but the last is full.  With the sweep's dense runs it gathers a
 * batch onto few compute units and pays two barriers per stretch: 6.9 us against 4.8 us per launch at d = 12, n = 65, r = 20.  It
 * pays only for integrands whose raised flags are thinly scattered; the engine launches both the same way. */
#ifdef TTX_DEVFUN_COMPACT
#define TTX_DEVFUN_SLOTS_LANE_BODY(NAME)                                                                                          \
    __shared__ unsigned short ttx_list[TTX_DEVFUN_STRETCH];                                                                       \
    __shared__ int ttx_total;                                                                                                     \
    const int tid = threadIdx.x, lane = tid & 63;                                                                                 \
    const long long nstretch = (nslot + TTX_DEVFUN_STRETCH - 1) / TTX_DEVFUN_STRETCH;                                              \
    for (long long st = blockIdx.x; st < nstretch; st += gridDim.x) {                                                             \
        const long long base = st * TTX_DEVFUN_STRETCH;                                                                           \
        if (tid < 64) {                                                                                                           \
            const unsigned m = ttx_devfun_flags16(hreq, base + 16 * lane, nslot);                                                  \
            int incl = __popc(m);                                                                                                 \
            if (__ballot(m != 0) == 0ull) {                                                                                       \
                if (lane == 0) ttx_total = 0;                                                                                     \
            } else {                                                                                                              \
                const int cnt = incl;                                                                                             \
                _Pragma("unroll") for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; } \
                int at = incl - cnt;                                                                                              \
                for (unsigned mm = m; mm; mm &= mm - 1) ttx_list[at++] = (unsigned short)(16 * lane + __ffs(mm) - 1);              \
                if (lane == 63) ttx_total = incl;                                                                                 \
            }                                                                                                                     \
        }                                                                                                                         \
        __syncthreads();                                                                                                          \
        const int total = ttx_total;                                                                                              \
        for (int e = tid; e < total; e += TTX_DEVFUN_BLOCK) {                                                                     \
            const long long s = base + ttx_list[e];                                                                               \
            const ttx_ind ix = {hidx + (size_t)s * d, nullptr};                                                                   \
            hval[s] = NAME(d, ix, n, par);                                                                                        \
            hreq[s] = 0;                                                                                                          \
        }                                                                                                                         \
        __syncthreads();                                                                                                          \
    }
#else
#define TTX_DEVFUN_SLOTS_LANE_BODY(NAME)                                                                                          \
    for (long long s = (long long)blockIdx.x * TTX_DEVFUN_BLOCK + threadIdx.x; s < nslot; s += (long long)gridDim.x * TTX_DEVFUN_BLOCK) { \
        if (!hreq[s]) continue;                                                                                                   \
        const ttx_ind ix = {hidx + (size_t)s * d, nullptr};                                                                       \
        hval[s] = NAME(d, ix, n, par);                                                                                            \
        hreq[s] = 0;                                                                                                              \
    }
#endif

/* TTX_DEVICE_INTEGRAND(name) for  __device__ double name(int d, ttx_ind ind, const int *n, const double *par) */
#define TTX_DEVICE_INTEGRAND(NAME)                                                                                                \
    extern "C" __device__ __attribute__((used, visibility("default"))) const ttx_devfun_info ttx_devfun_info_##NAME =              \
        {TTX_DEVFUN_ABI, TTX_DEVFUN_KIND_LANE, TTX_DEVFUN_BLOCK, 0};                                                              \
    extern "C" __global__ __launch_bounds__(TTX_DEVFUN_BLOCK) void ttx_devfun_slots_##NAME(                                       \
        int d, const int *n, const double *par, long long nslot, const short *hidx, unsigned char *hreq, double *hval)            \
    {                                                                                                                             \
        TTX_DEVFUN_SLOTS_LANE_BODY(NAME)                                                                                          \
    }                                                                                                                             \
    extern "C" __global__ __launch_bounds__(TTX_DEVFUN_BLOCK) void ttx_devfun_list_##NAME(                                        \
        int d, const int *n, const double *par, long long npts, const int *ind, double *out)                                      \
    {                                                                                                                             \
        for (long long p = (long long)blockIdx.x * TTX_DEVFUN_BLOCK + threadIdx.x; p < npts; p += (long long)gridDim.x * TTX_DEVFUN_BLOCK) { \
            const ttx_ind ix = {nullptr, ind + (size_t)p * d};                                                                    \
            out[p] = NAME(d, ix, n, par);                                                                                         \
        }                                                                                                                         \
    }

/* ---- wave form: one wave64 per element, for integrands with inner parallelism ---------------------------------------------------
 * TTX_DEVICE_INTEGRAND_WAVE(name [, lds_bytes_per_wave]) for
 *     __device__ double name(int d, ttx_ind ind, const int *n, const double *par, int lane)
 * All 64 lanes of a wave call `name` with the same element and lane = 0 .. 63; the value lane 0 returns is the element's value.
 * lds_bytes_per_wave (a constant, default 0) is what ttx_wave_lds() hands out; TTX_DEVFUN_WAVES times it may not exceed 64 KB. */
#define TTX_DEVICE_INTEGRAND_WAVE(NAME, ...)                                                                                      \
    extern "C" __device__ __attribute__((used, visibility("default"))) const ttx_devfun_info ttx_devfun_info_##NAME =              \
        {TTX_DEVFUN_ABI, TTX_DEVFUN_KIND_WAVE, TTX_DEVFUN_BLOCK, (0 + __VA_ARGS__ + 0)};                                           \
    extern "C" __global__ __launch_bounds__(TTX_DEVFUN_BLOCK) void ttx_devfun_slots_##NAME(                                       \
        int d, const int *n, const double *par, long long nslot, const short *hidx, unsigned char *hreq, double *hval)            \
    {                                                                                                                             \
        const int lane = threadIdx.x & 63;                                                                                        \
        const long long nw = (long long)gridDim.x * TTX_DEVFUN_WAVES;                                                             \
        for (long long s = (long long)blockIdx.x * TTX_DEVFUN_WAVES + (threadIdx.x >> 6); s < nslot; s += nw) {                   \
            if (!hreq[s]) continue;                                     /* wave-uniform */                                        \
            const ttx_ind ix = {hidx + (size_t)s * d, nullptr};                                                                   \
            const double v = NAME(d, ix, n, par, lane);                                                                           \
            if (lane == 0) { hval[s] = v; hreq[s] = 0; }                                                                          \
        }                                                                                                                         \
    }                                                                                                                             \
    extern "C" __global__ __launch_bounds__(TTX_DEVFUN_BLOCK) void ttx_devfun_list_##NAME(                                        \
        int d, const int *n, const double *par, long long npts, const int *ind, double *out)                                      \
    {                                                                                                                             \
        const int lane = threadIdx.x & 63;                                                                                        \
        const long long nw = (long long)gridDim.x * TTX_DEVFUN_WAVES;                                                             \
        for (long long p = (long long)blockIdx.x * TTX_DEVFUN_WAVES + (threadIdx.x >> 6); p < npts; p += nw) {                    \
            const ttx_ind ix = {nullptr, ind + (size_t)p * d};                                                                    \
            const double v = NAME(d, ix, n, par, lane);                                                                           \
            if (lane == 0) out[p] = v;                                                                                            \
        }                                                                                                                         \
    }

/* ---- combiner of an integrand of trains (TTX_FUN_TRAINS, TTX_TOP_DEVICE) ----------------------------------------------------------
 * TTX_DEVICE_COMBINER(name) for
 *     __device__ double name(int m, const double *v, int d, ttx_ind ind, const int *n, const double *par)
 * v[0 .. m-1] are the values of the m operand trains at the multi-index ind, computed by the engine (each bit for bit what
 * ttx_ijk_batch gives in its exact mode); the function returns g(v, ind).  Lane form.  The macro generates
 *   ttx_devcomb_info_NAME   a ttx_devfun_info as above
 *   ttx_devcomb_slots_NAME  (int m, int d, const int *n, const double *par, long long nslot, const short *hidx, unsigned char *hreq,
 *                            const double *tval, double *hval): tval[nslot][m] holds the operand values of every raised slot.  The
 *                           contract of ttx_devfun_slots_NAME: write hval[s], THEN clear hreq[s]; touch no other slot; any grid.
 *   ttx_devcomb_list_NAME   (int m, int d, const int *n, const double *par, long long npts, const int *ind, const double *tval,
 *                            double *out): the 32-bit list twin, tval[npts][m]
 * and the file is handed to ttx_set_integrand_trains_device[_file] (include/ttx.h).  For a pivot sequence equal to a host run keep
 * to + - * / and sqrt, in the host code's order (BIT REPRODUCIBILITY above).
 *
 * The same macro serves a pulled-back integrand (TTX_FUN_PULLBACK, ttx_set_integrand_pullback[_file] of include/ttx.h): there the
 * engine calls the function with m = d + 2 and v = [x_1 .. x_d, logq, val] -- the point of the multi-index ind pulled back through the
 * layers, the log density of the transport's push-forward of the uniform at x, and the value of the outermost layer's train at x.  A
 * sample that failed arrives as x = NaN, logq = NaN, val = 0.0; what the function returns for it is the integrand's value.  A target
 * density enters as h = sqrt(exp(logpi(x) - logq)) (examples/devfun/pullback_tempered.hip); exp and log are not IEEE operations, so
 * such a combiner agrees with a host evaluation to a few units in the last place, not bit for bit. */
#define TTX_DEVICE_COMBINER(NAME)                                                                                                \
    extern "C" __device__ __attribute__((used, visibility("default"))) const ttx_devfun_info ttx_devcomb_info_##NAME =             \
        {TTX_DEVFUN_ABI, TTX_DEVFUN_KIND_LANE, TTX_DEVFUN_BLOCK, 0};                                                              \
    extern "C" __global__ __launch_bounds__(TTX_DEVFUN_BLOCK) void ttx_devcomb_slots_##NAME(                                      \
        int m, int d, const int *n, const double *par, long long nslot, const short *hidx, unsigned char *hreq, const double *tval, \
        double *hval)                                                                                                             \
    {                                                                                                                             \
        for (long long s = (long long)blockIdx.x * TTX_DEVFUN_BLOCK + threadIdx.x; s < nslot; s += (long long)gridDim.x * TTX_DEVFUN_BLOCK) { \
            if (!hreq[s]) continue;                                                                                               \
            const ttx_ind ix = {hidx + (size_t)s * d, nullptr};                                                                   \
            hval[s] = NAME(m, tval + (size_t)s * m, d, ix, n, par);                                                               \
            hreq[s] = 0;                                                                                                          \
        }                                                                                                                         \
    }                                                                                                                             \
    extern "C" __global__ __launch_bounds__(TTX_DEVFUN_BLOCK) void ttx_devcomb_list_##NAME(                                       \
        int m, int d, const int *n, const double *par, long long npts, const int *ind, const double *tval, double *out)           \
    {                                                                                                                             \
        for (long long p = (long long)blockIdx.x * TTX_DEVFUN_BLOCK + threadIdx.x; p < npts; p += (long long)gridDim.x * TTX_DEVFUN_BLOCK) { \
            const ttx_ind ix = {nullptr, ind + (size_t)p * d};                                                                    \
            out[p] = NAME(m, tval + (size_t)p * m, d, ix, n, par);                                                                \
        }                                                                                                                         \
    }

#endif
