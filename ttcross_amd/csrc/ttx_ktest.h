// ttx_ktest.h -- the kernels that exist only for a test or probe entry point (ttx_k_*), and those entry points.  Included last by
// ttx_engine.hip; nothing of the library proper depends on it.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>
#include "../../include/ttx.h"
#include "ttx_err.h"
#include "ttx_create_plan.h"   // powi
#include "ttx_kernels.h"
#include "ttx_de.h"            // lds_chain, lds_sum_chain, de_run
#include "ttx_mvn.h"
#include "ttx_cluster.h"       // xcc_id
#include "ttx_coscoeff.h"      // k_coscoeff_list, coscoeff_check

// ------------------------------------------------------------------------------------------------
// stand-alone kernels behind the ttx_k_* test entry points (same device functions as the sweep)
// ------------------------------------------------------------------------------------------------
template <int FUN>
__global__ void k_eval_list(DevProb P, long long npts, const int *ind, double *out)
{
    extern __shared__ __align__(16) double dyn[];
    for (int x = threadIdx.x; x < P.npar; x += blockDim.x) dyn[x] = P.par[x];
    __syncthreads();
    long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= npts) return;
    ListIdx ix{ind + t * P.d};
    out[t] = eval_fun<FUN>(P, dyn, ix);
}

// b = a - F x (dgemv 'n' order) + per-block first arg-max; F is m x r with leading dimension ld
__global__ __launch_bounds__(TTX_BLK) void k_resid_argmax(int m, int r, size_t ld, const double *a, const double *F, const double *x,
                                                          double *b_out, Partial *parts)
{
    __shared__ double xs[256];
    __shared__ double sha[4], shv[4]; __shared__ int shi[4];
    for (int s = threadIdx.x; s < r; s += TTX_BLK) xs[s] = x[s];
    __syncthreads();
    int t = blockIdx.x * TTX_BLK + threadIdx.x;
    double b = 0.0, ab = -1.0; int bi = INT_MAX;
    if (t < m) {
        b = a[t];
#pragma unroll 8
        for (int s = 0; s < r; s++) b = b + (-xs[s]) * F[t + ld * s];
        b_out[t] = b; ab = fabs(b); bi = t;
    }
    block_argmax(ab, b, bi, sha, shv, shi);
    if (threadIdx.x == 0) { Partial pr; pr.absmax = ab; pr.val = b; pr.idx = bi; pr.pad = 0; parts[blockIdx.x] = pr; }
}

__global__ void k_lottery_only(int npnt, int m, int n, int nz, const int *zcol, const int *zrow, unsigned long long rngpos, int *points)
{
    __shared__ ttx_cdfseg segc[TTX_MAXSEG], segr[TTX_MAXSEG];
    __shared__ int nsc, nsr;
    if (threadIdx.x == 0) nsc = ttx_cdf_build(m - nz, segc);
    if (threadIdx.x == 64) nsr = ttx_cdf_build(n - nz, segr);
    __syncthreads();
    for (int il = threadIdx.x; il < npnt; il += blockDim.x) {
        double d1 = ttx_flang_draw(rngpos + il), d2 = ttx_flang_draw(rngpos + npnt + il);
        points[il] = ttx_lottery_index(segc, nsc, m - nz, m, zcol, nz, d1);
        points[npnt + il] = ttx_lottery_index(segr, nsr, n - nz, n, zrow, nz, d2);
    }
}

__global__ void k_fill_synth(double *p, size_t n, unsigned long long seed)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned long long x = (i + 1) * 0x9E3779B97F4A7C15ull + seed; x ^= x >> 29; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 32;
        p[i] = (double)(x >> 11) * (1.0 / 9007199254740992.0) - 0.5;
    }
}
// grid-stride variant of k_resid_argmax for factors far larger than one wave of blocks (same arithmetic per row)
__global__ __launch_bounds__(TTX_BLK) void k_resid_argmax_stream(long long m, int r, size_t ld, const double *a, const double *F, const double *x,
                                                                 double *b_out, Partial *parts)
{
    __shared__ double xs[256];
    __shared__ double sha[4], shv[4]; __shared__ int shi[4];
    for (int s = threadIdx.x; s < r; s += TTX_BLK) xs[s] = x[s];
    __syncthreads();
    double ab = -1.0, bv = 0.0; int bi = INT_MAX;
    for (long long t = (long long)blockIdx.x * TTX_BLK + threadIdx.x; t < m; t += (long long)gridDim.x * TTX_BLK) {
        double b = a[t];
#pragma unroll 8
        for (int s = 0; s < r; s++) b = b + (-xs[s]) * F[t + ld * s];
        b_out[t] = b;
        double aa = fabs(b);
        if (aa > ab || (aa == ab && (int)t < bi)) { ab = aa; bv = b; bi = (int)t; }
    }
    block_argmax(ab, bv, bi, sha, shv, shi);
    if (threadIdx.x == 0) { Partial pr; pr.absmax = ab; pr.val = bv; pr.idx = bi; pr.pad = 0; parts[blockIdx.x] = pr; }
}
__global__ void k_xcc_probe(int *out) { if (threadIdx.x == 0) out[blockIdx.x] = xcc_id(); }

// ---- kernel-level test entry points ------------------------------------------------------------------
extern "C" int ttx_k_residual_argmax(int32_t device, int32_t m, int32_t r, const double *a, const double *F, const double *x,
                                     double *b_out, int32_t *imax, double *bmax)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TTX_ENODEV, "no HIP device");
    HIPCHECK(hipSetDevice(device));
    if (r > 256 || m < 1) return fail(TTX_EINVAL, "ttx_k_residual_argmax: bad sizes");
    double *da, *dF, *dx, *db; Partial *dp;
    int nb = (m + TTX_BLK - 1) / TTX_BLK;
    HIPCHECK(hipMalloc((void **)&da, sizeof(double) * m)); HIPCHECK(hipMalloc((void **)&dF, sizeof(double) * (size_t)m * std::max(r, 1)));
    HIPCHECK(hipMalloc((void **)&dx, sizeof(double) * std::max(r, 1))); HIPCHECK(hipMalloc((void **)&db, sizeof(double) * m));
    HIPCHECK(hipMalloc((void **)&dp, sizeof(Partial) * nb));
    HIPCHECK(hipMemcpy(da, a, sizeof(double) * m, hipMemcpyHostToDevice));
    if (r > 0) { HIPCHECK(hipMemcpy(dF, F, sizeof(double) * (size_t)m * r, hipMemcpyHostToDevice)); HIPCHECK(hipMemcpy(dx, x, sizeof(double) * r, hipMemcpyHostToDevice)); }
    hipLaunchKernelGGL(k_resid_argmax, dim3(nb), dim3(TTX_BLK), 0, 0, m, r, (size_t)m, da, dF, dx, db, dp);
    HIPCHECK(hipDeviceSynchronize());
    std::vector<Partial> parts(nb);
    HIPCHECK(hipMemcpy(parts.data(), dp, sizeof(Partial) * nb, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy(b_out, db, sizeof(double) * m, hipMemcpyDeviceToHost));
    double ba = -1; int bi = INT_MAX; double bv = 0;
    for (auto &p : parts) if (p.absmax > ba || (p.absmax == ba && p.idx < bi)) { ba = p.absmax; bi = p.idx; bv = p.val; }
    *imax = bi; *bmax = bv;
    (void)hipFree(da); (void)hipFree(dF); (void)hipFree(dx); (void)hipFree(db); (void)hipFree(dp);
    return TTX_OK;
}

extern "C" int ttx_k_residual_bench(int32_t device, int64_t m, int32_t r, int32_t iters, double *avg_ms, double *bytes)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TTX_ENODEV, "no HIP device");
    HIPCHECK(hipSetDevice(device));
    if (m < 1 || m > 2000000000LL || r < 1 || r > 256 || iters < 1) return fail(TTX_EINVAL, "ttx_k_residual_bench: bad sizes");
    double *da, *dF, *dx, *db; Partial *dp;
    const int nb = 256 * 8;                                 // 8 blocks per CU, grid-stride
    HIPCHECK(hipMalloc((void **)&da, sizeof(double) * m)); HIPCHECK(hipMalloc((void **)&dF, sizeof(double) * (size_t)m * r));
    HIPCHECK(hipMalloc((void **)&dx, sizeof(double) * r)); HIPCHECK(hipMalloc((void **)&db, sizeof(double) * m));
    HIPCHECK(hipMalloc((void **)&dp, sizeof(Partial) * nb));
    hipLaunchKernelGGL(k_fill_synth, dim3(2048), dim3(256), 0, 0, da, (size_t)m, 1ull);
    hipLaunchKernelGGL(k_fill_synth, dim3(2048), dim3(256), 0, 0, dF, (size_t)m * r, 2ull);
    hipLaunchKernelGGL(k_fill_synth, dim3(1), dim3(256), 0, 0, dx, (size_t)r, 3ull);
    hipEvent_t e0, e1;
    HIPCHECK(hipEventCreate(&e0)); HIPCHECK(hipEventCreate(&e1));
    for (int w = 0; w < 2; w++) hipLaunchKernelGGL(k_resid_argmax_stream, dim3(nb), dim3(TTX_BLK), 0, 0, (long long)m, r, (size_t)m, da, dF, dx, db, dp);
    HIPCHECK(hipEventRecord(e0, 0));
    for (int w = 0; w < iters; w++) hipLaunchKernelGGL(k_resid_argmax_stream, dim3(nb), dim3(TTX_BLK), 0, 0, (long long)m, r, (size_t)m, da, dF, dx, db, dp);
    HIPCHECK(hipEventRecord(e1, 0));
    HIPCHECK(hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHECK(hipEventElapsedTime(&ms, e0, e1));
    *avg_ms = ms / iters;
    *bytes = 8.0 * ((double)m * r + r + 2.0 * m);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(da); (void)hipFree(dF); (void)hipFree(dx); (void)hipFree(db); (void)hipFree(dp);
    return TTX_OK;
}

// ---- latency probe: the unit costs of the dependent chains that bound the sweep kernels at BASELINE sizes ----------
// one wave, one chain each, timed with the 100 MHz wall clock (s_memrealtime): out[0] ns per dependent fp64 multiply,
// out[1] ns per dependent fp64 add after multiply pair (the running sums of the Ising C integrand), out[2] ns per
// dependent L2 round trip (pointer chase with L1-bypassing loads, 64 KB ring = L2-resident), out[3] ns per dependent
// LDS read, out[4] ns per fp64 IEEE division in a dependent chain
__global__ __launch_bounds__(64) void k_latency_probe(const unsigned *ring, double *out, double seed)
{
    __shared__ unsigned lds_ring[1024];
    const int lane = threadIdx.x;
    const int N = 4096;
    for (int x = lane; x < 1024; x += 64) lds_ring[x] = (unsigned)((x * 37 + 11) & 1023);
    __syncthreads();
    double x = seed, y = 1.0 + 1e-9 * lane;
    long long t0 = wall_clock64();
#pragma unroll 16
    for (int k = 0; k < N; k++) x = x * y;
    long long t1 = wall_clock64();
    double s = seed, pk = 1.0;
#pragma unroll 16
    for (int k = 0; k < N; k++) { pk = pk * y; s = s + pk; }
    long long t2 = wall_clock64();
    unsigned p = (unsigned)lane;
    for (int k = 0; k < 1024; k++) { unsigned v; asm volatile("global_load_dword %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(ring + p) : "memory"); p = v; }
    long long t3 = wall_clock64();
    unsigned q = (unsigned)lane;
#pragma unroll 8
    for (int k = 0; k < N; k++) q = lds_ring[q];
    long long t4 = wall_clock64();
    double z = seed + 3.0;
#pragma unroll 4
    for (int k = 0; k < 1024; k++) z = (z - 1.0) / (z + 1.0) + 3.0;
    long long t5 = wall_clock64();
    if (lane == 0) {
        out[0] = 10.0 * (double)(t1 - t0) / N; out[1] = 10.0 * (double)(t2 - t1) / N; out[2] = 10.0 * (double)(t3 - t2) / 1024;
        out[3] = 10.0 * (double)(t4 - t3) / N; out[4] = 10.0 * (double)(t5 - t4) / 1024;
        out[5] = x + s + (double)p + (double)q + z;      // keep the chains alive
    }
}
// development probe: ns per element of the LDS-broadcast folds (one wave per block, `nblk` blocks), rows of `len` doubles
__global__ __launch_bounds__(64) void k_fold_probe(int len, int reps, double *out)
{
    __shared__ double row[1024];
    const int lane = threadIdx.x;
    for (int x = lane; x < 1024; x += 64) row[x] = 1.0 + 1e-9 * x;
    __syncthreads();
    double a = 1.0, s = 0.0;
    long long t0 = wall_clock64();
    for (int r = 0; r < reps; r++) a = lds_chain(a, row + (r & 7), len);
    long long t1 = wall_clock64();
    for (int r = 0; r < reps; r++) s = lds_sum_chain(s, row + (r & 7), len);
    long long t2 = wall_clock64();
    double u = 0.7 + 1e-9 * lane, b = 1.0;
    for (int r = 0; r < reps; r++) de_run<true>(b, u, 0.999, row, len);
    long long t3 = wall_clock64();
    // issue throughput of independent instructions on one wave: 8 streams each
    double f[8], g8[8]; float h8[8];
#pragma unroll
    for (int q = 0; q < 8; q++) { f[q] = 1.0 + 1e-9 * (lane + q); g8[q] = 1.5 + 1e-3 * (lane + q); h8[q] = 1.5f + 1e-3f * (lane + q); }
    long long t4 = wall_clock64();
    for (int r = 0; r < 512; r++) {
#pragma unroll
        for (int q = 0; q < 8; q++) f[q] = __builtin_fma(f[q], 1.0000001, 1e-9);
    }
    long long t5 = wall_clock64();
    for (int r = 0; r < 512; r++) {
#pragma unroll
        for (int q = 0; q < 8; q++) g8[q] = __builtin_amdgcn_rcp(g8[q]);
    }
    long long t6 = wall_clock64();
    for (int r = 0; r < 512; r++) {
#pragma unroll
        for (int q = 0; q < 8; q++) h8[q] = __builtin_amdgcn_rcpf(h8[q]);
    }
    long long t7 = wall_clock64();
    double n8[8], d8[8];
#pragma unroll
    for (int q = 0; q < 8; q++) { n8[q] = -0.3 - 1e-3 * q; d8[q] = 1.7 + 1e-3 * (lane + q); }
    for (int r = 0; r < 512; r++) {
#pragma unroll
        for (int q = 0; q < 8; q++) n8[q] = fdiv_unit(n8[q], d8[q]);
    }
    long long t8 = wall_clock64();
    if (lane == 0 && blockIdx.x == 0) {
        out[0] = 10.0 * (double)(t1 - t0) / ((double)reps * len); out[1] = 10.0 * (double)(t2 - t1) / ((double)reps * len);
        out[2] = 10.0 * (double)(t3 - t2) / ((double)reps * (len + 1));
        out[3] = 10.0 * (double)(t5 - t4) / 4096.0; out[4] = 10.0 * (double)(t6 - t5) / 4096.0; out[5] = 10.0 * (double)(t7 - t6) / 4096.0;
        out[6] = 10.0 * (double)(t8 - t7) / 4096.0;
        double acc = a + s + b;
#pragma unroll
        for (int q = 0; q < 8; q++) acc += f[q] + g8[q] + (double)h8[q] + n8[q];
        out[7] = acc;
    }
}
extern "C" int ttx_k_fold_probe(int32_t device, int32_t nblk, int32_t len, double out[7])
{
    HIPCHECK(hipSetDevice(device));
    double *d; HIPCHECK(hipMalloc((void **)&d, 128));
    double o[8];
    hipLaunchKernelGGL(k_fold_probe, dim3(nblk), dim3(64), 0, 0, len, 200, d);
    hipLaunchKernelGGL(k_fold_probe, dim3(nblk), dim3(64), 0, 0, len, 200, d);
    HIPCHECK(hipMemcpy(o, d, 64, hipMemcpyDeviceToHost));
    for (int k = 0; k < 7; k++) out[k] = o[k];
    (void)hipFree(d);
    return TTX_OK;
}

extern "C" int ttx_k_latency_probe(int32_t device, double out[5])
{
    if (!out) return fail(TTX_EINVAL, "ttx_k_latency_probe: null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TTX_ENODEV, "no HIP device");
    HIPCHECK(hipSetDevice(device));
    const int R = 16384;                                       // 64 KB ring of indices, a single cycle with stride 4099
    std::vector<unsigned> ring(R);
    for (int i = 0; i < R; i++) ring[i] = (unsigned)((i + 4099) % R);
    unsigned *dr; double *dout;
    HIPCHECK(hipMalloc((void **)&dr, sizeof(unsigned) * R)); HIPCHECK(hipMalloc((void **)&dout, sizeof(double) * 8));
    HIPCHECK(hipMemcpy(dr, ring.data(), sizeof(unsigned) * R, hipMemcpyHostToDevice));
    double best[5] = {1e30, 1e30, 1e30, 1e30, 1e30}, o[8];
    for (int rep = 0; rep < 5; rep++) {
        hipLaunchKernelGGL(k_latency_probe, dim3(1), dim3(64), 0, 0, (const unsigned *)dr, dout, 1.0 + 1e-12 * rep);
        HIPCHECK(hipMemcpy(o, dout, sizeof(double) * 6, hipMemcpyDeviceToHost));
        for (int k = 0; k < 5; k++) best[k] = std::min(best[k], o[k]);
    }
    for (int k = 0; k < 5; k++) out[k] = best[k];
    (void)hipFree(dr); (void)hipFree(dout);
    return TTX_OK;
}

static int k_eval_impl(int32_t device, int32_t fun_id, int32_t d, const int32_t *n, const double *par, int32_t npar,
                       const double *aux, int32_t naux, int64_t npts, const int32_t *ind, double *out, int arith);
extern "C" int ttx_k_eval(int32_t device, int32_t fun_id, int32_t d, const int32_t *n, const double *par, int32_t npar,
                          const double *aux, int32_t naux, int64_t npts, const int32_t *ind, double *out)
{ return k_eval_impl(device, fun_id, d, n, par, npar, aux, naux, npts, ind, out, 0); }
extern "C" int ttx_k_eval_arith(int32_t device, int32_t fun_id, int32_t d, const int32_t *n, const double *par, int32_t npar,
                                const double *aux, int32_t naux, int64_t npts, const int32_t *ind, double *out, int32_t arith)
{ return k_eval_impl(device, fun_id, d, n, par, npar, aux, naux, npts, ind, out, arith); }
static int k_eval_impl(int32_t device, int32_t fun_id, int32_t d, const int32_t *n, const double *par, int32_t npar,
                       const double *aux, int32_t naux, int64_t npts, const int32_t *ind, double *out, int arith)
{
    if (fun_id != TTX_FUN_ISING && fun_id != TTX_FUN_STDNORM && fun_id != TTX_FUN_MVN && fun_id != TTX_FUN_COSCOEFF)
        return fail(TTX_EINVAL, "ttx_k_eval: unknown fun_id %d", fun_id);
    if (d < 1 || !n || npts < 0 || (npts > 0 && !ind) || (npts > 0 && !out)) return fail(TTX_EINVAL, "ttx_k_eval: bad arguments");
    if (fun_id == TTX_FUN_COSCOEFF) {
        if (int rc0 = coscoeff_check("ttx_k_eval", d, n, aux, naux)) return rc0;
        for (int64_t p = 0; p < npts * d; p++)
            if (ind[p] < 1 || ind[p] > n[p % d]) return fail(TTX_EINVAL, "ttx_k_eval: index %d outside 1..n", ind[p]);
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TTX_ENODEV, "no HIP device");
        HIPCHECK(hipSetDevice(device));
        if (npts == 0) return TTX_OK;
        int *dind; double *daux, *dout;
        HIPCHECK(hipMalloc((void **)&dind, sizeof(int) * npts * d)); HIPCHECK(hipMalloc((void **)&dout, sizeof(double) * npts));
        HIPCHECK(hipMalloc((void **)&daux, sizeof(double) * naux));
        HIPCHECK(hipMemcpy(dind, ind, sizeof(int) * npts * d, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(daux, aux, sizeof(double) * naux, hipMemcpyHostToDevice));
        const unsigned grid = (unsigned)std::min<int64_t>((npts + TTX_CC_WAVES - 1) / TTX_CC_WAVES, 1024);
        hipLaunchKernelGGL(k_coscoeff_list, dim3(grid), dim3(64 * TTX_CC_WAVES), sizeof(double) * TTX_CC_WAVES * TTX_CC_LDS(d), 0,
                           d, (const double *)daux, (long long)npts, (const int *)dind, dout);
        HIPCHECK(hipDeviceSynchronize());
        HIPCHECK(hipMemcpy(out, dout, sizeof(double) * npts, hipMemcpyDeviceToHost));
        (void)hipFree(dind); (void)hipFree(dout); (void)hipFree(daux);
        return TTX_OK;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TTX_ENODEV, "no HIP device");
    HIPCHECK(hipSetDevice(device));
    DevProb P{};
    std::vector<int> n1(d + 2, 1);
    for (int k = 1; k <= d; k++) n1[k] = n[k - 1];
    int *dn, *dind; double *dpar, *daux = nullptr, *dout;
    HIPCHECK(hipMalloc((void **)&dn, sizeof(int) * (d + 2))); HIPCHECK(hipMalloc((void **)&dpar, sizeof(double) * npar));
    HIPCHECK(hipMalloc((void **)&dind, sizeof(int) * npts * d)); HIPCHECK(hipMalloc((void **)&dout, sizeof(double) * npts));
    HIPCHECK(hipMemcpy(dn, n1.data(), sizeof(int) * (d + 2), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(dpar, par, sizeof(double) * npar, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(dind, ind, sizeof(int) * npts * d, hipMemcpyHostToDevice));
    if (aux && naux > 0) { HIPCHECK(hipMalloc((void **)&daux, sizeof(double) * naux)); HIPCHECK(hipMemcpy(daux, aux, sizeof(double) * naux, hipMemcpyHostToDevice)); }
    P.d = d; P.n = dn; P.par = dpar; P.aux = daux; P.npar = npar; P.fun_id = fun_id;
    P.ising_id = (fun_id == TTX_FUN_ISING) ? (int)par[2 * n[0]] : 0;
    P.arith = (arith == TTX_ARITH_FAST && fun_id == TTX_FUN_ISING && P.ising_id != 1) ? 1 : 0;     // the one-thread evaluator f_ising_fast (nodes must lie in [0,1])
    P.mvn_norm = (fun_id == TTX_FUN_MVN) ? std::sqrt(powi(2.0 * 3.141592653589793, d) * aux[d + (size_t)d * d]) : 1.0;
    dim3 grid((unsigned)((npts + 255) / 256));
    size_t lds = sizeof(double) * (npar + 2);
    if (fun_id == TTX_FUN_ISING) hipLaunchKernelGGL(k_eval_list<FUN_ISING>, grid, dim3(256), lds, 0, P, (long long)npts, dind, dout);
    else if (fun_id == TTX_FUN_STDNORM) hipLaunchKernelGGL(k_eval_list<FUN_STDNORM>, grid, dim3(256), lds, 0, P, (long long)npts, dind, dout);
    else hipLaunchKernelGGL(k_eval_list<FUN_MVN>, grid, dim3(256), lds, 0, P, (long long)npts, dind, dout);
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(out, dout, sizeof(double) * npts, hipMemcpyDeviceToHost));
    (void)hipFree(dn); (void)hipFree(dpar); (void)hipFree(dind); (void)hipFree(dout); if (daux) (void)hipFree(daux);
    return TTX_OK;
}

__global__ void k_exp_list(long long n, const double *x, double *out)
{
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = ttx_exp(x[t]);
}
extern "C" int ttx_k_exp(int32_t device, int64_t n, const double *x, double *out)
{
    if (!x || !out || n < 1) return fail(TTX_EINVAL, "ttx_k_exp: bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TTX_ENODEV, "no HIP device");
    HIPCHECK(hipSetDevice(device));
    double *dx, *dy;
    HIPCHECK(hipMalloc((void **)&dx, sizeof(double) * n)); HIPCHECK(hipMalloc((void **)&dy, sizeof(double) * n));
    HIPCHECK(hipMemcpy(dx, x, sizeof(double) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_exp_list, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (long long)n, dx, dy);
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(out, dy, sizeof(double) * n, hipMemcpyDeviceToHost));
    (void)hipFree(dx); (void)hipFree(dy);
    return TTX_OK;
}

extern "C" int ttx_k_xcc_map(int32_t device, int32_t nblocks, int32_t *out)
{
    if (!out || nblocks < 1) return fail(TTX_EINVAL, "ttx_k_xcc_map: bad argument");
    HIPCHECK(hipSetDevice(device));
    int *d = nullptr;
    HIPCHECK(hipMalloc((void **)&d, sizeof(int) * nblocks));
    hipLaunchKernelGGL(k_xcc_probe, dim3(nblocks), dim3(256), 0, 0, d);
    HIPCHECK(hipMemcpy(out, d, sizeof(int) * nblocks, hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return TTX_OK;
}
extern "C" int ttx_k_lottery(int32_t device, int32_t npnt, int32_t m, int32_t n, int32_t nz, const int32_t *zcol,
                             const int32_t *zrow, uint64_t rngpos, int32_t *points)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TTX_ENODEV, "no HIP device");
    HIPCHECK(hipSetDevice(device));
    int *dzc, *dzr, *dp;
    HIPCHECK(hipMalloc((void **)&dzc, sizeof(int) * (nz + 1))); HIPCHECK(hipMalloc((void **)&dzr, sizeof(int) * (nz + 1)));
    HIPCHECK(hipMalloc((void **)&dp, sizeof(int) * 2 * npnt));
    if (nz > 0) { HIPCHECK(hipMemcpy(dzc, zcol, sizeof(int) * nz, hipMemcpyHostToDevice)); HIPCHECK(hipMemcpy(dzr, zrow, sizeof(int) * nz, hipMemcpyHostToDevice)); }
    hipLaunchKernelGGL(k_lottery_only, dim3(1), dim3(256), 0, 0, npnt, m, n, nz, dzc, dzr, (unsigned long long)rngpos, dp);
    HIPCHECK(hipDeviceSynchronize());
    HIPCHECK(hipMemcpy(points, dp, sizeof(int) * 2 * npnt, hipMemcpyDeviceToHost));
    (void)hipFree(dzc); (void)hipFree(dzr); (void)hipFree(dp);
    return TTX_OK;
}

// ------------------------------------------------------------------------------------------------
// ttx_k_fast_block: the table evaluators of TTX_ARITH=fast (ttx_fast.h) on one hand-made bond, element by element.  A minimal
// DevProb (one group, one table slot per side: fpersist = 0) stands in for an engine; every value comes from the device functions
// the sweep kernels call -- the kernels below only stage their inputs and store their results.
// ------------------------------------------------------------------------------------------------
struct FbArgs {
    const int *Lidx, *Ridx;            // [rL][p-1], [rR][d-p-1] mode indices (1-based) of the pivots
    int rL, rR, p, chain;
    double *tNear[2], *tDv[2], *tPiv[2];   // second set of tables: a child entry is never written over its parent's
};
// one wave per pivot (grid 2*RM).  chain = 0: the entry from scratch; 1: the dimension farthest from the bond from scratch, then
// one child step per dimension towards the bond, parent and child alternating between the two sets of tables so that the last
// step lands in the tables proper
template <int FUN>
__global__ __launch_bounds__(64) void k_fb_tables(DevProb P, FbArgs A)
{
    extern __shared__ __align__(16) double dyn[];
    const int lane = threadIdx.x, m = P.d, RM = P.RM, p = A.p;
    const int side = (int)blockIdx.x / RM, c = (int)blockIdx.x % RM;
    if (c >= (side == 0 ? A.rL : A.rR)) return;
    const int len = side == 0 ? p - 1 : m - p - 1, d0 = side == 0 ? 0 : p + 1;      // d0: 0-based dimension of entry 0
    const int *ix = (side == 0 ? A.Lidx : A.Ridx) + (size_t)c * len;
    double *xs = dyn, *ws = dyn + m + 8;
    double *nr[2] = {P.fNear[side] + c, A.tNear[side] + c}, *pv[2] = {P.fPiv[side] + c, A.tPiv[side] + c};
    double *dv[2] = {FUN == FUN_MVN ? P.fDv[side] + c : nullptr, FUN == FUN_MVN ? A.tDv[side] + c : nullptr};
    for (int k = lane; k < len; k += 64) {
        if (FUN == FUN_MVN) xs[k] = P.par[ix[k] - 1] - P.aux[d0 + k];
        else { xs[k] = P.par[ix[k] - 1]; ws[k] = P.par[P.n[1] + ix[k] - 1]; }
    }
    __syncthreads();
    if (!A.chain || len == 0) {
        if (FUN == FUN_MVN) mvn_entry_scratch(P, xs, len, d0, dv[0], nr[0], pv[0], lane);
        else fast_entry_scratch(xs, ws, len, side, nr[0], pv[0], RM, lane);
        return;
    }
    int e = side == 0 ? 0 : len - 1, b = (len - 1) & 1;
    if (FUN == FUN_MVN) mvn_entry_scratch(P, xs + e, 1, d0 + e, dv[b], nr[b], pv[b], lane);
    else fast_entry_scratch(xs + e, ws + e, 1, side, nr[b], pv[b], RM, lane);
    for (int k = 1; k < len; k++) {
        __syncthreads();                                   // the parent's entry is complete and visible to the wave
        e = side == 0 ? k : len - 1 - k;
        const int nb = b ^ 1;
        if (FUN == FUN_MVN) mvn_entry_child(P, side, dv[b], nr[b], pv[b], k, d0 + e, xs[e], dv[nb], nr[nb], pv[nb], lane);
        else fast_entry_child(nr[b], pv[b], xs[e], ws[e], nr[nb], pv[nb], RM, lane);
        b = nb;
    }
}
// lottery route: every element (i, j, k, q) of the block as one candidate; cap rows of the two decay tables in LDS
template <int FUN>
__global__ __launch_bounds__(TTX_BLK) void k_fb_lottery(DevProb P, FbArgs A, int cap, double *out)
{
    extern __shared__ __align__(16) double dyn[];
    const int tid = threadIdx.x, RM = P.RM, n = P.n[1], p = A.p;
    double *sNL = dyn, *sNR = dyn + (size_t)cap * RM;
    if (FUN == FUN_ISING) {
        const double *nL = P.fNear[0], *nR = P.fNear[1];
        for (int x = tid; x < cap * RM; x += TTX_BLK) { const int c = x % RM; sNL[x] = (c < A.rL) ? nL[x] : 0.0; sNR[x] = (c < A.rR) ? nR[x] : 0.0; }
    }
    __syncthreads();
    const int total = A.rL * n * n * A.rR;
    for (int t = blockIdx.x * TTX_BLK + tid; t < total; t += gridDim.x * TTX_BLK) {
        const int q = t % A.rR, k = (t / A.rR) % n, j = (t / (A.rR * n)) % n, i = t / (A.rR * n * n);
        out[t] = (FUN == FUN_MVN) ? mvn_fast_value(P, 0, p, 1, i, j, k, q, mvn_fast_cross(P, 0, p, 1, i, q))
                                  : de_fast_elem4(P, 0, p, 1, i, j, k, q, sNL, sNR, cap);
    }
}
// fiber routes: one block per fiber.  Column fibers: block = (k, q) fixed, elements (i, j); row fibers: block = (i, j) fixed,
// elements (k, q).  nfar: entries of the fixed side's far vector above the cut, per fiber (Ising)
template <int FUN>
__global__ __launch_bounds__(TTX_BLK) void k_fb_fiber(DevProb P, FbArgs A, int col, double *out, double *nfar)
{
    extern __shared__ __align__(16) double dyn[];
    __shared__ int s_nfar; __shared__ double s_rfix;
    const int tid = threadIdx.x, n = P.n[1], p = A.p, rL = A.rL, rR = A.rR, b = blockIdx.x;
    const bool iscol = col != 0;
    double *par = dyn, *far = dyn + ((P.npar + 1) & ~1), *Xv = far + ((max(P.FD, TTX_FNR) + 3) & ~1);
    for (int x = tid; x < P.npar; x += TTX_BLK) par[x] = P.par[x];
    const int vfix = iscol ? b / n : b % rL, xfix = iscol ? b % n : b / rL;
    if (tid == 0) s_nfar = 0;
    __syncthreads();
    if (FUN == FUN_ISING) de_fast_fiber_stage(P, iscol ? 0 : 1, 0, p, 1, vfix, xfix, far, s_nfar, s_rfix, tid);
    if (FUN == FUN_MVN) mvn_fast_fiber_stage(P, iscol, 0, p, 1, iscol ? rL : rR, vfix, Xv, tid);
    __syncthreads();
    if (tid == 0) nfar[b] = (double)s_nfar;
    const int nf = iscol ? rL * n : n * rR;
    for (int t = tid; t < nf; t += TTX_BLK) {
        const int u = iscol ? t % rL : t % n, v = iscol ? t / rL : t / n;
        const double a = (FUN == FUN_ISING) ? de_fast_fiber_elem(P, iscol, 0, p, 1, iscol ? u : v, iscol ? v : u, vfix, xfix, par, far, s_nfar, s_rfix)
                                            : mvn_fast_fiber_elem(P, iscol, 0, p, 1, u, v, vfix, xfix, Xv);
        const int i = iscol ? u : vfix, j = iscol ? v : xfix, k = iscol ? xfix : u, q = iscol ? vfix : v;
        out[(((size_t)i * n + j) * n + k) * rR + q] = a;
    }
}
// point route: one wave per full multi-index (1-based), as the boundary corners stage it
template <int FUN>
__global__ __launch_bounds__(64) void k_fb_point(DevProb P, const int *pts, double *out)
{
    extern __shared__ __align__(16) double dyn[];
    const int lane = threadIdx.x, m = P.d;
    double *xv = dyn, *wv = dyn + m + 8;
    for (int x = lane; x < m; x += 64) {
        const int ix = pts[(size_t)blockIdx.x * m + x] - 1;
        if (FUN == FUN_MVN) xv[x] = P.par[ix] - P.aux[x];
        else { xv[x] = P.par[ix]; wv[x] = P.par[P.n[1] + ix]; }
    }
    __syncthreads();
    const double f = (FUN == FUN_MVN) ? mvn_fast_point_wave(P, xv, lane) : de_fast_point_wave(P.ising_id, m, xv, wv, lane);
    if (lane == 0) out[blockIdx.x] = f;
}

template <int FUN>
static void fb_launch(const DevProb &P, const FbArgs &A, int cap, int64_t npts, const int *dpts, double *dlot, double *dcol, double *drow, double *dnfar, double *dpnt)
{
    const int d = P.d, RM = P.RM;
    hipLaunchKernelGGL(k_fb_tables<FUN>, dim3(2 * RM), dim3(64), sizeof(double) * 2 * (d + 8), 0, P, A);
    const int nn = P.NM, total = A.rL * nn * nn * A.rR;
    hipLaunchKernelGGL(k_fb_lottery<FUN>, dim3((total + TTX_BLK - 1) / TTX_BLK), dim3(TTX_BLK), sizeof(double) * ((2 * (size_t)cap + 1) * RM + 2), 0, P, A, cap, dlot);
    const size_t lds = sizeof(double) * ((size_t)P.npar + 2 + std::max(P.FD, TTX_FNR) + 4 + RM + 2);
    hipLaunchKernelGGL(k_fb_fiber<FUN>, dim3(nn * A.rR), dim3(TTX_BLK), lds, 0, P, A, 1, dcol, dnfar);
    hipLaunchKernelGGL(k_fb_fiber<FUN>, dim3(A.rL * nn), dim3(TTX_BLK), lds, 0, P, A, 0, drow, dnfar + (size_t)nn * A.rR);
    if (npts > 0) hipLaunchKernelGGL(k_fb_point<FUN>, dim3((unsigned)npts), dim3(64), sizeof(double) * 2 * (d + 8), 0, P, dpts, dpnt);
}

extern "C" int ttx_k_fast_block(int32_t device, int32_t fun_id, int32_t d, int32_t n, const double *par, int32_t npar, const double *aux, int32_t naux,
                                int32_t p, int32_t rL, const int32_t *Lidx, int32_t rR, const int32_t *Ridx, int32_t cap, int32_t chain,
                                int64_t npts, const int32_t *pts, double *near, double *dv, double *piv, double *lot, double *colf, double *rowf,
                                double *nfar, double *pnt)
{
    const char *me = "ttx_k_fast_block";
    if (fun_id != TTX_FUN_ISING && fun_id != TTX_FUN_MVN) return fail(TTX_EINVAL, "%s: fun_id %d has no table evaluator", me, fun_id);
    if (!par || !near || !dv || !piv || !lot || !colf || !rowf || !nfar || npts < 0 || (npts > 0 && (!pts || !pnt))) return fail(TTX_EINVAL, "%s: null argument", me);
    if (d < 2 || d > 4096 || n < 1 || n > 1024 || p < 1 || p > d - 1 || rL < 1 || rR < 1 || rL > 64 || rR > 64 || npts > 65535)
        return fail(TTX_EINVAL, "%s: sizes out of range (d %d n %d p %d rL %d rR %d)", me, d, n, p, rL, rR);
    const int FD = d + 1, RM = std::max(rL, rR), A_ = p - 1, B_ = d - p - 1;
    if (cap < 0 || cap > FD) return fail(TTX_EINVAL, "%s: cap %d outside 0..d+1", me, cap);
    if ((A_ > 0 && !Lidx) || (B_ > 0 && !Ridx)) return fail(TTX_EINVAL, "%s: null pivot table", me);
    for (int64_t x = 0; x < (int64_t)rL * A_; x++) if (Lidx[x] < 1 || Lidx[x] > n) return fail(TTX_EINVAL, "%s: left index %d outside 1..n", me, Lidx[x]);
    for (int64_t x = 0; x < (int64_t)rR * B_; x++) if (Ridx[x] < 1 || Ridx[x] > n) return fail(TTX_EINVAL, "%s: right index %d outside 1..n", me, Ridx[x]);
    for (int64_t x = 0; x < npts * d; x++) if (pts[x] < 1 || pts[x] > n) return fail(TTX_EINVAL, "%s: point index %d outside 1..n", me, pts[x]);
    DevProb P{};
    if (fun_id == TTX_FUN_ISING) {
        if (npar < 2 * n + 1) return fail(TTX_EINVAL, "%s: par too short", me);
        P.ising_id = (int)par[2 * n];
        if (P.ising_id != 2 && P.ising_id != 3) return fail(TTX_EINVAL, "%s: Ising id %d has no table evaluator", me, P.ising_id);
        for (int j = 0; j < n; j++) if (!(par[j] >= 0.0 && par[j] <= 1.0)) return fail(TTX_EINVAL, "%s: node %g outside [0,1]", me, par[j]);
    } else {
        if (npar < n || !aux || naux < d + d * d + 1) return fail(TTX_EINVAL, "%s: mvn: par or aux too short", me);
        P.mvn_norm = std::sqrt(powi(2.0 * 3.141592653589793, d) * aux[d + (size_t)d * d]);
        if (!(P.mvn_norm > 0.0) || !std::isfinite(P.mvn_norm)) return fail(TTX_EINVAL, "%s: mvn normalisation is not a positive finite number", me);
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TTX_ENODEV, "no HIP device");
    HIPCHECK(hipSetDevice(device));
    const size_t tn = (size_t)FD * RM, tp = (size_t)TTX_FS * RM, nb = (size_t)rL * n * n * rR, nfib = (size_t)n * rR + (size_t)rL * n;
    // one allocation of doubles: par | aux | auxS | 2 x (near, dv, piv) | the same again (second set) | lot | col | row | nfar | pnt
    std::vector<double> hostd;
    hostd.insert(hostd.end(), par, par + npar);
    const size_t o_aux = hostd.size();
    if (fun_id == TTX_FUN_MVN) {
        hostd.insert(hostd.end(), aux, aux + (d + (size_t)d * d + 1));
        const double *ic = aux + d;
        for (int j = 0; j < d; j++) for (int i = 0; i < d; i++) hostd.push_back(0.5 * (ic[i + (size_t)d * j] + ic[j + (size_t)d * i]));   // as create_integrand_tables
    }
    const size_t o_S = o_aux + (fun_id == TTX_FUN_MVN ? d + (size_t)d * d + 1 : 0), o_tab = hostd.size();
    const size_t o_out = o_tab + 4 * (2 * tn + tp), total = o_out + 3 * nb + nfib + (size_t)npts + 1;
    double *dd = nullptr; int *di = nullptr;
    std::vector<int> hosti(d + 2, n);
    const size_t o_L = hosti.size();
    hosti.insert(hosti.end(), Lidx, Lidx + (size_t)rL * A_);
    const size_t o_R = hosti.size();
    hosti.insert(hosti.end(), Ridx, Ridx + (size_t)rR * B_);
    const size_t o_P = hosti.size();
    hosti.insert(hosti.end(), pts, pts + (size_t)npts * d);
    hosti.push_back(0);
    HIPCHECK(hipMalloc((void **)&dd, sizeof(double) * total));
    if (hipMalloc((void **)&di, sizeof(int) * hosti.size()) != hipSuccess) { (void)hipFree(dd); return fail(TTX_EHIP, "%s: hipMalloc failed", me); }
    int rc = TTX_OK;
    auto chk = [&](hipError_t e, const char *what) { if (e != hipSuccess && rc == TTX_OK) rc = fail(TTX_EHIP, "%s: %s failed: %s", me, what, hipGetErrorString(e)); };
    chk(hipMemset(dd, 0, sizeof(double) * total), "hipMemset");
    chk(hipMemcpy(dd, hostd.data(), sizeof(double) * hostd.size(), hipMemcpyHostToDevice), "hipMemcpy");
    chk(hipMemcpy(di, hosti.data(), sizeof(int) * hosti.size(), hipMemcpyHostToDevice), "hipMemcpy");
    P.d = d; P.RM = RM; P.NM = n; P.G = 1; P.NC = 1; P.fun_id = fun_id; P.npar = npar; P.arith = 1; P.FD = FD; P.fpersist = 0;
    P.n = di; P.par = dd; P.aux = fun_id == TTX_FUN_MVN ? dd + o_aux : nullptr; P.auxS = fun_id == TTX_FUN_MVN ? dd + o_S : nullptr;
    FbArgs A{};
    A.Lidx = di + o_L; A.Ridx = di + o_R; A.rL = rL; A.rR = rR; A.p = p; A.chain = chain ? 1 : 0;
    double *t = dd + o_tab;
    for (int sd = 0; sd < 2; sd++) { P.fNear[sd] = t; t += tn; }
    for (int sd = 0; sd < 2; sd++) { P.fDv[sd] = t; t += tn; }
    for (int sd = 0; sd < 2; sd++) { P.fPiv[sd] = t; t += tp; }
    for (int sd = 0; sd < 2; sd++) { A.tNear[sd] = t; t += tn; }
    for (int sd = 0; sd < 2; sd++) { A.tDv[sd] = t; t += tn; }
    for (int sd = 0; sd < 2; sd++) { A.tPiv[sd] = t; t += tp; }
    double *dlot = dd + o_out, *dcol = dlot + nb, *drow = dcol + nb, *dnfar = drow + nb, *dpnt = dnfar + nfib;
    if (rc == TTX_OK) {
        if (fun_id == TTX_FUN_ISING) fb_launch<FUN_ISING>(P, A, cap, npts, di + o_P, dlot, dcol, drow, dnfar, dpnt);
        else fb_launch<FUN_MVN>(P, A, cap, npts, di + o_P, dlot, dcol, drow, dnfar, dpnt);
        chk(hipGetLastError(), "launch");
        chk(hipDeviceSynchronize(), "hipDeviceSynchronize");
    }
    if (rc == TTX_OK) {
        chk(hipMemcpy(near, P.fNear[0], sizeof(double) * 2 * tn, hipMemcpyDeviceToHost), "hipMemcpy");
        chk(hipMemcpy(dv, P.fDv[0], sizeof(double) * 2 * tn, hipMemcpyDeviceToHost), "hipMemcpy");
        chk(hipMemcpy(piv, P.fPiv[0], sizeof(double) * 2 * tp, hipMemcpyDeviceToHost), "hipMemcpy");
        chk(hipMemcpy(lot, dlot, sizeof(double) * nb, hipMemcpyDeviceToHost), "hipMemcpy");
        chk(hipMemcpy(colf, dcol, sizeof(double) * nb, hipMemcpyDeviceToHost), "hipMemcpy");
        chk(hipMemcpy(rowf, drow, sizeof(double) * nb, hipMemcpyDeviceToHost), "hipMemcpy");
        chk(hipMemcpy(nfar, dnfar, sizeof(double) * nfib, hipMemcpyDeviceToHost), "hipMemcpy");
        if (npts > 0) chk(hipMemcpy(pnt, dpnt, sizeof(double) * npts, hipMemcpyDeviceToHost), "hipMemcpy");
    }
    (void)hipFree(dd); (void)hipFree(di);
    return rc;
}
