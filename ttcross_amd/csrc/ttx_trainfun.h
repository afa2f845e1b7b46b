// ttx_trainfun.h -- TTX_FUN_TRAINS: the integrand of a sweep is a function of resident trains, fun(i) = g(x_1(i), .., x_m(i)).
//
// The sweep is the two-pass one of TTX_FUN_HOST / TTX_FUN_DEVICE (include/ttx_device_fun.h): pass 1 raises slots, k_tf_slots fills
// them on the engine's stream, pass 2 reads them.  A slot's value needs one element of every operand: the chain of k_ev_exact
// (ttx_eval.h) through sm_chain_step (ttx_sample.h), x = U_d(:, i_d, 1), then i = d-1 .. 1 with sums from 0.0 over ascending k and a
// separate multiply and add -- so operand t contributes ttx_ijk_batch(x_t, ind, TTX_EVAL_EXACT) bit for bit, and the built-in
// combiners are single IEEE operations in the order include/ttx.h writes them.
//
// Launch shape: one wave64 per raised slot, 4 waves per workgroup, a capped grid that strides.  Per wave the dynamic LDS holds two
// state vectors of the largest ldx over the operands, the slot's index row as ints and the m operand values: nothing is shared
// between waves, wave barriers only.
// Empty stretches: the sweep raises dense runs at the start of each bond group's slots and leaves holes behind them.  A wave does
// not test its slots one by one: the 64 lanes read the flags of the NEXT 64 slots this wave would visit in grid-stride order
// (slot (64 j + lane) NW + w for wave w of NW), one ballot gives the raised ones, and the wave walks the set bits.  A dense run
// of K slots is still spread over min(K, NW) waves, and 64 empty slots cost a wave one byte load per lane and one ballot.
#pragma once
#include <hip/hip_runtime.h>
#include "ttx_sample.h"     // sm_chain_step

#define TTX_TF_MAX 8                // TTX_TRAINS_MAX of include/ttx.h
#define TTX_TF_WAVES 4
// the combiners (TTX_TOP_* of include/ttx.h); TF_DEVICE: the values go to tval, a loaded combiner kernel runs behind
enum { TF_PRODUCT = 1, TF_RATIO = 2, TF_SQRTABS = 3, TF_DEVICE = 4 };

// one operand as the chain sees it: what EvTrain holds, with the operand's OWN layout (row stride RM, slab stride SS)
struct TfTrain {
    int RM;
    size_t SS;
    const double *const *core;      // [d], 0-based mode
    const int *r;                   // [d+1]
};
struct TfOps {
    int m, d, ldx;                  // operands, cores, doubles per state vector (largest rank over the operands, rounded up to 4)
    const int *n;                   // [d] the engine's mode sizes (equal to every operand's)
    TfTrain t[TTX_TF_MAX];
};
// doubles of dynamic LDS per wave: x[ldx], z[ldx], id[d] ints, val[TTX_TF_MAX]
__host__ __device__ inline size_t tf_lds_doubles(int ldx, int d) { return 2 * (size_t)ldx + (((size_t)d + 1) >> 1) + TTX_TF_MAX; }

// the m operand values at the index row id[0 .. d-1] (1-based, already in this wave's LDS, checked against n) into val[0 .. m-1]
__device__ inline void tf_chains(const TfOps &O, const int *id, double *x, double *z, double *val, int lane)
{
    const int d = O.d;
    for (int t = 0; t < O.m; t++) {
        const TfTrain &T = O.t[t];
        double *xa = x, *za = z;
        {
            const int q0 = T.r[d - 1];
            const double *A = T.core[d - 1] + (size_t)T.RM * (id[d - 1] - 1);
            for (int a = lane; a < q0; a += 64) xa[a] = A[a];
        }
        __builtin_amdgcn_wave_barrier();
        for (int i = d - 2; i >= 0; i--) {
            sm_chain_step(T.core[i] + (size_t)T.RM * (id[i] - 1), T.SS, T.r[i], T.r[i + 1], xa, za, lane);
            __builtin_amdgcn_wave_barrier();
            double *s_ = xa; xa = za; za = s_;
        }
        if (lane == 0) val[t] = xa[0];
        __builtin_amdgcn_wave_barrier();
    }
}
template <int OP>
__device__ inline double tf_combine(int m, const double *v)
{
    if (OP == TF_RATIO) return v[0] / v[1];
    if (OP == TF_SQRTABS) return sqrt(fabs(v[0]));
    double p = v[0];
    for (int t = 1; t < m; t++) p = p * v[t];
    return p;
}
// an index row into the wave's LDS; true when every entry lies in 1..n (wave-uniform)
template <class I>
__device__ inline bool tf_load_row(const TfOps &O, const I *row, int *id, int lane)
{
    bool bad = false;
    for (int i = lane; i < O.d; i += 64) { const int v = (int)row[i]; id[i] = v; bad |= (v <= 0 || v > O.n[i]); }
    const bool ok = __ballot(bad) == 0ull;
    __builtin_amdgcn_wave_barrier();
    return ok;
}

// ---- the slot kernel: behind pass 1 on the engine's stream ------------------------------------------------------------------------
// Built-in OP: hval[s] = g(values), THEN hreq[s] = 0.  TF_DEVICE: tval[s][0 .. m-1] = values, the flag stays raised for the loaded
// combiner.  A row with an entry outside 1..n (the sweep writes none) reads no core and gives NaN.
template <int OP>
__global__ __launch_bounds__(64 * TTX_TF_WAVES) void k_tf_slots(TfOps O, long long nslot, const short *hidx, unsigned char *hreq, double *hval, double *tval,
                                                                  unsigned long long *cnt)
{
    extern __shared__ __align__(16) double tf_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, d = O.d;
    double *x = tf_dyn + tf_lds_doubles(O.ldx, d) * wave, *z = x + O.ldx;
    int *id = (int *)(x + 2 * O.ldx);
    double *val = x + 2 * O.ldx + ((d + 1) >> 1);
    const long long nw = (long long)gridDim.x * TTX_TF_WAVES, w = (long long)blockIdx.x * TTX_TF_WAVES + wave;
    unsigned long long done = 0;
    for (long long base = w; base < nslot; base += 64 * nw) {
        const long long mine = base + (long long)lane * nw;
        unsigned long long todo = __ballot(mine < nslot && hreq[mine] != 0);
        done += __popcll(todo);
        while (todo) {
            const int b = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const long long s = base + (long long)b * nw;
            __builtin_amdgcn_wave_barrier();
            const bool ok = tf_load_row(O, hidx + (size_t)s * d, id, lane);
            if (ok) tf_chains(O, id, x, z, val, lane);
            if (OP == TF_DEVICE) {
                if (lane < O.m) tval[(size_t)s * O.m + lane] = ok ? val[lane] : __builtin_nan("");
            } else if (lane == 0) {
                hval[s] = ok ? tf_combine<OP>(O.m, val) : __builtin_nan("");
                hreq[s] = 0;
            }
        }
    }
    if (lane == 0 && done) atomicAdd(cnt, done);        // the elements this launch evaluated (ttx_trainfun_last): one add per busy wave
}

// ---- the list twin (ttx_eval_device): one wave per point of a 32-bit index list -----------------------------------------------------
// the host entry refuses an index outside the modes before anything is launched; a row that is out of range all the same reads no core
template <int OP>
__global__ __launch_bounds__(64 * TTX_TF_WAVES) void k_tf_list(TfOps O, long long npts, const int *ind, double *out, double *tval, unsigned long long *cnt)
{
    extern __shared__ __align__(16) double tf_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, d = O.d;
    double *x = tf_dyn + tf_lds_doubles(O.ldx, d) * wave, *z = x + O.ldx;
    int *id = (int *)(x + 2 * O.ldx);
    double *val = x + 2 * O.ldx + ((d + 1) >> 1);
    const long long nw = (long long)gridDim.x * TTX_TF_WAVES;
    unsigned long long done = 0;
    for (long long p = (long long)blockIdx.x * TTX_TF_WAVES + wave; p < npts; p += nw) {
        done++;
        __builtin_amdgcn_wave_barrier();
        const bool ok = tf_load_row(O, ind + (size_t)p * d, id, lane);
        if (ok) tf_chains(O, id, x, z, val, lane);
        if (OP == TF_DEVICE) {
            if (lane < O.m) tval[(size_t)p * O.m + lane] = ok ? val[lane] : __builtin_nan("");
        } else if (lane == 0)
            out[p] = ok ? tf_combine<OP>(O.m, val) : __builtin_nan("");
    }
    if (lane == 0 && done) atomicAdd(cnt, done);
}
