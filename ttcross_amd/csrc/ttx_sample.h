// ttx_sample.h -- samples drawn from the resident tensor train by sequential conditional sampling (ttx_sample / ttx_sample_dev).
//
// The definition is in include/ttx.h.  Modes are drawn from the last to the first, so the running state is dtt_ijk's own chain
// (k_ev_exact, ttx_eval.h) and the value of the train at the drawn index falls out of the draw.  Per call:
//   k_ct_modesum, k_ct_chains (ttx_contract.h, unchanged) form the prefix vectors l_k from the effective weights
//   k_sm_head   all head tables H_k(i, b) = w_k(i) sum_a l_(k-1)(a) G_k(a, i, b) in one launch; table k is stored [b][i], i contiguous
//   k_sm_draw   one wave per sample: per drawn mode p(i) = |sum_b H_k(i, b) x(b)| with lanes along i, a wave scan, the search
//               for the index, then the state update of k_ev_exact (sm_chain_step)
//   k_sm_count  the failed samples of a chunk (their index rows start with 0), added to the call's counter by one workgroup
// No atomics, and no sum whose order depends on the grid, the chunk or the other samples: a call repeats bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include "ttx_eval.h"      // EvTrain
#include "ttx_contract.h"  // CtCore
#include "ttx_wave.h"      // wave_scan

#define TTX_SM_LDSROW 1024          // modes up to this size keep their row of p in LDS (8 KB per wave); longer ones use the call's global rows
#define TTX_SM_TILE 4096            // products one work item of k_sm_head stages in LDS (before the odd row padding)
#define TTX_SM_HLDS 4352            // doubles of LDS k_sm_head owns: the largest tile, r0 = 16: 256 rows of 17

struct SmTile { int c, b, i0, ni; };        // core (0-based mode), slab b, indices i0 .. i0 + ni - 1

// rows of one tile of k_sm_head for a core with r0 rows: 256 threads sum one row each, the image stays within TTX_SM_TILE products
__host__ __device__ inline int sm_tile_rows(int r0) { const int t = TTX_SM_TILE / r0; return t < 256 ? t : 256; }

// One work item = (core k, slab b, up to sm_tile_rows indices i).  Phase 1 streams the tile, lanes along the contiguous a, and
// leaves the products l(a) G(a, i, b) in LDS (row i at i (r0 | 1): the odd stride keeps phase 2 free of bank conflicts); phase 2
// has one thread per i, which adds its row over ascending a from 0.0 and multiplies by w(i).  Padding is never read.
__global__ __launch_bounds__(256) void k_sm_head(const CtCore *cores, const SmTile *tiles, int RM, size_t SS, const double *w, const double *L, int ldv,
                                                 const size_t *hoff, double *H)
{
    __shared__ double prod[TTX_SM_HLDS];
    __shared__ double lv[128];
    const SmTile t = tiles[blockIdx.x];
    const CtCore c = cores[t.c];
    const int tid = threadIdx.x, stride = c.r0 | 1, rows = 256 / c.ta, al = tid & (c.ta - 1);
    if (tid < c.r0) lv[tid] = L[(size_t)t.c * ldv + tid];
    __syncthreads();
    const double *G = c.src + (size_t)RM * t.i0 + SS * t.b;
    for (int ii = tid / c.ta; ii < t.ni; ii += rows)
        for (int a = al; a < c.r0; a += 64) prod[ii * stride + a] = lv[a] * G[a + (size_t)RM * ii];
    __syncthreads();
    if (tid < t.ni) {
        const double *q = prod + tid * stride;
        double s = 0.0;
#pragma unroll 8
        for (int a = 0; a < c.r0; a++) s = s + q[a];
        H[hoff[t.c] + (size_t)t.b * c.n + t.i0 + tid] = w[c.woff + t.i0 + tid] * s;
    }
}

// z = A x for the slice A = G(:, j, :) (q0 x q1, element (a, b) at A[a + SS b]): the inner loop of k_ev_exact -- sums from 0.0
// over ascending b, separate multiply and add, two rows per lane above rank 64 -- so a chain of these steps gives dtt_ijk's bits
__device__ inline void sm_chain_step(const double *A, size_t SS, int q0, int q1, const double *x, double *z, int lane)
{
    if (q0 <= 64) {
        if (lane < q0) {
            double s = 0.0;
#pragma unroll 8
            for (int k = 0; k < q1; k++) s = s + A[lane + SS * k] * x[k];
            z[lane] = s;
        }
    } else {
        const bool two = lane + 64 < q0;
        const double *A1 = two ? A + 64 : A;
        double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
        for (int k = 0; k < q1; k++) { const double xk = x[k]; s0 = s0 + A[lane + SS * k] * xk; s1 = s1 + A1[lane + SS * k] * xk; }
        z[lane] = s0;
        if (two) z[lane + 64] = s1;
    }
}

// A sample's row of uniforms u[0 .. d-1]: true if a drawn mode (held(i) false) has a NaN or a negative u, which refuses the sample.
// us (may be null): the wave's copy of the row
template <class Held>
__device__ inline bool sm_bad_u(const double *u, int d, int lane, Held held, double *us)
{
    bool badu = false;
    for (int i = lane; i < d; i += 64) { const double uu = u[i]; if (us) us[i] = uu; badu |= !held(i) && !(uu >= 0.0); }   // NaN or negative
    return __ballot(badu) != 0;
}

// The search of the cell samplers (k_sr_draw, k_sqr_pick) among the masses e(0 .. n-1) >= 0 of a sample's cells, lanes along i in rounds
// of 64, by the rules of the index search in k_sm_draw and k_sq_pick.  first(i) and again(i) give e(i), and 0.0 for i >= n, in the first
// and in the second pass.  Pass one: the total and the last positive entry.  Pass two (u < 1): the first i with e(i) > 0 and t < c(i),
// t = u total, c the inclusive running sum.  Where there is none, or u >= 1, the largest i with e(i) > 0 is chosen.  A total that is
// 0, NaN or Inf, or no positive entry, fails the sample.  Every lane of the wave takes part and gets the same answer; a position
// comes from lane numbers alone, never from a value.  The running sum is carried from round to round through lane 63.
// k_sm_draw and k_sq_pick keep these loops written out: through a shared helper k_sm_draw kept eight more scalars in vector lanes
// and its draws took 0.2 % longer, k_sq_pick's picks 0.15 % (profiles/sampler_frame_mi355x.txt); a change of a rule is made in all three.
//
// ok: false if the sample fails (nothing else is set then).  pos: the chosen cell; hit: it came from the second pass, and then
// at = e(pos) and before = c(pos - 1), from which the cell samplers invert inside the cell (sr_mass_within).
struct SmFound { bool ok, hit; int pos; double total, t, at, before; };

template <class First, class Again>
__device__ inline SmFound sm_wave_search(int n, double u, int lane, First first, Again again)
{
    SmFound f{false, false, -1, 0.0, 0.0, 0.0, 0.0};
    double carry = 0.0;
    for (int i0 = 0; i0 < n; i0 += 64) {                                        // e, and the total c(n-1)
        const double e = first(i0 + lane);
        carry = __shfl(carry + wave_scan(e, lane), 63);
        const unsigned long long pos = __ballot(e > 0.0);
        if (pos) f.pos = i0 + 63 - __builtin_clzll(pos);
    }
    f.total = carry;
    if (!(f.total > 0.0) || f.total == __builtin_inf() || f.pos < 0) return f;  // 0, NaN or Inf
    f.ok = true;
    f.t = u * f.total;
    if (u < 1.0) {                                                              // else, or with no i with t < c(i): the largest i with e > 0
        carry = 0.0;
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + lane;
            const double e = again(i), c = carry + wave_scan(e, lane);
            const unsigned long long hit = __ballot(i < n && e > 0.0 && f.t < c);
            if (hit) {
                const int fl = __builtin_ctzll(hit);
                f.hit = true; f.pos = i0 + fl; f.at = __shfl(e, fl); f.before = fl ? __shfl(c, fl - 1) : carry;
                break;
            }
            carry = __shfl(c, 63);
        }
    }
    return f;
}

// The way back (k_sqr_cdf): for a given position pos in 0 .. n-1, the same in every lane, total = c(n-1) and before = c(pos - 1)
// (0.0 for pos = 0) of the inclusive running sum c of e(0 .. n-1), in sm_wave_search's association: a wave scan per round of 64, the
// carry through lane 63.  total has the bits of the search's f.total and before those of its f.before for the same e.  One pass,
// no search: every lane takes part and gets the same answer.  A pos outside 0 .. n-1 leaves before at 0.0.
struct SmBefore { double total, before; };

template <class Mass>
__device__ inline SmBefore sm_wave_before(int n, int pos, int lane, Mass mass)
{
    SmBefore f{0.0, 0.0};
    double carry = 0.0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const double c = carry + wave_scan(mass(i0 + lane), lane);
        const int fl = pos - i0;                                                // wave-uniform: no lane diverges
        if (fl >= 0 && fl < 64) f.before = fl ? __shfl(c, fl - 1) : carry;
        carry = __shfl(c, 63);
    }
    f.total = carry;
    return f;
}

// One wave per sample, grid-stride.  Dynamic LDS per wave: x[ldx], z[ldx], the sample's row of u [d], its index row [d] and the
// row of p of the current mode [ldsrow]; nothing is shared between waves, so there is no workgroup barrier.  A mode longer than
// ldsrow keeps its row in grow (growlen doubles per wave of the grid).  A lane reads back only the entries of the row it wrote
// itself, what other lanes need travels by wave shuffles.  The index comes from lane numbers alone, never from a value: whatever
// the cores hold, it lies in 0 .. n(k) - 1 and every read stays inside its table.
__global__ __launch_bounds__(256) void k_sm_draw(EvTrain T, const size_t *hoff, const int *fixed, const double *H, int ldsrow, double *grow, size_t growlen,
                                                 long long npts, const double *u, int *ind, double *logq, double *val)
{
    extern __shared__ __align__(16) double sm_dyn[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6, d = T.d;
    const size_t per = 2 * (size_t)T.ldx + d + (((size_t)d + 1) >> 1) + ldsrow;
    double *xb = sm_dyn + per * wave, *us = xb + 2 * T.ldx, *lrow = us + d + (((size_t)d + 1) >> 1);
    int *id = (int *)(us + d);
    double *wrow = grow ? grow + growlen * ((size_t)blockIdx.x * nw + wave) : nullptr;
    for (long long p = (long long)blockIdx.x * nw + wave; p < npts; p += (long long)gridDim.x * nw) {
        double *x = xb, *z = xb + T.ldx;
        __builtin_amdgcn_wave_barrier();
        bool badu = false;
        for (int i = lane; i < d; i += 64) { const double uu = u[(size_t)p * d + i]; us[i] = uu; badu |= !fixed[i] && !(uu >= 0.0); }   // NaN or negative
        bool fail = __ballot(badu) != 0;
        if (lane == 0) x[0] = 1.0;                                              // x_(d+1) = [1]
        double lq = 0.0;
        __builtin_amdgcn_wave_barrier();
        for (int k = d - 1; k >= 0 && !fail; k--) {
            const int q0 = T.r[k], q1 = T.r[k + 1], n = T.n[k];
            int ik = fixed[k] - 1;
            if (ik < 0) {
                const double *Hk = H + hoff[k];
                double *row = n <= ldsrow ? lrow : wrow;
                const double uk = us[k];
                double carry = 0.0, plast = 0.0;
                int last = -1;
                for (int i0 = 0; i0 < n; i0 += 64) {                            // p, and the total c(n)
                    const int i = i0 + lane;
                    double pi = 0.0;
                    if (i < n) {
                        double m = 0.0;
#pragma unroll 4
                        for (int b = 0; b < q1; b++) m = m + Hk[(size_t)b * n + i] * x[b];
                        pi = fabs(m);
                        row[i] = pi;
                    }
                    carry = __shfl(carry + wave_scan(pi, lane), 63);
                    const unsigned long long pos = __ballot(pi > 0.0);
                    if (pos) { const int hl = 63 - __builtin_clzll(pos); last = i0 + hl; plast = __shfl(pi, hl); }
                }
                const double total = carry;
                if (!(total > 0.0) || total == __builtin_inf() || last < 0) { fail = true; break; }   // 0, NaN or Inf
                const double t = uk * total;
                double psel = plast;
                ik = last;                                                      // u >= 1, or no i with t < c(i): the largest i with p > 0
                if (uk < 1.0) {
                    carry = 0.0;
                    for (int i0 = 0; i0 < n; i0 += 64) {
                        const int i = i0 + lane;
                        const double pi = i < n ? row[i] : 0.0, c = carry + wave_scan(pi, lane);
                        const unsigned long long hit = __ballot(i < n && pi > 0.0 && t < c);
                        if (hit) { const int fl = __builtin_ctzll(hit); ik = i0 + fl; psel = __shfl(pi, fl); break; }
                        carry = __shfl(c, 63);
                    }
                }
                lq = lq + log(psel / total);
            }
            if (lane == 0) id[k] = ik + 1;
            const double *A = T.core[k] + (size_t)T.RM * ik;
            if (k == d - 1) { for (int a = lane; a < q0; a += 64) z[a] = A[a]; }     // x_d = G_d(:, i_d, 1), a copy as in k_ev_exact
            else sm_chain_step(A, T.SS, q0, q1, x, z, lane);
            __builtin_amdgcn_wave_barrier();
            double *t_ = x; x = z; z = t_;
        }
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < d; i += 64) ind[(size_t)p * d + i] = fail ? 0 : id[i];
        if (lane == 0) {
            if (logq) logq[p] = fail ? __builtin_nan("") : lq;
            if (val) val[p] = fail ? 0.0 : x[0];
        }
    }
}

// cnt[0] += samples of the chunk whose index row starts with 0 (the failed ones); one workgroup, launched chunk after chunk on one stream
__global__ __launch_bounds__(1024) void k_sm_count(long long npts, int d, const int *ind, long long *cnt)
{
    __shared__ long long part[1024];
    long long s = 0;
    for (long long p = threadIdx.x; p < npts; p += 1024) s += ind[(size_t)p * d] == 0;
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 512; o; o >>= 1) { if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) cnt[0] += part[0];
}
