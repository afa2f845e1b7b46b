// ttx_coscoeff.h -- the COS-coefficient integrand of the fork's option-pricing driver, one evaluation order for host and device.
//
// test_crs_coscoeff.f90 cross-approximates calc_coefficient (lib/coefficients.f90) over the multi-index ind(1:d):
//
//   f(ind) = 2 (1/(b-a))^d  sum_{s in S}  Re( exp(-i a sum_j t_j) * phi(t) ),   t_j = pi s_j (ind_j - 1) / (b-a),
//   phi(t) = exp(i t'mu - t'Sigma t / 2)     (gaussian_chf_nd, lib/funcs.f90),
//
// S the 2^(d-1) sign vectors of generate_s_vectors (lib/s_vectors.f90): s_1 = +1, s_j = -1 iff bit j-2 of the vector number is set,
// vector numbers ascending.  ttx_coscoeff_eval below evaluates, per element, operation for operation:
//
//   ob        = 1 / (b - a)
//   factor    = 2 * ob^d                              (ob^d by binary powering, as the compiler's integer power)
//   T_j       = (pi * (ind_j - 1)) * ob               t_j = ((pi*s_j)*(ind_j-1))*ob = s_j T_j exactly (negation is exact)
//   M_j       = T_j * mu_j                            t_j mu_j = s_j M_j
//   P_ij      = Sigma_ij * T_j                        Sigma_ij t_j = s_j P_ij
//   for each s, in generation order:
//     dot_mu  = ((0 + s_1 M_1) + s_2 M_2) + ...       sum(omega*mu), j ascending
//     y_i     = ((0 + s_1 P_i1) + s_2 P_i2) + ...     matmul(sigma, omega), j ascending
//     q       = ((0 + y_1 t_1) + y_2 t_2) + ...       sum(matmul(...) * omega), y_i t_i = s_i (y_i T_i)
//     st      = ((0 + t_1) + t_2) + ...               sum(t)
//     phi     = cexp(-0.5 q + i dot_mu)   = (E cos(dot_mu), E sin(dot_mu)),  E = exp(-0.5 q)   (glibc cexp: e^x cos y, e^x sin y)
//     e_term  = cexp(+-0 - i (a st))      = (cos(a st), -sin(a st))                           (e^0 = 1; cos even, sin odd)
//     term    = Re(e_term * phi) = ac - bd = cos(a st) * (E cos dot_mu) - (-sin(a st)) * (E sin dot_mu)
//     real_sum = real_sum + term
//   f = factor * real_sum
//
// So the sign-vector loop needs only additions of sign-flipped products formed once per element, and gives the same bits as the
// naive order.  No FP contraction anywhere (the library and the tests compile with -ffp-contract=off).
//
// exp is ttx_exp (ttx_exp.h), bit-identical to glibc's.  sin and cos are the project's own (ttx_sin / ttx_cos below): glibc's
// sin/cos (IBM Accurate Mathematical Library, dbl-64/s_sin.c) cannot be restated here, its source is not part of this project's
// inputs, so unlike exp they are NOT bit-identical to the run-time library: they stay within 1 ulp of it over |x| <= TTX_TRIG_MAX
// (tests/test_coscoeff_cpu.py), and ttx_create refuses problems whose arguments could leave that range.  The consequence: the
// device integrand equals this restatement bit for bit, and the genuine reference's values to rounding (tests/golden/coscoeff_*).
//
// sin / cos: Cody-Waite reduction x = k pi/2 + r with pi/2 = C1 + C2 + C3 + C4 (33-bit pieces: k Ci is exact for k < 2^20), the
// reduced argument as an exact-sum pair (y0, y1), then the minimax kernels of gen_trig_coef.py on |r| <= pi/4.  Both functions
// work on |x|: sin(-x) = -sin(x) and cos(-x) = cos(x) hold exactly.
#pragma once
#include <stdint.h>
#include "ttx_exp.h"
#include "ttx_trig_coef.h"

#if defined(__HIPCC__)
#define TTX_CC_HD __host__ __device__ inline
#else
#define TTX_CC_HD static inline
#endif

#define TTX_TRIG_MAX 0x1p19          // |x| accepted by ttx_sin / ttx_cos: quadrant numbers stay below 2^19
#define TTX_COSCOEFF_MAXD 20         // ttx_create: 2^(d-1) sign vectors per element bound one launch's time
#define TTX_COSCOEFF_PI 3.14159265358979323846   // constants.f90: pi

// a + b = s + e exactly (Knuth's two-sum)
TTX_CC_HD double ttx_two_sum(double a, double b, double *e)
{
    const double s = a + b;
    const double bb = s - a;
    *e = (a - (s - bb)) + (b - bb);
    return s;
}

// ax >= 0, ax <= TTX_TRIG_MAX: ax = k pi/2 + y0 + y1, |y0| <= ~pi/4; returns k mod 4
TTX_CC_HD int ttx_trig_reduce(double ax, double *y0, double *y1)
{
    if (ax <= TTX_TRIG_PIO4) { *y0 = ax; *y1 = 0.0; return 0; }
    const double shift = 0x1.8p52;
    const double kd = (ax * TTX_TRIG_INVPIO2 + shift) - shift;      // nearest integer (ties to even)
    const double r = ax - kd * TTX_TRIG_PIO2_C1;                      // exact: k C1 is exact, and ax, k C1 lie within a factor 2
    double e1, e2;
    double hi = ttx_two_sum(r, -(kd * TTX_TRIG_PIO2_C2), &e1);        // k C2, k C3 exact
    hi = ttx_two_sum(hi, -(kd * TTX_TRIG_PIO2_C3), &e2);
    const double lo = (e1 + e2) - kd * TTX_TRIG_PIO2_C4;
    double t;
    *y0 = ttx_two_sum(hi, lo, &t);
    *y1 = t;
    return (int)((int64_t)kd & 3);
}

// kernels on the pair (x, y), |x + y| <= ~pi/4
TTX_CC_HD double ttx_trig_ksin(double x, double y)
{
    const double z = x * x;
    const double v = z * x;
    const double r = TTX_TRIG_S2 + z * (TTX_TRIG_S3 + z * (TTX_TRIG_S4 + z * (TTX_TRIG_S5 + z * TTX_TRIG_S6)));
    return x - ((z * (0.5 * y - v * r) - y) - v * TTX_TRIG_S1);
}
TTX_CC_HD double ttx_trig_kcos(double x, double y)
{
    const double z = x * x;
    const double r = z * (TTX_TRIG_K1 + z * (TTX_TRIG_K2 + z * (TTX_TRIG_K3 + z * (TTX_TRIG_K4 + z * (TTX_TRIG_K5 + z * TTX_TRIG_K6)))));
    const double hz = 0.5 * z;
    const double w = 1.0 - hz;
    return w + (((1.0 - w) - hz) + (z * r - x * y));
}

TTX_CC_HD double ttx_sin(double x)
{
    const double ax = x < 0.0 ? -x : x;
    double y0, y1;
    const int k = ttx_trig_reduce(ax, &y0, &y1);
    double s = (k & 1) ? ttx_trig_kcos(y0, y1) : ttx_trig_ksin(y0, y1);
    if (k & 2) s = -s;
    return x < 0.0 ? -s : s;
}
TTX_CC_HD double ttx_cos(double x)
{
    const double ax = x < 0.0 ? -x : x;
    double y0, y1;
    const int k = ttx_trig_reduce(ax, &y0, &y1);
    double c = (k & 1) ? ttx_trig_ksin(y0, y1) : ttx_trig_kcos(y0, y1);
    if (((k + 1) & 2) != 0) c = -c;                                   // k = 1: -sin, k = 2: -cos
    return c;
}

// ob^d, the binary powering of the compiler's integer power (as powi in ttx_engine.hip)
TTX_CC_HD double ttx_coscoeff_powi(double a, int b)
{
    double r = 1.0;
    for (;;) { if (b & 1) r *= a; b /= 2; if (b == 0) break; a *= a; }
    return r;
}

// the element's per-s work: T, M, P formed (d, d, d*d doubles: P[i + d*j] = Sigma_ij T_j), sign vector s given by its number sv;
// returns the term Re(e_term * phi), *mag = E (an upper bound of |term|, for the tests' tolerance)
TTX_CC_HD double ttx_coscoeff_term(int d, const double *T, const double *M, const double *P, double a, uint32_t sv, double *mag)
{
    double dot_mu = 0.0, q = 0.0, st = 0.0;
    for (int j = 0; j < d; j++) {
        const int neg = j > 0 && ((sv >> (j - 1)) & 1u);
        dot_mu = dot_mu + (neg ? -M[j] : M[j]);
    }
    for (int i = 0; i < d; i++) {
        double y = 0.0;
        for (int j = 0; j < d; j++) {
            const int neg = j > 0 && ((sv >> (j - 1)) & 1u);
            y = y + (neg ? -P[i + d * j] : P[i + d * j]);
        }
        const int ni = i > 0 && ((sv >> (i - 1)) & 1u);
        const double yt = y * T[i];
        q = q + (ni ? -yt : yt);
        st = st + (ni ? -T[i] : T[i]);
    }
    const double E = ttx_exp(-0.5 * q);
    const double w = a * st;
    const double re_phi = E * ttx_cos(dot_mu), im_phi = E * ttx_sin(dot_mu);
    const double re_e = ttx_cos(w), im_e = -ttx_sin(w);
    if (mag) *mag = E;
    return re_e * re_phi - im_e * im_phi;
}

// T, M, P of one element (ind 1-based); aux = [mu(1:d), Sigma(1:d,1:d) column-major, a, b]
TTX_CC_HD void ttx_coscoeff_prep(int d, const int32_t *ind, const double *aux, double *T, double *M, double *P)
{
    const double a = aux[d + d * d], b = aux[d + d * d + 1];
    const double ob = 1.0 / (b - a);
    for (int j = 0; j < d; j++) { T[j] = (TTX_COSCOEFF_PI * (double)(ind[j] - 1)) * ob; M[j] = T[j] * aux[j]; }
    for (int j = 0; j < d; j++)
        for (int i = 0; i < d; i++) P[i + d * j] = aux[d + i + d * j] * T[j];
}

TTX_CC_HD double ttx_coscoeff_factor(int d, const double *aux)
{
    const double ob = 1.0 / (aux[d + d * d + 1] - aux[d + d * d]);
    return 2.0 * ttx_coscoeff_powi(ob, d);
}

// calc_coefficient(d, ind, n) on one thread (d <= TTX_COSCOEFF_MAXD); abssum (may be NULL): factor * sum over s of E
TTX_CC_HD double ttx_coscoeff_eval(int d, const int32_t *ind, const double *aux, double *abssum)
{
    double T[TTX_COSCOEFF_MAXD], M[TTX_COSCOEFF_MAXD], P[TTX_COSCOEFF_MAXD * TTX_COSCOEFF_MAXD];
    ttx_coscoeff_prep(d, ind, aux, T, M, P);
    const double a = aux[d + d * d];
    const uint32_t ns = 1u << (d - 1);
    double real_sum = 0.0, mags = 0.0;
    for (uint32_t sv = 0; sv < ns; sv++) {
        double mg;
        real_sum = real_sum + ttx_coscoeff_term(d, T, M, P, a, sv, &mg);
        mags = mags + mg;
    }
    const double factor = ttx_coscoeff_factor(d, aux);
    if (abssum) *abssum = factor * mags;
    return factor * real_sum;
}

#if defined(__HIPCC__)
#include "ttx_de.h"        // lds_sum_chain

// ---- device: one wave64 per element ------------------------------------------------------------------------------------------
// The wave forms T, M, P of its element in LDS (lane-parallel), then walks the sign vectors in chunks of 64, one per lane; each
// lane evaluates ttx_coscoeff_term (the P_ij reads are wave-uniform LDS broadcasts) and parks its term in LDS, and every lane adds
// the chunk's terms into the running sum in generation order (lds_sum_chain of ttx_de.h) -- the host loop's sequence exactly.
// LDS per wave: TTX_CC_LDS(d) doubles.
#define TTX_CC_LDS(d) (2 * (d) + (d) * (d) + 64)
#define TTX_CC_WAVES 4                // waves per workgroup of the coscoeff kernels

template <class IND>
__device__ __forceinline__ double coscoeff_wave(int d, const double *aux, const IND *row, double *lds, int lane)
{
    double *T = lds, *M = T + d, *P = M + d, *tb = P + d * d;
    const double a = aux[d + d * d], b = aux[d + d * d + 1];
    const double ob = 1.0 / (b - a);
    __builtin_amdgcn_wave_barrier();
    if (lane < d) { const double t = (TTX_COSCOEFF_PI * (double)((int)row[lane] - 1)) * ob; T[lane] = t; M[lane] = t * aux[lane]; }
    __builtin_amdgcn_wave_barrier();
    for (int x = lane; x < d * d; x += 64) P[x] = aux[d + x] * T[x / d];       // P[i + d*j] = Sigma_ij T_j
    __builtin_amdgcn_wave_barrier();
    const uint32_t ns = 1u << (d - 1);
    double real_sum = 0.0;
    for (uint32_t c0 = 0; c0 < ns; c0 += 64) {
        const uint32_t sv = c0 + (uint32_t)lane;
        const double term = sv < ns ? ttx_coscoeff_term(d, T, M, P, a, sv, nullptr) : 0.0;
        __builtin_amdgcn_wave_barrier();
        tb[lane] = term;
        __builtin_amdgcn_wave_barrier();
        real_sum = lds_sum_chain(real_sum, tb, (int)(ns - c0 < 64u ? ns - c0 : 64u));
    }
    return ttx_coscoeff_factor(d, aux) * real_sum;
}

// the sweep's requested slots (DevProb::slot_dev): a grid-stride scan of the request flags, one wave per raised flag; the value goes
// to hval[slot], the flag is cleared (as host_eval does)
__global__ __launch_bounds__(64 * TTX_CC_WAVES) void k_coscoeff_slots(int d, const double *aux, long long nslot, const short *hidx,
                                                                       unsigned char *hreq, double *hval)
{
    extern __shared__ __align__(16) double cc_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double *lds = cc_lds + (size_t)wv * TTX_CC_LDS(d);
    const long long nw = (long long)gridDim.x * TTX_CC_WAVES;
    for (long long s = (long long)blockIdx.x * TTX_CC_WAVES + wv; s < nslot; s += nw) {
        if (!hreq[s]) continue;                                   // wave-uniform
        const double v = coscoeff_wave(d, aux, hidx + (size_t)s * d, lds, lane);
        if (lane == 0) { hval[s] = v; hreq[s] = 0; }
    }
}

// ttx_k_eval: npts elements, ind row-major 1-based
__global__ __launch_bounds__(64 * TTX_CC_WAVES) void k_coscoeff_list(int d, const double *aux, long long npts, const int *ind, double *out)
{
    extern __shared__ __align__(16) double cc_lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double *lds = cc_lds + (size_t)wv * TTX_CC_LDS(d);
    const long long nw = (long long)gridDim.x * TTX_CC_WAVES;
    for (long long p = (long long)blockIdx.x * TTX_CC_WAVES + wv; p < npts; p += nw) {
        const double v = coscoeff_wave(d, aux, ind + (size_t)p * d, lds, lane);
        if (lane == 0) out[p] = v;
    }
}

// ---- host: what is refused before anything reaches the device -------------------------------------------------------------------
#include <cmath>
#include <algorithm>
#include "ttx_err.h"
// TTX_FUN_COSCOEFF: aux = [mu(1:d), Sigma(1:d,1:d), a, b].  Refused before anything reaches the device: a wrong naux, non-finite
// data, a >= b, d > TTX_COSCOEFF_MAXD, and an index box on which |t'mu| or |a sum t| could leave the range of ttx_sin / ttx_cos.
static int coscoeff_check(const char *who, int d, const int32_t *n, const double *aux, int naux)
{
    if (d > TTX_COSCOEFF_MAXD) return fail(TTX_EINVAL, "%s: coscoeff: at most %d dimensions (2^(d-1) sign vectors per element), got %d", who, TTX_COSCOEFF_MAXD, d);
    if (!aux || naux != d + d * d + 2) return fail(TTX_EINVAL, "%s: coscoeff: aux must hold mu(1:d), Sigma(1:d,1:d), a, b: %d values (got %d)", who, d + d * d + 2, naux);
    for (int k = 0; k < naux; k++) if (!std::isfinite(aux[k])) return fail(TTX_EINVAL, "%s: coscoeff: aux(%d) is not finite", who, k + 1);
    const double a = aux[d + d * d], b = aux[d + d * d + 1];
    if (!(a < b)) return fail(TTX_EINVAL, "%s: coscoeff: lower bound %g must be below upper bound %g", who, a, b);
    const double ob = 1.0 / (b - a);
    if (!std::isfinite(ob)) return fail(TTX_EINVAL, "%s: coscoeff: 1/(b-a) is not finite", who);
    // |t_j| <= pi (n_j - 1) / (b - a): bounds of |dot_mu| and |a sum t| (and of every partial sum), with room for rounding
    double bmu = 0.0, bst = 0.0;
    for (int j = 0; j < d; j++) {
        const double tj = TTX_COSCOEFF_PI * (double)std::max(n[j] - 1, 0) * ob;
        bmu += tj * std::fabs(aux[j]); bst += tj;
    }
    bst *= std::fabs(a);
    if (!(bmu * (1 + 1e-9) <= TTX_TRIG_MAX) || !(bst * (1 + 1e-9) <= TTX_TRIG_MAX))
        return fail(TTX_EINVAL, "%s: coscoeff: the arguments of sin/cos can reach %g (|t'mu|) and %g (|a sum t|), beyond the supported %g",
                    who, bmu, bst, (double)TTX_TRIG_MAX);
    return TTX_OK;
}
#endif
