// The integrand of rational.hip in WAVE form (one wave64 per tensor element), as a pattern for integrands with inner parallelism:
// the 64 lanes fetch 64 nodes x_i = par(ind_i) at a time -- the part that waits on memory -- and park them in the wave's LDS;
// the two sums are then formed in the fixed order i = 1 .. d (every lane forms them; lane 0's value counts), so the result is the
// left-to-right sum of rational.hip and of the host twin, bit for bit.
#include "ttx_device_fun.h"

#define RW_LDS (64 * sizeof(double))            // dynamic LDS per wave: one chunk of nodes

__device__ double rational_wave(int d, ttx_ind ind, const int *n, const double *par, int lane)
{
    (void)n;
    double *x = (double *)ttx_wave_lds(RW_LDS);
    double s1 = 0.0, s2 = 0.0;
    for (int c = 0; c < d; c += 64) {
        const int m = (d - c < 64) ? d - c : 64;
        __builtin_amdgcn_wave_barrier();         // the previous chunk has been read
        if (lane < m) x[lane] = par[ind[c + lane] - 1];
        __builtin_amdgcn_wave_barrier();
        for (int i = 0; i < m; i++) {
            const double xi = x[i];
            s1 = s1 + xi;
            s2 = s2 + xi * xi;
        }
    }
    return s1 / (1.0 + s2);
}
TTX_DEVICE_INTEGRAND_WAVE(rational_wave, RW_LDS)
