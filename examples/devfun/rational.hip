// Example device integrand, lane form (one GPU lane per tensor element):
//     f(ind) = (sum_i x_i) / (1 + sum_i x_i^2),   x_i = par(ind_i),   both sums left to right.
// Only + * / : the host C twin (tests/devfun_ref.c), the Fortran function of test_crs_devfun.f90 and this code agree bit for bit.
//     hipcc --genco --offload-arch=gfx950 -O3 -ffp-contract=off -I include examples/devfun/rational.hip -o rational.hsaco
#include "ttx_device_fun.h"

__device__ double rational(int d, ttx_ind ind, const int *n, const double *par)
{
    (void)n;
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < d; i++) {
        const double x = par[ind[i] - 1];
        s1 = s1 + x;
        s2 = s2 + x * x;
    }
    return s1 / (1.0 + s2);
}
TTX_DEVICE_INTEGRAND(rational)

// Degenerate variants for robustness tests: NaN everywhere / NaN on part of the domain (ordinary arithmetic, no fault).
__device__ double rational_nan(int d, ttx_ind ind, const int *n, const double *par)
{
    (void)d; (void)ind; (void)n; (void)par;
    return __builtin_nan("");
}
TTX_DEVICE_INTEGRAND(rational_nan)

__device__ double rational_partnan(int d, ttx_ind ind, const int *n, const double *par)
{
    if (ind[0] == 2 || ind[d - 1] == 1) return __builtin_nan("");
    return rational(d, ind, n, par);
}
TTX_DEVICE_INTEGRAND(rational_partnan)
