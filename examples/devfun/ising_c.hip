// The Ising integral C_m of the reference's driver (dfunc_ising_discr, test_crs_ising.f90:176-218, branch id = 1) as a loadable
// device integrand, lane form.  par = [nodes(1:n1), weights(1:n1), id] as the driver builds it; only + * / are used, so it agrees
// bit for bit with the engine's built-in TTX_FUN_ISING and with the host function.
#include "ttx_device_fun.h"

__device__ double ising_c(int d, ttx_ind ind, const int *n, const double *par)
{
    const double *nodes = par - 1, *weights = par + n[0] - 1;      // 1-based, as par(nodes + ind(i)) / par(weights + ind(i))
    double v = 1.0, w = 1.0, vk = 1.0, wk = 1.0;
    for (int i = 1; i <= d; i++) {
        vk = vk * nodes[ind(d - i + 1)];
        wk = wk * nodes[ind(i)];
        v = v + vk;
        w = w + wk;
    }
    double f = 2 * (1.0 / (v * w));
    for (int i = 1; i <= d; i++) f = f * weights[ind(i)];
    return f;
}
TTX_DEVICE_INTEGRAND(ising_c)
