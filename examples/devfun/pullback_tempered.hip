// pullback_tempered.hip -- a loaded combiner for a pulled-back integrand (TTX_FUN_PULLBACK, include/ttx.h): the next layer of a
// layered transport towards a tempered target,
//     h(x, logq) = sqrt(exp(beta * logpi(x) - logq)),
// for the small analytic target logpi(x) = -0.5 * sum_k (x_k - mu)^2 / sigma^2 - c * (x_1 * x_2 - rho)^2 (a Gaussian bent along a
// hyperbola in its first two coordinates), with par = (beta, mu, sigma, c, rho).
//
// The engine calls the function with m = d + 2 and v = [x_1 .. x_d, logq, val].  A failed sample (x = NaN) gives 0.0: it carries no
// mass.  The sums run over ascending k from 0.0 with separate multiplies and adds; exp is not an IEEE operation, so a host
// evaluation of the same expression agrees to a few units in the last place, not bit for bit.
//
//     hipcc --genco --offload-arch=gfx950 -O3 -ffp-contract=off -I include examples/devfun/pullback_tempered.hip -o pullback_tempered.hsaco
#include "ttx_device_fun.h"

// the target's log density at the point x[0 .. d-1]
__device__ inline double tempered_logpi(int d, const double *x, const double *par)
{
    const double mu = par[1], sigma = par[2], c = par[3], rho = par[4];
    double s = 0.0;
    for (int k = 0; k < d; k++) { const double z = (x[k] - mu) / sigma; s = s + z * z; }
    const double b = x[0] * x[1] - rho;
    return -0.5 * s - c * (b * b);
}

__device__ double pullback_tempered(int m, const double *v, int d, ttx_ind ind, const int *n, const double *par)
{
    (void)m; (void)ind; (void)n;
    const double e = par[0] * tempered_logpi(d, v, par) - v[d];
    if (!(e == e)) return 0.0;
    return sqrt(exp(e));
}
TTX_DEVICE_COMBINER(pullback_tempered)

// Layer 1 of the same ladder, an ordinary device integrand (TTX_FUN_DEVICE) on the physical grid: sqrt(exp(beta * logpi(x))) at the
// grid point x_k = lo + (hi - lo) (ind_k - 1) / (n_k - 1), with par = (beta, mu, sigma, c, rho, lo, hi); at most 64 modes.
__device__ double tempered_root(int d, ttx_ind ind, const int *n, const double *par)
{
    double x[64];
    const double lo = par[5], hi = par[6];
    for (int k = 0; k < d && k < 64; k++) x[k] = lo + (hi - lo) * (double)(ind[k] - 1) / (double)(n[k] - 1);
    return sqrt(exp(par[0] * tempered_logpi(d < 64 ? d : 64, x, par)));
}
TTX_DEVICE_INTEGRAND(tempered_root)
