// comb_rational.hip -- a loaded combiner for an integrand of trains (TTX_FUN_TRAINS, TTX_TOP_DEVICE):
//     g(v, ind) = v[0] / (1 + v[1] v[1]) + par[0] ind(1)
// v[0], v[1] are the values of the two operand trains at the multi-index.  Only + * /: the host twin computes the same bits.
//     hipcc --genco --offload-arch=gfx950 -O3 -ffp-contract=off -I include examples/devfun/comb_rational.hip -o comb_rational.hsaco
#include "ttx_device_fun.h"

__device__ double comb_rational(int m, const double *v, int d, ttx_ind ind, const int *n, const double *par)
{
    const double q = 1.0 + v[1] * v[1];
    return v[0] / q + par[0] * (double)ind[0];
}
TTX_DEVICE_COMBINER(comb_rational)
