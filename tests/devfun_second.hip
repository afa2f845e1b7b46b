// Test integrands that are not examples: a second function (two engines with two integrands; replacing an integrand), a file
// that declares more LDS than a workgroup may have, and a file compiled against another ABI version (see test_devfun_cpu.py).
#include "ttx_device_fun.h"

__device__ double second(int d, ttx_ind ind, const int *n, const double *par)
{
    (void)n;
    double s = 1.0;
    for (int i = 0; i < d; i++) s = s + (double)(i + 1) * par[ind[i] - 1];
    return 1.0 / s;
}
TTX_DEVICE_INTEGRAND(second)

__device__ double greedy(int d, ttx_ind ind, const int *n, const double *par, int lane)
{
    (void)d; (void)ind; (void)n; (void)par; (void)lane;
    return 0.0;
}
TTX_DEVICE_INTEGRAND_WAVE(greedy, 20000)      // 4 waves x 20000 bytes > 64 KB: the loader refuses it

// the same function under another name, compiled as if the header spoke a later slot ABI: the loader refuses it
__device__ double future(int d, ttx_ind ind, const int *n, const double *par) { return second(d, ind, n, par); }
#undef TTX_DEVFUN_ABI
#define TTX_DEVFUN_ABI 99
TTX_DEVICE_INTEGRAND(future)
