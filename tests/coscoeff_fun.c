/* The COS-coefficient integrand (calc_coefficient, the fork's lib/coefficients.f90) in C: ttcross_amd/csrc/ttx_coscoeff.h compiled
 * for the host.  Test infrastructure: handed to the ORACLE (ttxo_problem.user) and, through ttx_set_integrand_host, to the engine,
 * with the reference's callback interface fun(m, ind, n, par); `par` carries the engine's aux = [mu(1:m), Sigma column-major, a, b]. */
#include <stdint.h>
#include "../ttcross_amd/csrc/ttx_coscoeff.h"

double ttx_test_coscoeff(const int32_t *m, const int32_t *ind, const int32_t *n, const double *par)
{
    (void)n;
    return ttx_coscoeff_eval(*m, ind, par, 0);
}

/* npts elements (ind: npts rows of d 1-based indices): values and factor * sum_s exp(-q/2) (a bound of the sum of |terms|) */
void ttx_test_coscoeff_list(int32_t d, const double *aux, int64_t npts, const int32_t *ind, double *val, double *abssum)
{
    for (int64_t p = 0; p < npts; p++) val[p] = ttx_coscoeff_eval(d, ind + p * d, aux, abssum + p);
}

void ttx_test_sin(int64_t n, const double *x, double *out) { for (int64_t i = 0; i < n; i++) out[i] = ttx_sin(x[i]); }
void ttx_test_cos(int64_t n, const double *x, double *out) { for (int64_t i = 0; i < n; i++) out[i] = ttx_cos(x[i]); }

/* the run-time library's sin / cos over the same arrays (the yardstick of the tests) */
#include <math.h>
void ttx_test_libm_sin(int64_t n, const double *x, double *out) { for (int64_t i = 0; i < n; i++) out[i] = sin(x[i]); }
void ttx_test_libm_cos(int64_t n, const double *x, double *out) { for (int64_t i = 0; i < n; i++) out[i] = cos(x[i]); }
