/* Host C twins of the example device integrands (examples/devfun/), with the reference's callback interface
 * fun(m, ind, n, par) (lib/dmrgg.f90:18).  Test infrastructure: handed to the ORACLE (ttxo_problem.user) and, through
 * ttx_set_integrand_host, to the engine; the device integrands must return the same bits. */
#include <math.h>
#include <stdint.h>

/* rational.hip / rational_wave.hip: f = (sum x_i) / (1 + sum x_i^2), x_i = par[ind_i - 1], sums left to right */
double ttx_devfun_rational(const int32_t *m, const int32_t *ind, const int32_t *n, const double *par)
{
    double s1 = 0.0, s2 = 0.0;
    (void)n;
    for (int i = 0; i < *m; i++) { const double x = par[ind[i] - 1]; s1 = s1 + x; s2 = s2 + x * x; }
    return s1 / (1.0 + s2);
}

/* a second function (two engines with two integrands): f = 1 / (1 + sum i * x_i) */
double ttx_devfun_second(const int32_t *m, const int32_t *ind, const int32_t *n, const double *par)
{
    double s = 1.0;
    (void)n;
    for (int i = 0; i < *m; i++) s = s + (double)(i + 1) * par[ind[i] - 1];
    return 1.0 / s;
}

double ttx_devfun_rational_nan(const int32_t *m, const int32_t *ind, const int32_t *n, const double *par)
{
    (void)m; (void)ind; (void)n; (void)par;
    return NAN;
}
double ttx_devfun_rational_partnan(const int32_t *m, const int32_t *ind, const int32_t *n, const double *par)
{
    if (ind[0] == 2 || ind[*m - 1] == 1) return NAN;
    return ttx_devfun_rational(m, ind, n, par);
}
