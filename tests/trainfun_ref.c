/* Host twins of the integrands of trains (TTX_FUN_TRAINS, include/ttx.h): a table of up to 8 trains and callbacks with the
 * ttx_host_fun signature that walk the cores in the chain order of dtt_ijk -- x = U_d(:, i_d, 1); for i = d-1 .. 1:
 * x = U_i(:, i_i, :) x with sums from 0.0 over ascending k and a separate multiply and add -- and then apply the combiner in the
 * order include/ttx.h writes it.  Build with -O2 -ffp-contract=off.  The callbacks only read the table: thread-safe. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define TF_MAX 8
#define TF_RMAX 128

typedef struct { int d; int *n, *r; double **core; } tf_train;
static tf_train T[TF_MAX];
static int M = 0;

static void tf_free(tf_train *t)
{
    if (t->core) for (int k = 0; k < t->d; k++) free(t->core[k]);
    free(t->core); free(t->n); free(t->r);
    memset(t, 0, sizeof *t);
}
/* train t = d cores given compact, column-major, concatenated (core k: r[k] x n[k] x r[k+1]); returns 0, or 1 on a bad argument */
int trainfun_set(int t, int d, const int *n, const int *r, const double *cores)
{
    if (t < 0 || t >= TF_MAX || d < 1) return 1;
    for (int k = 0; k <= d; k++) if (r[k] < 1 || r[k] > TF_RMAX) return 1;
    tf_free(&T[t]);
    T[t].d = d;
    T[t].n = malloc(sizeof(int) * d); T[t].r = malloc(sizeof(int) * (d + 1)); T[t].core = calloc(d, sizeof(double *));
    memcpy(T[t].n, n, sizeof(int) * d); memcpy(T[t].r, r, sizeof(int) * (d + 1));
    for (int k = 0; k < d; k++) {
        const size_t sz = (size_t)r[k] * n[k] * r[k + 1];
        T[t].core[k] = malloc(sizeof(double) * sz);
        memcpy(T[t].core[k], cores, sizeof(double) * sz);
        cores += sz;
    }
    return 0;
}
/* the number of operands the callbacks combine */
void trainfun_count(int m) { M = m; }

/* one element of train t (ind 1-based) */
double trainfun_element(int t, const int32_t *ind)
{
    const tf_train *tt = &T[t];
    const int d = tt->d;
    double a[TF_RMAX], b[TF_RMAX], *x = a, *z = b;
    {
        const int q0 = tt->r[d - 1];
        const double *A = tt->core[d - 1] + (size_t)q0 * (ind[d - 1] - 1);
        for (int i = 0; i < q0; i++) x[i] = A[i];
    }
    for (int i = d - 2; i >= 0; i--) {
        const int q0 = tt->r[i], q1 = tt->r[i + 1];
        const size_t SS = (size_t)q0 * tt->n[i];
        const double *A = tt->core[i] + (size_t)q0 * (ind[i] - 1);
        for (int row = 0; row < q0; row++) {
            double s = 0.0;
            for (int k = 0; k < q1; k++) s = s + A[row + SS * k] * x[k];
            z[row] = s;
        }
        double *sw = x; x = z; z = sw;
    }
    return x[0];
}

double trainfun_product(const int32_t *m, const int32_t *ind, const int32_t *n, const double *par)
{
    (void)m; (void)n; (void)par;
    double p = trainfun_element(0, ind);
    for (int t = 1; t < M; t++) p = p * trainfun_element(t, ind);
    return p;
}
double trainfun_ratio(const int32_t *m, const int32_t *ind, const int32_t *n, const double *par)
{
    (void)m; (void)n; (void)par;
    const double a = trainfun_element(0, ind), b = trainfun_element(1, ind);
    return a / b;
}
double trainfun_sqrtabs(const int32_t *m, const int32_t *ind, const int32_t *n, const double *par)
{
    (void)m; (void)n; (void)par;
    return sqrt(fabs(trainfun_element(0, ind)));
}
/* examples/devfun/comb_rational.hip */
double trainfun_comb_rational(const int32_t *m, const int32_t *ind, const int32_t *n, const double *par)
{
    (void)m; (void)n;
    const double v0 = trainfun_element(0, ind), v1 = trainfun_element(1, ind);
    const double q = 1.0 + v1 * v1;
    return v0 / q + par[0] * (double)ind[0];
}
