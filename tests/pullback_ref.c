/* pullback_ref.c -- the host callback of the tests of pulled-back integrands (TTX_FUN_PULLBACK; test_gpu_pullback.py): fun(i) is looked
 * up in a dense table of the integrand over ALL multi-indices of the grid, row-major (the last mode runs fastest), which the test
 * fills from eval_device of the device engine.  A TTX_FUN_HOST engine with this callback walks the same values as the device engine.
 * Built like tests/trainfun_ref.c. */
#include <stdint.h>
#include <stddef.h>

static const double *TAB = 0;
static int64_t COUNT = 0;

void pullback_table(const double *tab, int64_t count) { TAB = tab; COUNT = count; }

/* the reference's user callback fun(m, ind, n, par), everything by reference; outside the table: -3.0 (dtt_ijk's out-of-range value) */
double pullback_lookup(const int32_t *m, const int32_t *ind, const int32_t *n, const double *par)
{
    int64_t at = 0;
    (void)par;
    for (int k = 0; k < *m; k++) {
        if (ind[k] < 1 || ind[k] > n[k]) return -3.0;
        at = at * n[k] + (ind[k] - 1);
    }
    return TAB && at < COUNT ? TAB[at] : -3.0;
}
