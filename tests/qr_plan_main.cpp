// Stand-alone check of ttcross_amd/csrc/ttx_qr_plan.h (host code only): prints the whole QR plan of a list of shapes, one line
// each (tests/test_qr_plan_cpu.py holds the expected lines), then checks every plan of a grid of shapes against the bounds of
// the work buffers and of the device's LDS.  Built plain and with -fsanitize=address,undefined by that test.
#include "ttx_qr_plan.h"

#include <cstdio>
#include <string>

static std::string kernel_name(const QrLaunch &L)
{
    switch (L.kernel) {
    case QRK_OWN: return "own<" + std::to_string(L.mr) + "," + std::to_string(L.nc) + ">";
    case QRK_PANEL: return "panel";
    case QRK_LDS: return "qr<true>";
    case QRK_STREAM: return "qr<false>";
    default: return "none";
    }
}
static void print_plan(int m, int n, bool wa, const QrEnv &e)
{
    const QrPlan p = qr_plan(m, n, wa, e);
    printf("%dx%d wa=%d own=%d tsqr=%d thr=%d top=%d panel=%d -> %s", m, n, (int)wa, (int)!e.own_off, (int)!e.tsqr_off, e.threads, e.top_threads, e.panel,
           qr_route_name(p.route));
    for (size_t l = 0; l < p.lv.size(); l++) {
        const QrLevel &L = p.lv[l];
        printf(" | L%zu %s rows=%d P=%d rbs=%d thr=%d lds=%zu M=%s+%zu Q=%s+%zu R=Wc+%zu", l, kernel_name(L).c_str(), L.rows, L.P, L.rbs, L.threads, L.lds,
               l ? "Wc" : "A", L.m_off, l ? "Wd" : "Wb", L.q_off, L.r_off);
    }
    if (p.route != QR_REFUSED)
        printf(" | top %s rows=%d thr=%d lds=%zu M=%s+%zu", kernel_name(p.top).c_str(), p.top.rows, p.top.threads, p.top.lds, p.lv.empty() ? "A" : "Wc", p.top_off);
    printf("\n");
}

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 20) printf("FAILED %d x %d (wa %d, variant %d): %s\n", m, n, (int)wa, v, #c); } } while (0)
static void check_plan(int m, int n, bool wa, const QrEnv &e, int v)
{
    const QrPlan p = qr_plan(m, n, wa, e);
    const size_t mn = (size_t)m * n;
    CHECK(p.route >= QR_REFUSED && p.route <= QR_STREAM);
    CHECK((p.route == QR_TSQR_REG || p.route == QR_TSQR_LDS) == !p.lv.empty());
    CHECK((p.route == QR_REFUSED) == (p.top.kernel == QRK_NONE));
    CHECK(p.lv.empty() || wa);
    int rows = m;
    size_t wc = 0, wd = 0;                      // doubles of Wc and Wd the levels before this one have taken
    for (size_t l = 0; l < p.lv.size(); l++) {
        const QrLevel &L = p.lv[l];
        CHECK(L.kernel == QRK_OWN || L.kernel == QRK_PANEL);
        CHECK(L.rows == rows && L.P >= 1 && L.rbs >= n);
        CHECK((long)L.P * L.rbs >= L.rows);
        CHECK(L.rows - (L.P - 1) * L.rbs >= n);                              // every panel, the last one too, has at least n rows
        CHECK(L.lds <= TTX_LDS_DEVICE && L.threads >= 64 && L.threads <= 1024 && L.threads % 64 == 0);
        if (L.kernel == QRK_OWN) CHECK(L.rbs <= 64 * L.mr && L.nc * (L.threads / 64) >= n);
        const size_t tri = (size_t)L.P * n * n, q = (size_t)L.rows * n;     // this level's triangles, its Q panels
        CHECK(L.r_off == wc && L.r_off + tri <= mn);                         // Wb, Wc, Wd hold the m n doubles of A, not more
        if (l == 0) CHECK(L.m_off == 0 && L.q_off == 0 && q == mn);          // A itself, Q panels from the start of Wb
        else { CHECK(L.m_off + q == L.r_off); CHECK(L.q_off == wd && L.q_off + q <= mn); wd += q; }
        wc += tri;
        rows = L.P * n;
    }
    if (p.route == QR_REFUSED) { CHECK(sizeof(double) * ((size_t)m + n + 4) > TTX_LDS_WORK); return; }
    CHECK(p.top.rows == rows && p.top.P == 1 && p.top.rbs == rows && p.top.lds <= TTX_LDS_DEVICE);
    CHECK(p.top.threads >= 64 && p.top.threads <= 1024 && p.top.threads % 64 == 0);
    if (p.top.kernel == QRK_OWN) CHECK(rows <= 64 * p.top.mr && p.top.nc * (p.top.threads / 64) >= n);
    if (!p.lv.empty()) CHECK(p.top_off + (size_t)rows * n == wc);            // the top works in place on the last level's triangles
    else CHECK(p.top_off == 0);
}

int main()
{
    const QrEnv dflt;
    QrEnv no_own, no_tsqr, neither, short_panels;
    no_own.own_off = true; no_tsqr.tsqr_off = true; neither.own_off = neither.tsqr_off = true;
    short_panels.panel = 64; short_panels.threads = 512;
    // the shapes of the GPU tests: anchors, then test_shape_sweep's ort unfolding of core 2 and transposed svd unfolding of core 3
    print_plan(1632, 32, true, dflt);
    print_plan(276, 64, true, dflt);
    print_plan(10, 2, true, dflt);
    print_plan(408, 97, true, dflt);
    const int sweep[] = {1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 96, 97, 127, 128};
    for (int rk : sweep) {
        const int r1 = rk < 12 ? rk : 12, n2 = (4 * rk + r1 - 1) / r1 + 1;
        print_plan(r1 * n2, rk, true, dflt);
        print_plan(4 * rk + 1, rk, true, dflt);
    }
    print_plan(1632, 32, true, no_own);
    print_plan(1632, 32, true, short_panels);
    print_plan(1632, 32, true, no_tsqr);
    print_plan(3000, 40, true, neither);
    print_plan(1632, 32, false, dflt);
    print_plan(20000, 8, true, no_tsqr);        // refused: too many rows for one workgroup
    print_plan(1632, 96, true, dflt);           // levels that would run past the work buffers: one workgroup instead
    print_plan(4896, 96, true, dflt);           // ... and levels of the same width that fit exactly

    // every (m, n) of the grid under every variant of the switches
    QrEnv few_waves; few_waves.threads = 64; few_waves.top_threads = 256;
    QrEnv wide_panels; wide_panels.panel = 512;
    const QrEnv variants[] = {dflt, no_own, no_tsqr, neither, short_panels, few_waves, wide_panels};
    long pairs = 0;
    for (int n = 1; n <= 128; n++) {
        const int ms[] = {n, 2 * n, 4 * n - 1, 4 * n, 4 * n + 1, 255, 256, 257, 511, 512, 513, 1632, 6528, 20000};
        for (int m : ms) {
            pairs++;
            for (int wa = 0; wa < 2; wa++)
                for (int v = 0; v < (int)(sizeof variants / sizeof variants[0]); v++) check_plan(m, n, wa != 0, variants[v], v);
        }
    }
    if (bad) printf("qr plan: %d checks FAILED\n", bad);
    else printf("qr plan: ok (%ld shapes)\n", pairs);
    return bad != 0;
}
