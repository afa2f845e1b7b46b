// pullback_plan_main.cpp -- the host-only part of TTX_FUN_PULLBACK (ttcross_amd/csrc/ttx_pullback_plan.h) on the CPU: the launch
// shape at its edges and every argument refusal that needs no GPU.  Built and run stand-alone, also with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <string>
#include <vector>

#include "ttx_pullback_plan.h"

static int checks = 0, failures = 0;
#define CHECK(c) do { checks++; if (!(c)) { failures++; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

// m well-formed layers of d modes, a well-formed reference grid; the tests spoil one thing at a time
struct Fixture {
    int d, m;
    std::vector<int> n, r, hn;
    std::vector<std::vector<std::vector<double>>> nodes;        // [m][d][n_k]
    std::vector<std::vector<const double *>> rows;              // [m][d]
    std::vector<std::vector<double>> ref;
    std::vector<const double *> refp;
    std::vector<PbLayer> L;
    int handles[TTX_PULLBACK_MAX + 2];
    Fixture(int d_, int m_) : d(d_), m(m_), n(d_), r(d_ + 1, 3), hn(d_), nodes(m_), rows(m_), ref(d_), refp(d_), L(m_)
    {
        r[0] = r[d] = 1;
        for (int k = 0; k < d; k++) { n[k] = 2 + k; hn[k] = 3 + k; }
        for (int t = 0; t < m; t++) {
            nodes[t].resize(d); rows[t].resize(d);
            for (int k = 0; k < d; k++) {
                nodes[t][k].resize(n[k]);
                for (int i = 0; i < n[k]; i++) nodes[t][k][i] = t == 0 ? -2.0 + 4.0 * i / (n[k] - 1) : (i == n[k] - 1 ? 1.0 : (double)i / (n[k] - 1));
            }
            L[t].x = &handles[t]; L[t].has_train = true; L[t].one_process = true; L[t].device = 0; L[t].d = d; L[t].n = n.data(); L[t].r = r.data(); L[t].gamma = 0.25 * t;
        }
        for (int k = 0; k < d; k++) { ref[k].resize(hn[k]); for (int i = 0; i < hn[k]; i++) ref[k][i] = (double)i / (hn[k] - 1); }
        fix();
    }
    void fix()
    {
        for (int t = 0; t < m; t++) { for (int k = 0; k < d; k++) rows[t][k] = nodes[t][k].data(); L[t].nodes = rows[t].data(); }
        for (int k = 0; k < d; k++) refp[k] = ref[k].data();
    }
    int run(std::string *msg, int mm = -1, const PbLayer *LL = nullptr, bool noL = false) const
    {
        return pb_check("set", mm < 0 ? m : mm, noL ? nullptr : (LL ? LL : L.data()), &handles[TTX_PULLBACK_MAX + 1], 0, d, hn.data(), refp.data(), msg);
    }
};
static bool has(const std::string &s, const char *w) { return s.find(w) != std::string::npos; }

static void lds_and_waves()
{
    // (ldx, nmax, d) = (4, 2, 1): 2*4 + 2*2 + 1 + 1 = 14 doubles per wave, four waves
    CHECK(pb_lds_doubles(4, 2, 1) == 14);
    PbPlan p = pb_plan(4, 2, 1, 256, 0);
    CHECK(p.per_wave == 14 && p.waves == 4 && p.lds == 14 * 8 * 4 && !p.raise && !p.refused && p.grid_cap == 2048);
    CHECK(p.grid(1) == 1 && p.grid(4) == 1 && p.grid(5) == 2 && p.grid(1 << 20) == 2048);
    // (128, 1025, 255): 256 + 2050 + 255 + 128 = 2689 doubles = 21512 bytes per wave; four waves are 86048 bytes: above 64 KB, within the budget
    CHECK(pb_lds_doubles(128, 1025, 255) == 2689);
    p = pb_plan(128, 1025, 255, 256, 0);
    CHECK(p.waves == 4 && p.lds == 86048 && p.raise && !p.refused);
    // the waves halve as the sheets grow, down to one; then the first size that no longer fits
    const size_t budget = TTX_LDS_WORK / sizeof(double);
    int last_waves = 4, first_refused = -1;
    for (int nmax = 2; nmax < 20000; nmax++) {
        p = pb_plan(128, nmax, 255, 256, 0);
        CHECK(p.waves <= last_waves && (p.waves == 4 || p.waves == 2 || p.waves == 1));
        CHECK(p.refused == (p.per_wave > budget));
        if (!p.refused) CHECK(p.lds <= TTX_LDS_WORK && p.lds == 8 * p.per_wave * p.waves && (p.waves == 4 || 8 * p.per_wave * p.waves * 2 > TTX_LDS_WORK));
        if (p.refused && first_refused < 0) first_refused = nmax;
        last_waves = p.waves;
    }
    // 2 nmax + 256 + 255 + 128 > 19200  <=>  nmax > 9280.5
    CHECK(first_refused == 9281);
    std::string msg;
    CHECK(pb_check_lds("set", pb_plan(128, 9280, 255, 256, 0), 128, 9280, 255, &msg) == TTX_OK);
    CHECK(pb_check_lds("set", pb_plan(128, 9281, 255, 256, 0), 128, 9281, 255, &msg) == TTX_EINVAL && has(msg, "LDS") && has(msg, "9281"));
    // TTX_PB_GRID caps the grid; nonsense leaves it alone
    CHECK(pb_plan(4, 2, 1, 256, pb_env_grid("1")).grid(1000) == 1);
    CHECK(pb_plan(4, 2, 1, 256, pb_env_grid("3")).grid(1000) == 3);
    CHECK(pb_plan(4, 2, 1, 256, pb_env_grid("99999")).grid_cap == 2048);
    CHECK(pb_plan(4, 2, 1, 256, pb_env_grid("")).grid_cap == 2048 && pb_plan(4, 2, 1, 256, pb_env_grid(nullptr)).grid_cap == 2048);
    CHECK(pb_plan(4, 2, 1, 256, pb_env_grid("-5")).grid_cap == 2048 && pb_plan(4, 2, 1, 256, pb_env_grid("x")).grid_cap == 2048);
}

static void node_and_ref_rules()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const double a[] = {-1.0, 0.5, 3.0}, u[] = {0.0, 0.25, 1.0};
    CHECK(pb_bad_nodes(a, 3, false).empty() && !pb_bad_nodes(a, 3, true).empty());
    CHECK(pb_bad_nodes(u, 3, true).empty() && pb_bad_nodes(u, 3, false).empty());
    CHECK(pb_bad_nodes(nullptr, 3, false) == "is missing");
    const double e0[] = {1e-300, 0.5, 1.0}, e1[] = {0.0, 0.5, std::nextafter(1.0, 0.0)}, e2[] = {-0.0, 1.0};
    CHECK(has(pb_bad_nodes(e0, 3, true), "exactly 0 and 1") && has(pb_bad_nodes(e1, 3, true), "exactly 0 and 1"));
    CHECK(pb_bad_nodes(e2, 2, true).empty());                       // -0.0 == 0.0
    const double b0[] = {0.0, 0.5, 0.5, 1.0}, b1[] = {0.0, 0.7, 0.5, 1.0}, b2[] = {0.0, nan, 1.0}, b3[] = {0.0, 0.5, inf}, b4[] = {-inf, 0.5, 1.0};
    CHECK(has(pb_bad_nodes(b0, 4, true), "ascending") && has(pb_bad_nodes(b1, 4, false), "ascending"));
    CHECK(has(pb_bad_nodes(b2, 3, false), "finite") && has(pb_bad_nodes(b3, 3, false), "finite") && has(pb_bad_nodes(b4, 3, false), "finite"));
    CHECK(pb_bad_ref(u, 3).empty() && pb_bad_ref(nullptr, 3) == "is missing");
    const double r0[] = {0.0, 1.0, 0.5, 0.5}, r1[] = {0.0, -1e-300}, r2[] = {std::nextafter(1.0, 2.0)}, r3[] = {0.5, nan}, r4[] = {-0.0, 1.0};
    CHECK(pb_bad_ref(r0, 4).empty());                               // any order, repeats allowed: only the range is a rule
    CHECK(has(pb_bad_ref(r1, 2), "entry 2") && has(pb_bad_ref(r2, 1), "entry 1") && has(pb_bad_ref(r3, 2), "entry 2") && pb_bad_ref(r4, 2).empty());
}

static void refusals()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    std::string msg;
    for (int m = 1; m <= TTX_PULLBACK_MAX; m++) { Fixture f(3, m); CHECK(f.run(&msg) == TTX_OK); }
    { Fixture f(3, 2); CHECK(f.run(&msg, 0) == TTX_EINVAL && has(msg, "set: 0 layers")); CHECK(f.run(&msg, 9) == TTX_EINVAL && has(msg, "9 layers")); }
    { Fixture f(3, 2); CHECK(f.run(&msg, -1, nullptr, true) == TTX_EINVAL && has(msg, "layer list missing")); }
    { Fixture f(3, 3); f.L[1].x = nullptr; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 2 is null")); }
    { Fixture f(3, 3); f.L[2].x = &f.handles[TTX_PULLBACK_MAX + 1]; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 3 is the engine itself")); }
    { Fixture f(3, 2); f.L[0].has_train = false; f.L[0].n = nullptr; f.L[0].r = nullptr; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 1 holds no tensor train")); }
    { Fixture f(3, 2); f.L[1].one_process = false; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 2 is spread over processes")); }
    { Fixture f(3, 2); f.L[1].device = 1; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 2 lives on device 1")); }
    { Fixture f(3, 2); f.L[0].d = 4; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 1 has 4 modes, the engine 3")); }
    { Fixture f(3, 2); std::vector<int> r = f.r; r[1] = 129; f.L[1].r = r.data(); CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 2: rank 129 at bond 1")); }
    { Fixture f(3, 2); std::vector<int> r = f.r; r[2] = 128; f.L[1].r = r.data(); CHECK(f.run(&msg) == TTX_OK); }
    { Fixture f(3, 2); std::vector<int> r = f.r; r[3] = 2; f.L[0].r = r.data(); CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "boundary")); }
    { Fixture f(3, 2); std::vector<int> n = f.n; n[1] = 1; f.L[1].n = n.data(); CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 2: mode 2 has one index")); }
    { Fixture f(3, 2); f.L[1].nodes = nullptr; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 2: node rows missing")); }
    { Fixture f(3, 2); f.rows[1][2] = nullptr; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 2, mode 3: the node row is missing")); }
    { Fixture f(3, 2); f.nodes[0][1][1] = nan; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 1, mode 2") && has(msg, "finite")); }
    { Fixture f(3, 2); f.nodes[0][2][3] = inf; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 1, mode 3") && has(msg, "finite")); }
    { Fixture f(3, 2); f.nodes[1][2][1] = f.nodes[1][2][2]; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 2, mode 3") && has(msg, "ascending")); }
    // the node-end rule: layer 1 may span any box, layers 2 and up run from exactly 0.0 to exactly 1.0
    { Fixture f(3, 3); f.nodes[0][0][0] = -7.0; CHECK(f.run(&msg) == TTX_OK); }
    { Fixture f(3, 3); f.nodes[1][0][0] = 1e-17; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 2, mode 1") && has(msg, "exactly 0 and 1")); }
    { Fixture f(3, 3); f.nodes[2][1][f.n[1] - 1] = std::nextafter(1.0, 2.0); CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 3, mode 2") && has(msg, "exactly 0 and 1")); }
    // gamma
    { Fixture f(3, 2); f.L[1].gamma = -1e-300; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 2: gamma")); }
    { Fixture f(3, 2); f.L[0].gamma = nan; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 1: gamma")); }
    { Fixture f(3, 2); f.L[0].gamma = inf; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layer 1: gamma")); }
    { Fixture f(3, 2); f.L[0].gamma = 0.0; f.L[1].gamma = 1e300; CHECK(f.run(&msg) == TTX_OK); }
    // one engine as two layers: the same nodes (by value) and gamma, or refused
    { Fixture f(3, 3); f.nodes[0] = f.nodes[1]; f.fix(); f.L[0].x = f.L[1].x; f.L[0].gamma = f.L[1].gamma; CHECK(f.run(&msg) == TTX_OK); }
    { Fixture f(3, 3); f.nodes[0] = f.nodes[1]; f.fix(); f.L[0].x = f.L[1].x; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layers 1 and 2 are one engine")); }
    { Fixture f(3, 3); f.L[2].x = f.L[1].x; f.L[2].gamma = f.L[1].gamma; f.nodes[2][1][1] *= 0.5; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "layers 2 and 3 are one engine")); }
    // the reference grid
    { Fixture f(3, 1); f.refp[1] = nullptr; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "mode 2: the reference row is missing")); }
    { Fixture f(3, 1); f.ref[2][4] = std::nextafter(1.0, 2.0); CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "mode 3: the reference row") && has(msg, "entry 5")); }
    { Fixture f(3, 1); f.ref[0][0] = -1e-300; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "mode 1: the reference row") && has(msg, "entry 1")); }
    { Fixture f(3, 1); f.ref[0][1] = nan; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "mode 1")); }
    { Fixture f(3, 1); std::string m2; CHECK(pb_check("set", 1, f.L.data(), &f.handles[9], 0, 3, f.hn.data(), nullptr, &m2) == TTX_EINVAL && has(m2, "reference rows missing")); }
    // the order: a layer's fault is reported before the reference grid's
    { Fixture f(3, 2); f.ref[0][0] = 2.0; f.L[1].gamma = -1.0; CHECK(f.run(&msg) == TTX_EINVAL && has(msg, "gamma")); }
}

int main()
{
    lds_and_waves();
    node_and_ref_rules();
    refusals();
    if (failures) { printf("pullback plan: %d of %d checks FAILED\n", failures, checks); return 1; }
    printf("pullback plan: ok (%d checks)\n", checks);
    return 0;
}
