// The plan of an enrichment call (en_plan, ttcross_amd/csrc/ttx_op_plan.h) as a stand-alone host program: no GPU, nothing loaded into
// Python.  Built by tests/test_enrich_cpu.py with the host compiler, plain and under the address and undefined-behaviour sanitizers.
// Every rule is restated here independently of the header's code and compared.  For each shape of the tests it prints one JSON line
// (k, the new ranks, ldx, S, the QR shapes) that the test compares with tests/enrich_ref.py; then "enrich plan: ok (N plans)".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ttx_op_plan.h"

static long long nplans = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s fails (d=%d npts=%lld chunk=%zu store=%zu src=%d add=%d)\n", __LINE__, #c, d, (long long)npts, chunk, store, (int)src, add0); exit(1); } } while (0)

static void check(const std::vector<int> &n, const std::vector<int> &r, int add0, BsSrc src, int64_t npts, int mode, size_t chunk, size_t store)
{
    const int d = (int)n.size(), ncu = 256;
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    std::vector<int32_t> add(d - 1, add0);
    const EnPlan p = en_plan(d, n.data(), r.data(), add.data(), ncu, src, npts, mode, chunk, store);
    nplans++;
    int rmax = 0, nm = 1;
    for (int v : r) rmax = std::max(rmax, v);
    for (int v : n) nm = std::max(nm, v);
    if (rmax > 128) { CHECK(p.refusal == BS_RANK); return; }
    if (r[0] != 1 || r[d] != 1) { CHECK(p.refusal == BS_BOUNDARY); return; }
    CHECK(p.refusal == BS_OK);
    // step 1, and the storage of a new engine
    int kmax = 0, bad = 0;
    size_t ysize = 0;
    double ws = 0.0, w = 0.0;
    for (int k = 0; k < d; k++) w += (double)r[k] * n[k] * r[k + 1];
    for (int b = 1; b < d; b++) {
        long long k = add0;
        k = std::min<long long>(k, (long long)r[b - 1] * n[b - 1] - r[b]);
        k = std::min<long long>(k, (long long)n[b] * r[b + 1]);
        k = std::min<long long>(k, 128 - r[b]);
        if (k < 0) k = 0;
        CHECK(p.step[b].k == (int)k && r[b] + k <= 128);
        if (!bad && (long long)(r[b] + k) * nm > 512ll * 256) bad = b;
        kmax = std::max(kmax, (int)k);
        const EnStep &s = p.step[b];
        CHECK(s.rows == r[b - 1] * n[b - 1] && s.cols == r[b] + (int)k && (k == 0 || s.rows >= s.cols));    // a QR that runs is tall
        CHECK(s.acc.goff == ysize && s.acc.size == (size_t)s.rows * (size_t)k);
        ysize += s.acc.size;
        ws += (double)k * ((double)n[b] * r[b + 1] + (double)s.rows);
    }
    CHECK(p.storage_bond == bad);
    if (bad) { CHECK(p.storage_rank == r[bad] + p.step[bad].k); return; }
    CHECK(p.kmax == kmax && p.ysize == ysize && p.b_y >= 8 * ysize && p.b_y >= 8 && p.b_stat == 8u * 2 * 256 * (size_t)(d - 1));
    CHECK(p.flops == (double)npts * (4.0 * w + 2.0 * ws));
    CHECK(p.eff == (mode != TTX_EVAL_AUTO ? mode : p.flops >= TTX_EN_AUTO_FLOPS ? TTX_EVAL_MFMA : TTX_EVAL_EXACT));
    CHECK(p.sketch == (kmax > 0 && npts > 0));
    const CgPlan &g = p.cg;
    // one stride for X, L and z that holds every rank and every k; the store takes d blocks of it
    const int big = std::max(rmax, kmax);
    CHECK(g.ldx >= big && g.ldx % 4 == 0 && g.ldx < big + 4);
    CHECK(g.S == (size_t)d * g.ldx && p.zoff() == (size_t)(d - 1) * g.ldx);
    for (int i = 1; i < d; i++) CHECK(g.soff(i) == (size_t)(i - 1) * g.ldx && g.soff(i) + g.ldx <= p.zoff());
    const size_t fit = store / (8 * g.S) / 256 * 256, cap = std::min(chunk, fit >= 256 ? fit : (size_t)256);
    CHECK(g.cap == cap);
    if (!p.sketch) { CHECK(g.chunk == 0 && g.b_gst == 0 && g.b_xa == 0 && g.b_x == 0 && g.b_btab == 0 && p.b_part == 0); return; }
    CHECK(g.chunk >= 1 && g.chunk <= cap && g.chunk <= (size_t)npts);
    if (src != BS_TAB_HOST) CHECK(g.chunk == std::min(cap, (size_t)npts));
    else CHECK(g.chunk * g.sumn <= ((size_t)1 << 25) || g.chunk == 1);
    CHECK(g.b_gst == 8 * g.S * g.chunk && g.b_xa == 8 * g.chunk * (size_t)g.ldx && g.b_xb == g.b_xa);
    CHECK(g.b_btab == (tab ? 0 : 8 * g.chunk * g.nmax));
    CHECK(g.b_x == (dev ? 0 : 8 * g.chunk * ((tab ? g.sumn : (size_t)d) + 1)));
    CHECK(g.lds_back == 4u * 8 * (size_t)g.ldx && g.lds_fwd == 2 * g.lds_back && g.lds_fwd <= 64 * 1024);
    const int c = (int)g.chunk;
    for (int b = 1; b < d; b++) {
        const EnStep &s = p.step[b];
        if (!s.k) continue;
        // z: QT tiles of 16 cover k, PT point tiles per wave, four waves
        CHECK((s.qt == 1 || s.qt == 2 || s.qt == 4 || s.qt == 8) && 16 * s.qt >= s.k && (s.qt == 1 || 8 * s.qt < s.k));
        CHECK(s.tp == 64 * en_pt(s.qt) && (long long)p.g_z(b, c) * s.tp >= c && (long long)(p.g_z(b, c) - 1) * s.tp < c);
        // Y: the accumulation launch of the core gradient with r1 = k
        CHECK(s.acc.tier >= 1 && s.acc.tier <= 8 && 16 * s.acc.tier >= r[b - 1] && 16 * (s.acc.tier - 1) < r[b - 1]);
        const size_t wcol = 64 * (size_t)cg_ct(s.acc.tier), ncol = (size_t)n[b - 1] * s.k;
        CHECK((size_t)s.acc.ngrp * wcol >= ncol && ((size_t)s.acc.ngrp - 1) * wcol < ncol);
        CHECK(s.acc.seg >= 256 && s.acc.seg % 16 == 0);
        const int ns = p.nsplit(b, c);
        CHECK(ns >= 1 && ns <= 65535 && (long long)ns * s.acc.seg >= c && (long long)(ns - 1) * s.acc.seg < c);
        CHECK(s.acc.lds == 8u * 16 * ((size_t)cg_lda(s.acc.tier) + cg_ldw(s.acc.tier) + cg_ldq(s.k)) && s.acc.lds <= 64 * 1024);
        if (p.eff == TTX_EVAL_MFMA) CHECK(p.b_part >= 8 * s.acc.size * (size_t)ns);
        CHECK(s.k <= g.ldx);                                                    // a row of z fits its stride
    }
    if (p.eff != TTX_EVAL_MFMA) CHECK(p.b_part == 0);
    // the summation order depends on the points per chunk and not on the device
    const EnPlan q = en_plan(d, n.data(), r.data(), add.data(), 64, src, (size_t)npts >= g.cap ? npts + 12345 : npts, mode, chunk, store);
    CHECK(q.cg.chunk == g.chunk);
    for (int b = 1; b < d; b++) CHECK(q.step[b].acc.seg == p.step[b].acc.seg && q.step[b].acc.ngrp == p.step[b].acc.ngrp);
}

static void print_shape(const std::vector<int> &n, const std::vector<int> &r, int add0)
{
    const int d = (int)n.size();
    std::vector<int32_t> add(d - 1, add0);
    const EnPlan p = en_plan(d, n.data(), r.data(), add.data(), 256, BS_TAB_HOST, 300, TTX_EVAL_EXACT, (size_t)1 << 18, TTX_BG_STORE_DEFAULT);
    printf("{\"k\": [");
    for (int b = 1; b < d; b++) printf("%s%d", b > 1 ? ", " : "", p.step[b].k);
    printf("], \"rnew\": [1");
    for (int b = 1; b < d; b++) printf(", %d", r[b] + p.step[b].k);
    printf(", 1], \"ldx\": %d, \"S\": %zu, \"qr\": [", p.cg.ldx, p.cg.S);
    bool first = true;
    for (int b = 1; b < d; b++) if (p.step[b].k) { printf("%s[%d, %d]", first ? "" : ", ", p.step[b].rows, p.step[b].cols); first = false; }
    printf("]}\n");
}

int main()
{
    const BsSrc srcs[] = {BS_X_HOST, BS_X_DEV, BS_TAB_HOST, BS_TAB_DEV};
    const int modes[] = {TTX_EVAL_EXACT, TTX_EVAL_MFMA, TTX_EVAL_AUTO};
    const int64_t counts[] = {0, 1, 5, 17, 65, 257, 300, 100000, 3000000};
    const size_t chunks[] = {1, 64, 256, (size_t)1 << 17, (size_t)1 << 18};
    const size_t stores[] = {1, 8 * 256, 100000, (size_t)1 << 32, (size_t)1 << 40};
    const int adds[] = {0, 1, 4, 16, 20, 200};
    std::vector<std::pair<std::vector<int>, std::vector<int>>> shapes = {
        {{7, 2, 51, 1, 9}, {1, 3, 17, 5, 4, 1}}, {{4, 5, 3, 2}, {1, 16, 33, 65, 1}}, {{2, 2, 2}, {1, 128, 128, 1}}, {{3, 2, 3}, {1, 96, 113, 1}},
        {{3, 4, 2, 5}, {1, 2, 70, 3, 1}}, {{5, 7}, {1, 3, 1}}, {{4, 6, 5, 6, 4}, {1, 4, 15, 17, 4, 1}},                // the shapes of the tests
    };
    for (const auto &s : shapes) print_shape(s.first, s.second, 20);
    shapes.push_back({{5, 6, 4}, {1, 2, 1, 1}});                                                        // the recovery run
    shapes.push_back({{3, 5000, 3}, {1, 7, 5, 1}});                                                     // a long mode
    shapes.push_back({{70, 2000}, {1, 60, 1}});                                                          // 60 x 2000 is stored, 66 x 2000 is not: refused from add = 6 on
    shapes.push_back({{2, 2, 2}, {1, 129, 2, 1}});                                                      // rank 129: refused
    shapes.push_back({{2, 2}, {2, 3, 1}});                                                              // a boundary rank: refused
    shapes.push_back({std::vector<int>(64, 65), std::vector<int>(65, 20)});                             // a D_64-like shape
    shapes.back().second.front() = shapes.back().second.back() = 1;
    for (const auto &s : shapes)
        for (int add0 : adds) for (BsSrc src : srcs) for (int mode : modes) for (int64_t npts : counts) for (size_t chunk : chunks) for (size_t store : stores)
            check(s.first, s.second, add0, src, npts, mode, chunk, store);
    {   // the refusal names the bond and the rank it would reach
        const int n3[] = {70, 2000}, r3[] = {1, 60, 1};
        const int32_t a5[] = {5}, a6[] = {6};
        if (en_plan(2, n3, r3, a5, 256, BS_TAB_DEV, 100, TTX_EVAL_EXACT, 256, 1 << 20).storage_bond != 0) { printf("65 x 2000 is refused\n"); return 1; }
        const EnPlan p = en_plan(2, n3, r3, a6, 256, BS_TAB_DEV, 100, TTX_EVAL_EXACT, 256, 1 << 20);
        if (p.storage_bond != 1 || p.storage_rank != 66) { printf("66 x 2000: bond %d rank %d\n", p.storage_bond, p.storage_rank); return 1; }
    }
    printf("enrich plan: ok (%lld plans)\n", nplans);
    return 0;
}
