// The plan of a gradient call (bg_plan, ttcross_amd/csrc/ttx_op_plan.h) as a stand-alone host program: no GPU, nothing loaded
// into Python.  Built by tests/test_basis_grad_cpu.py with the host compiler, plain and under the address and undefined-behaviour
// sanitizers.  Every rule is restated here independently of the header's code and compared; prints "basis grad plan: ok (N plans)".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ttx_op_plan.h"

static long long nplans = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s fails (d=%d npts=%lld chunk=%zu store=%zu)\n", __LINE__, #c, d, (long long)npts, chunk, store); exit(1); } } while (0)

static void check(const std::vector<int> &n, const std::vector<int> &r, BsSrc src, int64_t npts, int mode, size_t chunk, size_t store)
{
    const int d = (int)n.size(), ncu = 256;
    const BgPlan p = bg_plan(d, n.data(), r.data(), ncu, src, npts, mode, chunk, store);
    nplans++;
    int rmax = 0;
    for (int v : r) rmax = std::max(rmax, v);
    if (rmax > 128) { CHECK(p.refusal == BS_RANK); return; }
    if (r[0] != 1 || r[d] != 1) { CHECK(p.refusal == BS_BOUNDARY); return; }
    CHECK(p.refusal == BS_OK);
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    size_t S = 0, sumn = 0, nmax = 1;
    double w = 0.0;
    for (int k = 0; k < d; k++) {
        CHECK(p.soff[k] == S && p.off[k] == sumn);
        S += (size_t)r[k]; sumn += (size_t)n[k]; nmax = std::max(nmax, (size_t)n[k]);
        w += (double)r[k] * n[k] * r[k + 1];
        // tiers and LDS per step: 16 tier covers both ranks; the backward image is (r0 up to 16) x 16 at leading dimension ev_lda(r0),
        // the forward image (r1 up to 16) rows of TTX_BG_LDT, both double-buffered
        const BgStep &s = p.step[k];
        const int big = std::max(r[k], r[k + 1]);
        CHECK(s.tier >= 1 && s.tier <= 8 && 16 * s.tier >= big && 16 * (s.tier - 1) < big);
        CHECK(s.tp_back == 64 * bg_ct(s.tier) && s.tp_fwd == 64 * bs_ct(s.tier));
        CHECK(s.lds_back == 8u * 2 * (size_t)ev_lda(r[k]) * 16 && ev_lda(r[k]) >= r[k]);
        CHECK(s.lds_fwd == 8u * 2 * (size_t)TTX_BG_LDT * (size_t)((r[k + 1] + 15) / 16 * 16) && TTX_BG_LDT >= 16);
        CHECK(s.lds_back <= 64 * 1024 && s.lds_fwd <= 64 * 1024);               // no launch has to raise the LDS ceiling
    }
    CHECK(p.S == S && p.sumn == sumn && p.nmax == nmax);
    CHECK(p.flops == 6.0 * (double)npts * w);
    CHECK(p.eff == (mode != TTX_EVAL_AUTO ? mode : p.flops >= TTX_BG_AUTO_FLOPS ? TTX_EVAL_MFMA : TTX_EVAL_EXACT));
    CHECK(p.ldx >= rmax && p.ldx % 4 == 0);
    // the chunk: under the caller's chunk, under npts, and under the store budget -- except that a budget below one tile gives 256
    CHECK(p.chunk <= chunk && p.chunk <= (size_t)npts);
    if (npts > 0) CHECK(p.chunk >= 1);
    const size_t fit = store / (8 * S) / 256 * 256;                             // the largest multiple of 256 under the budget
    if (fit >= 256) {
        CHECK(8 * S * p.chunk <= store);
        if (src != BS_TAB_HOST && (size_t)npts >= fit + 256 && chunk >= fit + 256) CHECK(p.chunk == fit);      // and no smaller than it has to be
    } else {
        CHECK(p.chunk <= 256);
        if (src != BS_TAB_HOST && npts >= 256 && chunk >= 256) CHECK(p.chunk == 256);
    }
    if (src == BS_TAB_HOST) CHECK(p.chunk * sumn <= ((size_t)1 << 25) || p.chunk == 1);
    // the reservations hold what the launches of a chunk write
    CHECK(p.b_gst == 8 * S * p.chunk && p.b_xa == 8 * p.chunk * (size_t)p.ldx && p.b_xb == p.b_xa);
    CHECK(p.b_btab == (tab ? 0 : 8 * 2 * p.chunk * nmax));
    CHECK(p.b_x == (dev ? 0 : 8 * p.chunk * (tab ? 2 * sumn : (size_t)d)) && p.b_out == (dev ? 0 : 8 * p.chunk * ((size_t)d + 1)));
    CHECK(p.lds_back == 4u * 8 * (size_t)p.ldx && p.lds_fwd == 4u * 8 * 2 * (size_t)p.ldx);
    if (p.chunk) {
        const int c = (int)p.chunk;
        CHECK(p.g_exact(c) >= 1 && p.g_exact(c) <= ncu * 8);
        for (int k = 0; k < d; k++) {
            CHECK((long long)p.g_back(k, c) * p.step[k].tp_back >= c && (long long)(p.g_back(k, c) - 1) * p.step[k].tp_back < c);
            CHECK((long long)p.g_fwd(k, c) * p.step[k].tp_fwd >= c && (long long)(p.g_fwd(k, c) - 1) * p.step[k].tp_fwd < c);
        }
    }
}

int main()
{
    const BsSrc srcs[] = {BS_X_HOST, BS_X_DEV, BS_TAB_HOST, BS_TAB_DEV};
    const int modes[] = {TTX_EVAL_EXACT, TTX_EVAL_MFMA, TTX_EVAL_AUTO};
    const int64_t counts[] = {0, 1, 255, 256, 257, 300, 100000, 3000000};
    const size_t chunks[] = {1, 64, 256, 1000, (size_t)1 << 17, (size_t)1 << 18};
    const size_t stores[] = {1, 8, 2047, 8 * 256, 100000, (size_t)1 << 20, (size_t)1 << 32, (size_t)1 << 40};
    std::vector<std::pair<std::vector<int>, std::vector<int>>> shapes = {
        {{7, 2, 51, 1, 9}, {1, 3, 17, 5, 4, 1}}, {{4, 5, 3, 2}, {1, 16, 33, 65, 1}}, {{2, 2, 2}, {1, 128, 128, 1}}, {{3, 2, 3}, {1, 96, 113, 1}},
        {{3, 4, 2, 5}, {1, 2, 70, 3, 1}}, {{5, 7}, {1, 3, 1}}, {{5}, {1, 1}},                           // d = 1
        {{2, 2, 2}, {1, 129, 2, 1}}, {{2, 2}, {1, 129, 1}},                                             // rank 129: refused
        {{2, 2}, {2, 3, 1}}, {{2, 2}, {1, 3, 2}}, {{3}, {2, 2}},                                        // boundary ranks != 1: refused
    };
    for (int rk = 1; rk <= 128; rk++) shapes.push_back({{3, 65, 2}, {1, rk, 129 - rk, 1}});            // every tier on either side
    shapes.push_back({std::vector<int>(256, 65), std::vector<int>(257, 64)});                           // the D_256 shape: d = 256, rank 64
    shapes.back().second.front() = shapes.back().second.back() = 1;
    for (const auto &s : shapes)
        for (BsSrc src : srcs) for (int mode : modes) for (int64_t npts : counts) for (size_t chunk : chunks) for (size_t store : stores)
            check(s.first, s.second, src, npts, mode, chunk, store);
    // the figures the header states: 32768 points per chunk on the D_256 shape with the default budget
    {
        const auto &s = shapes.back();
        const BgPlan p = bg_plan(256, s.first.data(), s.second.data(), 256, BS_X_DEV, 100000, TTX_EVAL_MFMA, (size_t)1 << 17, TTX_BG_STORE_DEFAULT);
        if (p.chunk != 32768 || p.S != 1 + 255 * 64) { printf("D_256: chunk %zu S %zu\n", p.chunk, p.S); return 1; }
        const BgPlan q = bg_plan(256, s.first.data(), s.second.data(), 256, BS_X_DEV, 100000, TTX_EVAL_MFMA, (size_t)1 << 17, 1000);     // a budget below one tile
        if (q.chunk != 256) { printf("D_256, budget below one tile: chunk %zu\n", q.chunk); return 1; }
    }
    printf("basis grad plan: ok (%lld plans)\n", nplans);
    return 0;
}
