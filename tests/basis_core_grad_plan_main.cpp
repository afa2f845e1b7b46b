// The plan of a core-gradient call (cg_plan, ttcross_amd/csrc/ttx_op_plan.h) as a stand-alone host program: no GPU, nothing loaded
// into Python.  Built by tests/test_basis_core_grad_cpu.py with the host compiler, plain and under the address and undefined-behaviour
// sanitizers.  Every rule is restated here independently of the header's code and compared; prints "basis core grad plan: ok (N plans)".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ttx_op_plan.h"

static long long nplans = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s fails (d=%d npts=%lld chunk=%zu store=%zu src=%d)\n", __LINE__, #c, d, (long long)npts, chunk, store, (int)src); exit(1); } } while (0)

static void check(const std::vector<int> &n, const std::vector<int> &r, BsSrc src, int64_t npts, int mode, size_t chunk, size_t store)
{
    const int d = (int)n.size(), ncu = 256;
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    const CgPlan p = cg_plan(d, n.data(), r.data(), ncu, src, !dev, npts, mode, chunk, store);
    nplans++;
    int rmax = 0;
    for (int v : r) rmax = std::max(rmax, v);
    if (rmax > 128) { CHECK(p.refusal == BS_RANK); return; }
    if (r[0] != 1 || r[d] != 1) { CHECK(p.refusal == BS_BOUNDARY); return; }
    CHECK(p.refusal == BS_OK);
    CHECK(p.ldx >= rmax && p.ldx % 4 == 0 && p.ldx < rmax + 4);
    // the store: X_1 .. X_(d-1) at the row stride ldx
    const size_t S = (size_t)(d - 1) * p.ldx;
    CHECK(p.S == S);
    for (int i = 1; i < d; i++) CHECK(p.soff(i) == (size_t)(i - 1) * p.ldx && p.soff(i) + p.ldx <= S);
    // the chunk cap: under the caller's chunk and under the store budget -- except that a budget below one tile gives 256
    size_t cap = chunk;
    if (S) { const size_t fit = store / (8 * S) / 256 * 256; cap = std::min(chunk, fit >= 256 ? fit : (size_t)256); }
    CHECK(p.cap == cap && p.cap >= 1);
    if (S && store / (8 * S) >= 256) CHECK(8 * S * p.cap <= store);
    CHECK(p.chunk <= cap && p.chunk <= (size_t)npts);
    if (npts > 0) CHECK(p.chunk >= 1);
    if (src != BS_TAB_HOST) CHECK(p.chunk == std::min(cap, (size_t)npts));
    size_t sumn = 0, nmax = 1, gsize = 0;
    double w = 0.0;
    for (int k = 0; k < d; k++) {
        CHECK(p.off[k] == sumn);
        sumn += (size_t)n[k]; nmax = std::max(nmax, (size_t)n[k]);
        w += (double)r[k] * n[k] * r[k + 1];
        const int big = std::max(r[k], r[k + 1]);
        // the chains: the tiers and LDS of bs_plan and of bg_plan's forward step
        CHECK(p.back[k].tier >= 1 && p.back[k].tier <= 8 && 16 * p.back[k].tier >= big && 16 * (p.back[k].tier - 1) < big);
        CHECK(p.back[k].tp == 64 * bs_ct(p.back[k].tier) && p.back[k].lds == 8u * 2 * (size_t)ev_lda(r[k]) * 16);
        CHECK(p.fwd[k].tier == p.back[k].tier && p.fwd[k].tp_fwd == 64 * bs_ct(p.fwd[k].tier));
        CHECK(p.fwd[k].lds_fwd == 8u * 2 * (size_t)TTX_BG_LDT * (size_t)((r[k + 1] + 15) / 16 * 16));
        // the accumulation: rows in tiles of 16 covering r0, columns j + n k in groups of 64 CT, segments from the shapes and the points per chunk alone
        const CgStep &s = p.step[k];
        CHECK(s.tier >= 1 && s.tier <= 8 && 16 * s.tier >= r[k] && 16 * (s.tier - 1) < r[k]);
        CHECK(s.size == (size_t)r[k] * n[k] * r[k + 1] && s.goff == gsize);
        gsize += s.size;
        const size_t wcol = 64 * (size_t)cg_ct(s.tier), ncol = (size_t)n[k] * r[k + 1];
        CHECK(cg_ct(s.tier) == 2 || cg_ct(s.tier) == 4);
        CHECK((size_t)s.ngrp * wcol >= ncol && ((size_t)s.ngrp - 1) * wcol < ncol);
        CHECK(s.seg >= 256 && s.seg % 16 == 0);
        const long long nsmax = ((long long)p.chunk + s.seg - 1) / s.seg;       // segments of a full chunk
        CHECK(nsmax >= (p.chunk ? 1 : 0) && nsmax <= 65535);
        const size_t want = std::max<size_t>(1, 512 / (size_t)s.ngrp);          // about TTX_CG_WG workgroups per launch of a full chunk
        const size_t even = ((p.chunk + want - 1) / want + 15) / 16 * 16;       // the points that spread a chunk evenly over them, in whole staged blocks
        CHECK((size_t)s.seg == std::max<size_t>(256, even));                    // unless the floor of 256 points binds
        CHECK(nsmax <= (long long)want);
        // the staged rows: the a operand's leading dimension covers the row tiles and is 16 mod 32, the window's covers its columns
        CHECK(cg_lda(s.tier) >= 16 * s.tier && cg_lda(s.tier) % 32 == 16 && cg_ldw(s.tier) >= (int)wcol && cg_ldw(s.tier) % 32 == 16);
        CHECK(cg_ldq(r[k + 1]) > r[k + 1] && cg_ldq(r[k + 1]) % 2 == 1);
        CHECK(s.lds == 8u * 16 * ((size_t)cg_lda(s.tier) + cg_ldw(s.tier) + cg_ldq(r[k + 1])));
        CHECK(s.lds <= 64 * 1024);                                              // no launch has to raise the LDS ceiling
        if (p.chunk) {
            const int c = (int)p.chunk, ns = p.nsplit(k, c);
            CHECK(ns >= 1 && (long long)ns * s.seg >= c && (long long)(ns - 1) * s.seg < c && ns <= nsmax);
            if (p.eff == TTX_EVAL_MFMA) CHECK(p.b_part >= 8 * s.size * (size_t)ns);
        }
    }
    CHECK(p.sumn == sumn && p.nmax == nmax && p.gsize == gsize);
    CHECK(p.flops == 6.0 * (double)npts * w);
    CHECK(p.eff == (mode != TTX_EVAL_AUTO ? mode : p.flops >= TTX_CG_AUTO_FLOPS ? TTX_EVAL_MFMA : TTX_EVAL_EXACT));
    if (src == BS_TAB_HOST) CHECK(p.chunk * sumn <= ((size_t)1 << 25) || p.chunk == 1);
    // the reservations hold what the launches of a chunk write; an empty call reserves only the host caller's gradient
    CHECK(p.b_cgg == (dev ? 0 : 8 * gsize));
    CHECK(p.b_gst == 8 * S * p.chunk && p.b_xa == 8 * p.chunk * (size_t)p.ldx && p.b_xb == p.b_xa);
    CHECK(p.b_btab == (tab ? 0 : 8 * p.chunk * nmax));
    CHECK(p.b_x == (dev ? 0 : 8 * p.chunk * ((tab ? sumn : (size_t)d) + 1)) && p.b_out == (dev ? 0 : 8 * p.chunk));
    if (p.eff != TTX_EVAL_MFMA || !p.chunk) CHECK(p.b_part == 0);
    if (p.chunk) {
        const int c = (int)p.chunk;
        CHECK(p.lds_back == 4u * 8 * (size_t)p.ldx && p.lds_fwd == 4u * 8 * 2 * (size_t)p.ldx);
        CHECK(p.g_exact(c) >= 1 && p.g_exact(c) <= ncu * 8);
        for (int k = 0; k < d; k++) {
            CHECK((long long)p.g_back(k, c) * p.back[k].tp >= c && (long long)(p.g_back(k, c) - 1) * p.back[k].tp < c);
            CHECK((long long)p.g_fwd(k, c) * p.fwd[k].tp_fwd >= c && (long long)(p.g_fwd(k, c) - 1) * p.fwd[k].tp_fwd < c);
        }
    }
    // the summation order depends on the points per chunk and not on the device or on npts otherwise: another CU count, and another
    // npts that gives the same points per chunk, give the same segments
    const CgPlan q = cg_plan(d, n.data(), r.data(), 64, src, !dev, (size_t)npts >= p.cap ? npts + 12345 : npts, mode, chunk, store);
    CHECK(q.cap == p.cap && q.chunk == p.chunk);
    for (int k = 0; k < d; k++) CHECK(q.step[k].seg == p.step[k].seg && q.step[k].ngrp == p.step[k].ngrp && q.step[k].tier == p.step[k].tier);
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
        {{5, 6, 4}, {1, 3, 2, 1}},                                                                      // the fit of the tests
        {{3, 51, 3}, {1, 32, 32, 1}},                                                                   // a 32 x 51 x 32 core: 102 column tiles, 7 column groups
        {{3, 5000, 3}, {1, 7, 5, 1}},                                                                   // a long mode: n r1 = 25000, 98 column groups
        {{3, 40000, 3}, {1, 7, 5, 1}},                                                                  // n r1 = 200000: 782 column groups, more than TTX_CG_WG: one segment per chunk
        {{2, 2, 2}, {1, 129, 2, 1}}, {{2, 2}, {1, 129, 1}},                                             // rank 129: refused
        {{2, 2}, {2, 3, 1}}, {{2, 2}, {1, 3, 2}}, {{3}, {2, 2}},                                        // boundary ranks != 1: refused
    };
    for (int rk = 1; rk <= 128; rk++) shapes.push_back({{3, 65, 2}, {1, rk, 129 - rk, 1}});            // every tier on either side; n r1 = 65 (129 - rk) is no multiple of 16 or 64 for most
    shapes.push_back({std::vector<int>(256, 65), std::vector<int>(257, 64)});                           // the D_256 shape: d = 256, rank 64
    shapes.back().second.front() = shapes.back().second.back() = 1;
    for (const auto &s : shapes)
        for (BsSrc src : srcs) for (int mode : modes) for (int64_t npts : counts) for (size_t chunk : chunks) for (size_t store : stores)
            check(s.first, s.second, src, npts, mode, chunk, store);
    // figures the documents state
    {
        const auto &s = shapes.back();
        const CgPlan p = cg_plan(256, s.first.data(), s.second.data(), 256, BS_X_DEV, false, 100000, TTX_EVAL_MFMA, (size_t)1 << 17, TTX_BG_STORE_DEFAULT);
        if (p.S != 255 * 64 || p.chunk != 32768) { printf("D_256: chunk %zu S %zu\n", p.chunk, p.S); return 1; }
        const CgPlan q = cg_plan(256, s.first.data(), s.second.data(), 256, BS_X_DEV, false, 100000, TTX_EVAL_MFMA, (size_t)1 << 17, 1000);     // a budget below one tile
        if (q.chunk != 256 || q.step[5].seg != 256 || p.step[5].ngrp != 33 || p.nsplit(5, 32768) != 15) { printf("D_256, budget below one tile: chunk %zu seg %d\n", q.chunk, q.step[5].seg); return 1; }
        const int n3[] = {3, 51, 3}, r3[] = {1, 32, 32, 1};
        const CgPlan t = cg_plan(3, n3, r3, 256, BS_TAB_DEV, false, 1000000, TTX_EVAL_MFMA, (size_t)1 << 18, TTX_BG_STORE_DEFAULT);
        if (t.step[1].tier != 2 || t.step[1].ngrp != 7 || t.nsplit(1, (int)t.chunk) * t.step[1].ngrp < 256) {                               // enough workgroups for 256 CUs
            printf("32 x 51 x 32: tier %d ngrp %d nsplit %d\n", t.step[1].tier, t.step[1].ngrp, t.nsplit(1, (int)t.chunk)); return 1;
        }
    }
    printf("basis core grad plan: ok (%lld plans)\n", nplans);
    return 0;
}
