// The plan of a JVP call (jv_plan, ttcross_amd/csrc/ttx_op_plan.h) as a stand-alone host program: no GPU, nothing loaded into Python.
// Built by tests/test_basis_jvp_cpu.py with the host compiler, plain and under the address and undefined-behaviour sanitizers.  Every
// rule is restated here independently of the header's code and compared; prints "basis jvp plan: ok (N plans)".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ttx_op_plan.h"

static long long nplans = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s fails (d=%d npts=%lld chunk=%zu src=%d)\n", __LINE__, #c, d, (long long)npts, chunk, (int)src); exit(1); } } while (0)

static void check(const std::vector<int> &n, const std::vector<int> &r, BsSrc src, int64_t npts, int mode, size_t chunk)
{
    const int d = (int)n.size(), ncu = 256;
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    const JvPlan p = jv_plan(d, n.data(), r.data(), ncu, src, !dev, npts, mode, chunk);
    nplans++;
    int rmax = 0;
    for (int v : r) rmax = std::max(rmax, v);
    if (rmax > 128) { CHECK(p.refusal == BS_RANK); return; }
    if (r[0] != 1 || r[d] != 1) { CHECK(p.refusal == BS_BOUNDARY); return; }
    CHECK(p.refusal == BS_OK);
    CHECK(p.ldx >= rmax && p.ldx % 4 == 0 && p.ldx < rmax + 4);
    // the chunk is the value call's: no state store bounds it
    const BsPlan v = bs_plan(d, n.data(), r.data(), ncu, src, npts, mode, chunk);
    CHECK(p.chunk == v.chunk && p.chunk <= chunk && p.chunk <= (size_t)npts);
    if (npts > 0) CHECK(p.chunk >= 1);
    size_t sumn = 0, nmax = 1, vsize = 0;
    double w = 0.0;
    for (int k = 0; k < d; k++) {
        CHECK(p.off[k] == sumn && p.voff[k] == vsize);
        sumn += (size_t)n[k]; nmax = std::max(nmax, (size_t)n[k]);
        vsize += (size_t)r[k] * n[k] * r[k + 1];
        w += (double)r[k] * n[k] * r[k + 1];
        const int big = std::max(r[k], r[k + 1]);
        const JvStep &s = p.step[k];
        CHECK(s.tier >= 1 && s.tier <= 8 && 16 * s.tier >= big && 16 * (s.tier - 1) < big && s.tier == v.step[k].tier);
        const int ct = jv_ct(s.tier), mh = jv_mh(s.tier);
        CHECK(ct == 1 || ct == 2 || ct == 4);
        CHECK(s.tp == 64 * ct);
        CHECK(mh >= 1 && mh <= s.tier && mh <= 5);
        CHECK((16 * s.tier + 16 * mh) * ct <= 384);                              // a lane's two states (16 MR CT registers) and two accumulator sets (16 MH CT) leave a quarter of the 512 registers

        // the row groups cover the rows of the mode, and no group is empty
        CHECK(s.gy >= 1 && 16 * mh * s.gy >= r[k] && 16 * mh * (s.gy - 1) < r[k]);
        // two buffers of two images of the group's rows x 16 columns; never above the default LDS ceiling
        const int rows = std::min(r[k], 16 * mh);
        CHECK(s.lds.bytes == 2u * 2 * 8 * (size_t)ev_lda(rows) * 16 && !s.lds.raise && s.lds.bytes <= 64 * 1024);
        CHECK(jv_waves(s.tier) == 1 || jv_waves(s.tier) == 2);
    }
    CHECK(p.sumn == sumn && p.nmax == nmax && p.vsize == vsize);
    CHECK(p.flops == 6.0 * (double)npts * w);
    CHECK(p.eff == (mode != TTX_EVAL_AUTO ? mode : p.flops >= TTX_JV_AUTO_FLOPS ? TTX_EVAL_MFMA : TTX_EVAL_EXACT));
    CHECK(TTX_JV_AUTO_FLOPS == TTX_BS_AUTO_FLOPS);
    if (src == BS_TAB_HOST) CHECK(p.chunk * sumn <= ((size_t)1 << 25) || p.chunk == 1);
    CHECK(p.row == (tab ? sumn : (size_t)d));
    CHECK(p.ystr == p.chunk * (size_t)p.ldx);
    if (!p.chunk) { CHECK(p.b_xa == 0 && p.b_xb == 0 && p.b_btab == 0 && p.b_x == 0 && p.b_out == 0 && p.b_v == 0); return; }     // an empty call reserves nothing
    // both states of a chunk in each buffer; val and dval of a host caller; the direction of a host caller
    CHECK(p.b_xa == 8 * 2 * p.chunk * (size_t)p.ldx && p.b_xb == p.b_xa);
    CHECK(p.b_btab == (tab ? 0 : 8 * p.chunk * nmax));
    CHECK(p.b_x == (dev ? 0 : 8 * p.chunk * p.row) && p.b_out == (dev ? 0 : 8 * 2 * p.chunk));
    CHECK(p.b_v == (dev ? 0 : 8 * vsize));
    const int c = (int)p.chunk;
    CHECK(p.exact_lds == 4u * 8 * 2 * (size_t)p.ldx);
    CHECK(p.g_exact(c) >= 1 && p.g_exact(c) <= ncu * 8);
    for (int k = 0; k < d; k++) CHECK((long long)p.g_gemm(k, c) * p.step[k].tp >= c && (long long)(p.g_gemm(k, c) - 1) * p.step[k].tp < c);
}

int main()
{
    const BsSrc srcs[] = {BS_X_HOST, BS_X_DEV, BS_TAB_HOST, BS_TAB_DEV};
    const int modes[] = {TTX_EVAL_EXACT, TTX_EVAL_MFMA, TTX_EVAL_AUTO};
    const int64_t counts[] = {0, 1, 255, 256, 257, 300, 100000, 3000000};
    const size_t chunks[] = {1, 64, 256, 1000, (size_t)1 << 17, (size_t)1 << 18};
    std::vector<std::pair<std::vector<int>, std::vector<int>>> shapes = {
        {{7, 2, 51, 1, 9}, {1, 3, 17, 5, 4, 1}}, {{4, 5, 3, 2}, {1, 16, 33, 65, 1}}, {{2, 2, 2}, {1, 128, 128, 1}}, {{3, 2, 3}, {1, 96, 113, 1}},
        {{3, 4, 2, 5}, {1, 2, 70, 3, 1}}, {{5, 7}, {1, 3, 1}}, {{5}, {1, 1}}, {{5, 6, 4}, {1, 3, 2, 1}},
        {{2, 2, 2}, {1, 129, 2, 1}}, {{2, 2}, {1, 129, 1}},                                             // rank 129: refused
        {{2, 2}, {2, 3, 1}}, {{2, 2}, {1, 3, 2}}, {{3}, {2, 2}},                                        // boundary ranks != 1: refused
    };
    for (int rk = 1; rk <= 128; rk++) shapes.push_back({{3, 65, 2}, {1, rk, 129 - rk, 1}});            // every tier on either side
    shapes.push_back({std::vector<int>(256, 65), std::vector<int>(257, 64)});                           // the D_256 shape
    shapes.back().second.front() = shapes.back().second.back() = 1;
    for (const auto &s : shapes)
        for (BsSrc src : srcs) for (int mode : modes) for (int64_t npts : counts) for (size_t chunk : chunks)
            check(s.first, s.second, src, npts, mode, chunk);
    // the segments of the fixed-order dot product
    for (long long tot : {0LL, 1LL, 59LL, 65535LL, 65536LL, 65537LL, 131072LL, 131073LL, 52000000LL}) {
        const long long L = dot_seg(tot);
        if (L % 256 || L * TTX_DOT_SEGS < tot || (tot > 0 && (L - 256) * TTX_DOT_SEGS >= tot) || (tot == 0 && L != 0)) { printf("dot_seg(%lld) = %lld\n", tot, L); return 1; }
    }
    if (dot_seg(65536) != 256 || dot_seg(65537) != 512) { printf("dot_seg at the boundary\n"); return 1; }
    // figures the documents state: the rows of rank 128 go to two workgroups of 64, the D_256 shape needs none of that
    {
        const int n3[] = {2, 2, 2}, r3[] = {1, 128, 128, 1};
        const JvPlan p = jv_plan(3, n3, r3, 256, BS_TAB_DEV, false, 300, TTX_EVAL_MFMA, (size_t)1 << 17);
        if (p.step[1].tier != 8 || p.step[1].gy != 2 || p.step[0].gy != 1 || p.step[2].gy != 2 || p.step[1].lds.bytes != 40960) { printf("bond128: gy %d lds %zu\n", p.step[1].gy, p.step[1].lds.bytes); return 1; }
        const auto &s = shapes.back();
        const JvPlan q = jv_plan(256, s.first.data(), s.second.data(), 256, BS_X_DEV, false, 100000, TTX_EVAL_AUTO, (size_t)1 << 17);
        if (q.chunk != 100000 || q.step[5].tier != 4 || q.step[5].gy != 1 || q.eff != TTX_EVAL_MFMA) { printf("D_256: chunk %zu\n", q.chunk); return 1; }
    }
    printf("basis jvp plan: ok (%lld plans)\n", nplans);
    return 0;
}
