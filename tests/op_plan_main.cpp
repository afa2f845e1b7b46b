// Stand-alone check of ttcross_amd/csrc/ttx_op_plan.h (host code only): prints the plan of a list of calls, one line each
// (tests/test_op_plan_cpu.py holds the expected lines), then checks every plan of a grid of trains against the device's LDS, the
// kernels' tiers and the bytes its own launches address.  Built plain and with -fsanitize=address,undefined by that test.
//
// A line names the call, then what the engine does with the plan: the effective mode, the slots it reserves with their bytes, in
// order, and the launches whose grid, tier or LDS the plan decides as kernel:grid:lds (a trailing ! where the LDS ceiling is raised
// first) -- of the first and the last chunk of a batch, of every mode of a top-K search.
#include "ttx_op_plan.h"

#include <cstdio>
#include <string>

struct Train { std::vector<int> n, r; int RM = 128, NM = 1; };
static Train train(const std::vector<int> &n, const std::vector<int> &r)
{
    Train T;
    T.n = n; T.r = r;
    T.NM = *std::max_element(n.begin(), n.end());
    T.RM = *std::max_element(r.begin(), r.end()) <= 64 ? 64 : 128;
    return T;
}
static Train equal_ranks(int d, int n, int rank) { std::vector<int> r(d + 1, rank); r[0] = r[d] = 1; return train(std::vector<int>(d, n), r); }
template <class T> static std::string list(const std::vector<T> &v)
{
    std::string s;
    for (size_t i = 0; i < v.size(); i++) s += (i ? "," : "") + std::to_string(v[i]);
    return s;
}
static void slot(const char *name, size_t bytes) { if (bytes) printf(" %s=%zu", name, bytes); }
static void launch(const char *name, int tier, int gx, int gy, const OpLds &l)
{
    printf(" %s", name);
    if (tier) printf("<%d>", tier);
    if (gy) printf(":%dx%d", gx, gy); else printf(":%d", gx);
    printf(":%zu%s", l.bytes, l.raise ? "!" : "");
}
static OpLds plain(size_t bytes) { OpLds l; l.bytes = bytes; return l; }
static size_t chunk_of(const Train &T, size_t chunk) { return chunk ? chunk : op_chunk_default(T.RM); }      // 0: the variable is unset

static void print_ev(const Train &T, int ncu, EvStage st, long long npts, int dd, int mode, size_t chunk)
{
    const int d = (int)T.n.size();
    const EvPlan p = ev_plan(d, T.n.data(), T.r.data(), T.NM, ncu, st, npts, dd, mode, chunk_of(T, chunk));
    printf("ev n=%s r=%s RM=%d NM=%d ncu=%d st=%d npts=%lld dd=%d mode=%d chunk=%zu -> eff=%d", list(T.n).c_str(), list(T.r).c_str(), T.RM, T.NM, ncu, (int)st, npts, dd, mode, chunk, p.eff);
    slot("IND", p.b_ind); slot("OUT", p.b_out); slot("FLAG", p.b_flag); slot("X", p.b_x); slot("XA", p.b_xa); slot("XB", p.b_xb); slot("SORT", p.b_sort);
    const long long nch = npts ? (npts + (long long)p.chunk - 1) / (long long)p.chunk : 0;
    printf(" chunks=%lld", nch);
    for (int e = 0; e < (nch > 1 ? 2 : (int)nch); e++) {
        const int c = (int)(e ? npts - (nch - 1) * (long long)p.chunk : std::min<long long>(npts, (long long)p.chunk));
        printf(e ? " | last:" : " | first:");
        if (p.eff == TTX_EVAL_EXACT) { launch("k_ev_exact", 0, p.g_wave(c), 0, plain(p.exact_lds)); continue; }
        launch("k_ev_init", 0, p.g_wave(c), 0, plain(0));
        for (int i = d - 2; i >= 0; i--) {
            const EvStep &s = p.step[i];
            launch("k_ev_hist", 0, p.g_sort(c), 0, plain(s.hist_lds)); launch("k_ev_scatter", 0, p.g_sort(c), 0, plain(s.hist_lds));
            launch("k_ev_gemm", s.tier, p.g_gemm(i, c), 0, s.lds);
        }
        launch("k_ev_final", 0, p.g_final(c), 0, plain(0));
    }
    printf("\n");
}
static void print_bs(const Train &T, int ncu, BsSrc src, long long npts, int mode, size_t chunk)
{
    const int d = (int)T.n.size();
    const BsPlan p = bs_plan(d, T.n.data(), T.r.data(), ncu, src, npts, mode, chunk_of(T, chunk));
    printf("bs n=%s r=%s RM=%d ncu=%d src=%d npts=%lld mode=%d chunk=%zu ->", list(T.n).c_str(), list(T.r).c_str(), T.RM, ncu, (int)src, npts, mode, chunk);
    if (p.refusal != BS_OK) { if (p.refusal == BS_RANK) printf(" refused rank rmax=%d\n", p.rmax); else printf(" refused boundary\n"); return; }
    printf(" eff=%d flops=%.17g", p.eff, p.flops);
    slot("XA", p.b_xa); slot("XB", p.b_xb); slot("BTAB", p.b_btab); slot("X", p.b_x); slot("OUT", p.b_out);
    const long long nch = npts ? (npts + (long long)p.chunk - 1) / (long long)p.chunk : 0;
    printf(" chunks=%lld", nch);
    for (int e = 0; e < (nch > 1 ? 2 : (int)nch); e++) {
        const int c = (int)(e ? npts - (nch - 1) * (long long)p.chunk : std::min<long long>(npts, (long long)p.chunk));
        printf(e ? " | last:" : " | first:");
        for (int i = d - 1; i >= 0; i--) {
            if (p.eff == TTX_EVAL_EXACT) launch("k_bs_exact", 0, p.g_exact(c), 0, plain(p.exact_lds));
            else launch("k_bs_gemm", p.step[i].tier, p.g_gemm(i, c), 0, plain(p.step[i].lds));
        }
    }
    printf("\n");
}
static void print_tk(const Train &T, int ncu, int K, const std::vector<int32_t> &fixed, int mode)
{
    const int d = (int)T.n.size();
    const TkPlan p = tk_plan(d, T.n.data(), T.r.data(), ncu, K, fixed.empty() ? nullptr : fixed.data(), mode);
    printf("tk n=%s r=%s RM=%d ncu=%d K=%d fixed=%s mode=%d ->", list(T.n).c_str(), list(T.r).c_str(), T.RM, ncu, K, fixed.empty() ? "-" : list(fixed).c_str(), mode);
    if (p.refused) { printf(" refused nmax=%d\n", p.nmax); return; }
    printf(" eff=%d flops=%.17g T=[%s] T=[%s] T=[%s] T=[%s]", p.eff, p.flops, list(p.nI).c_str(), list(p.ifx).c_str(), list(p.cnt).c_str(), list(p.sheet).c_str());
    slot("KP", p.b_kp); slot("KW", p.b_kw); slot("KS", p.b_ks); slot("KX", p.b_kx); slot("KREC", p.b_krec); slot("KSEL", p.b_ksel); slot("KOUT", p.b_kout);
    for (int k = d - 1; k >= 0; k--) {
        const TkStep &s = p.step[k];
        printf(" | k=%d:", k);
        if (p.eff == TTX_EVAL_MFMA) launch("k_tk_score_mfma", s.tier, s.gx, s.gy, s.lds);
        else launch("k_tk_score_exact", 0, s.g_exact, 0, plain(sizeof(double) * 4 * p.ldx));
        if (s.radix) for (int pass = 0; pass < 6; pass++) launch("k_tk_hist", 0, s.hg, 0, plain(0));
        launch("k_tk_count", 0, s.nblk, 0, plain(0)); launch("k_tk_scatter", 0, s.nblk, 0, plain(0));
        launch("k_tk_advance", 0, s.g_adv, 0, plain(sizeof(double) * 4 * p.ldx));
    }
    printf("\n");
}
static void print_ct(const Train &T, const std::vector<char> &contracted)
{
    CtPlan p;
    ct_plan((int)T.n.size(), T.n.data(), T.r.data(), contracted, p);
    printf("ct n=%s r=%s contracted=%s -> msize=%zu wsize=%zu bytes=%.17g tiles=%zu cores", list(T.n).c_str(), list(T.r).c_str(), list(std::vector<int>(contracted.begin(), contracted.end())).c_str(),
           p.msize, p.wsize, p.bytes, p.tiles.size());
    for (const CtCore &c : p.cores) printf(" %d:%zu:%zu", c.ta, c.moff, c.woff);
    printf("\n");
}
static void print_ma(const Train &T, const std::vector<int32_t> &m, int mode)
{
    const MaPlan p = ma_plan((int)T.n.size(), T.n.data(), T.r.data(), m.data(), mode);
    printf("ma n=%s r=%s m=%s mode=%d ->", list(T.n).c_str(), list(T.r).c_str(), list(m).c_str(), mode);
    if (p.refused) { printf(" refused tiles=%lld\n", std::max(p.tapp, p.tcpy)); return; }
    printf(" eff=%d rd=%.17g wr=%.17g fl=%.17g asize=%zu aoff=[%s]", p.eff, p.rd, p.wr, p.fl, p.asize, list(p.aoff).c_str());
    for (int a = 0; a < 2; a++) {
        printf(a ? " | copied %lld:" : " | applied %lld:", a ? p.tcpy : p.tapp);
        for (const MaCore &c : a ? p.cpy : p.app) printf(" %d,%d,%d,%d:%lld:%d,%d,%d", c.r0, c.n, c.r1, c.m, c.first, c.nab, c.npan, c.ngrp);
    }
    printf("\n");
}
// m terms, all of them the train T, sketched at rank L
static void print_rs(const Train &T, int m, int L, int mode)
{
    const int d = (int)T.n.size();
    const std::vector<const int32_t *> rt(m, T.r.data());
    std::vector<long long> S(d + 1, m);
    for (int k = 1; k < d; k++) S[k] = (long long)m * T.r[k];
    std::vector<int32_t> l(d + 1, 1);
    rs_sketch_ranks(d, T.n.data(), S.data(), L, l.data());
    const RsPlan p = rs_plan(d, T.n.data(), m, rt.data(), S.data(), l.data(), mode);
    printf("rs n=%s r=%s m=%d rank=%d mode=%d ->", list(T.n).c_str(), list(T.r).c_str(), m, L, mode);
    if (p.refused) { printf(" refused tiles=%lld\n", p.refused); return; }
    printf(" eff=%d fl=%.17g l=[%s] ooff=[%s] woff=[%s] tS=[%s] tA=[%s] ymax=%zu mmax=%zu omax=%zu blocks", p.eff, p.fl, list(l).c_str(), list(p.ooff).c_str(), list(p.woff).c_str(),
           list(p.tS).c_str(), list(p.tA).c_str(), p.ymax, p.mmax, p.omax);
    for (const RsBlk &B : p.blks) printf(" %d,%d:%d,%d:%lld,%lld", B.r0, B.r1, B.o0, B.o1, B.firstS, B.firstA);
    printf("\n");
}

static int bad = 0;
#define CHECK(c) do { if (!(c)) { if (bad++ < 20) printf("FAILED rank %d, n %d, mode %d, ncu %d: %s\n", rank, n, mode, ncu, #c); } } while (0)
static void check_lds(const OpLds &l, int rank, int n, int mode, int ncu) { CHECK(l.bytes <= TTX_LDS_DEVICE); CHECK(l.raise == (l.bytes > 64 * 1024)); }
// every figure of the three plans of one train against what the kernels address (their index expressions are restated here)
static long check_plans(int rank, int n, int mode, int ncu)
{
    const int d = 4, K = 17;
    const long long npts = 100000;
    const Train T = equal_ranks(d, n, rank);
    const EvPlan e = ev_plan(d, T.n.data(), T.r.data(), T.NM, ncu, EV_HOST_COORD, npts, d, mode, 4096);
    const size_t c = e.chunk;
    CHECK(e.eff == TTX_EVAL_EXACT || e.eff == TTX_EVAL_MFMA); CHECK(mode == TTX_EVAL_AUTO || e.eff == mode);
    CHECK(e.ldx >= rank && e.ldx % 4 == 0 && c == 4096);
    CHECK(e.b_ind >= sizeof(int) * c * d && e.b_out >= sizeof(double) * c && e.b_flag >= sizeof(int) * c && e.b_x >= sizeof(double) * c * d);
    CHECK(e.exact_lds >= 4 * (sizeof(double) * 2 * e.ldx + sizeof(int) * d) && e.exact_lds <= 64 * 1024);
    CHECK(e.g_wave((int)c) >= 1 && e.g_wave((int)c) <= 8 * ncu);
    if (e.eff == TTX_EVAL_MFMA) {
        CHECK(e.b_xa >= sizeof(double) * c * e.ldx && e.b_xb == e.b_xa);
        CHECK(e.b_sort >= sizeof(int) * (2 * c + (size_t)T.NM + 2 * ((size_t)T.NM + 1) + (size_t)n));     // valid, perm, cnt, off, tile, cur
        CHECK((int)e.step.size() == d - 1);
        for (int i = 0; i < d - 1; i++) {
            const EvStep &s = e.step[i];
            check_lds(s.lds, rank, n, mode, ncu);
            CHECK(s.q0 == T.r[i] && s.q1 == T.r[i + 1] && s.nmode == n);
            CHECK(16 * s.tier >= s.q0 && (s.tier == 1 || 8 * s.tier < s.q0));
            CHECK(s.lds.bytes >= sizeof(double) * ((size_t)(s.q0 + 15) & ~(size_t)15) * ((size_t)(s.q1 + 3) & ~(size_t)3));
            CHECK(s.hist_lds == sizeof(int) * n);
            CHECK((long long)e.g_gemm(i, (int)c) >= ((long long)c + TTX_EV_TP - 1) / TTX_EV_TP);        // a work item per TTX_EV_TP points at least
        }
    }
    const BsPlan b = bs_plan(d, T.n.data(), T.r.data(), ncu, BS_X_HOST, npts, mode, 4096);
    CHECK(b.refusal == BS_OK && b.chunk == 4096 && b.sumn == (size_t)d * n && b.nmax == (size_t)n && b.row == (size_t)d);
    CHECK(mode == TTX_EVAL_AUTO || b.eff == mode);
    CHECK(b.b_xa >= sizeof(double) * c * b.ldx && b.b_xb == b.b_xa && b.ldx >= rank && b.b_btab >= sizeof(double) * c * n && b.b_x >= sizeof(double) * c * d && b.b_out >= sizeof(double) * c);
    CHECK(b.exact_lds >= 4 * sizeof(double) * b.ldx && b.exact_lds <= 64 * 1024);
    for (int i = 0; i < d; i++) {
        const BsStep &s = b.step[i];
        const int q = std::max(T.r[i], T.r[i + 1]);
        CHECK(s.tier >= 1 && s.tier <= 8 && 16 * s.tier >= q && 16 * (s.tier - 1) < q);
        CHECK(s.tp == 64 * bs_ct(s.tier) && (long long)b.g_gemm(i, (int)c) * s.tp >= (long long)c);
        CHECK(s.lds >= sizeof(double) * 2 * (((size_t)T.r[i] + 15) & ~(size_t)15) * TTX_BS_KPAN && s.lds <= 64 * 1024);      // no raise: k_bs_gemm is launched without one
        CHECK(b.off[i] == (size_t)i * n);
    }
    const TkPlan t = tk_plan(d, T.n.data(), T.r.data(), ncu, K, nullptr, mode);
    CHECK(!t.refused && (mode == TTX_EVAL_AUTO || t.eff == mode) && t.ldx >= rank);
    CHECK(t.b_kp >= sizeof(double) * d * (size_t)t.ldx * t.ldx && t.b_kx >= sizeof(double) * 2 * K * t.ldx && t.b_krec >= sizeof(int) * (size_t)d * K);
    CHECK(t.b_kout >= 2 * (sizeof(double) * K + sizeof(int) * (size_t)K * d));
    for (int k = 0; k < d; k++) {
        const TkStep &s = t.step[k];
        const long long M = t.sheet[k];
        check_lds(s.lds, rank, n, mode, ncu);
        CHECK(M == (long long)t.cnt[k + 1] * t.nI[k] && M <= TTX_TK_SHEET && t.cnt[k] == std::min<long long>(K, M) && t.ifx[k] == -1 && t.nI[k] == n);
        CHECK(16 * s.tier >= T.r[k] && (s.tier == 1 || 8 * s.tier < T.r[k]));
        CHECK(s.lds.bytes >= sizeof(double) * 64 * ((((size_t)T.r[k] + 15) & ~(size_t)15) + 2));       // 64 columns of y, rows padded to 16 and two more
        CHECK((long long)s.gx * s.niper >= t.nI[k] && s.gy * 64 >= t.cnt[k + 1] && s.niper >= 1);
        CHECK(s.radix == (M > K) && (long long)s.nblk * TTX_TK_CHUNK >= M && s.nblk <= TTX_TK_SHEET / TTX_TK_CHUNK);
        CHECK(s.g_exact >= 1 && s.g_exact <= 8 * ncu && s.g_adv >= 1 && s.g_adv <= 8 * ncu && (!s.radix || (s.hg >= 1 && s.hg <= 4 * ncu)));
        CHECK(t.b_kw >= sizeof(double) * (size_t)T.r[k] * t.nI[k] * T.r[k + 1] && t.b_ks >= sizeof(tk_u64) * (size_t)M);
        CHECK(t.b_ksel >= sizeof(tk_u64) * (TKS_WORDS + (size_t)s.nblk) + sizeof(unsigned) * TTX_TK_BINS);
    }
    const std::vector<int32_t> mm = {n + 1, 0, 130, 0};
    const MaPlan a = ma_plan(d, T.n.data(), T.r.data(), mm.data(), mode);
    CHECK(!a.refused && a.tapp <= 0x7fffffffll && a.tcpy <= 0x7fffffffll && a.app.size() == 2 && a.cpy.size() == 2 && (mode == TTX_EVAL_AUTO || a.eff == mode));
    CHECK(a.asize == (size_t)(n + 1) * n + (size_t)130 * n && a.aoff[0] == 0 && a.aoff[1] == (size_t)(n + 1) * n);
    for (int side = 0; side < 2; side++) {
        long long first = 0;
        for (const MaCore &c : side ? a.cpy : a.app) {
            CHECK(c.first == first && 16 * c.nab >= c.r0 && c.npan * TTX_MA_JP >= c.m && (long long)c.ngrp * TTX_MA_UNITS >= (long long)c.nab * c.r1);
            first += (long long)c.ngrp * c.npan;
        }
        CHECK(first == (side ? a.tcpy : a.tapp));
    }
    const int m = 3;
    const std::vector<const int32_t *> rt(m, T.r.data());
    std::vector<long long> S(d + 1, m);
    for (int k = 1; k < d; k++) S[k] = (long long)m * T.r[k];
    std::vector<int32_t> l(d + 1, 1);
    rs_sketch_ranks(d, T.n.data(), S.data(), 64, l.data());
    const RsPlan q = rs_plan(d, T.n.data(), m, rt.data(), S.data(), l.data(), mode);
    CHECK(!q.refused && (mode == TTX_EVAL_AUTO || q.eff == mode) && q.blks.size() == (size_t)d * m);
    for (int k = 1; k <= d; k++) {
        CHECK(q.ooff[k] - q.ooff[k - 1] == (size_t)l[k - 1] * n * l[k] && q.omax >= q.ooff[k] - q.ooff[k - 1]);
        CHECK(q.woff[k + 1] - q.woff[k] == (size_t)S[k] * l[k] && q.ymax >= (size_t)l[k - 1] * n * S[k] && q.mmax >= (size_t)l[k] * S[k] && q.tA[k] <= 0x7fffffffll);
        long long tS = 0, tA = 0;
        for (int t = 0; t < m; t++) {
            const RsBlk &B = q.blks[(size_t)(k - 1) * m + t];
            CHECK(B.firstS == tS && B.firstA == tA && B.o0 == t * T.r[k - 1] && B.o1 == t * T.r[k]);
            tS += (B.r0 + 15) / 16; tA += (long long)((l[k - 1] + 15) / 16) * (((long long)n * B.r1 + 63) / 64);
        }
        CHECK(tS == q.tS[k] && tA == q.tA[k]);
    }
    return 5;
}

int main()
{
    const int ranks[] = {1, 16, 17, 32, 33, 64, 65, 80, 81, 112, 113, 128}, ncus[] = {256, 8};
    const Train U = train({3, 4, 2, 5, 3, 2, 4, 3}, {1, 3, 17, 64, 65, 9, 128, 2, 1});      // the unequal chain of the GPU tests
    const Train D = equal_ranks(3, 4, 64);
    for (int ncu : ncus) {
        for (int rk : ranks) {
            const Train T = equal_ranks(4, 3, rk);
            print_ev(T, ncu, EV_HOST_INDEX, 300, 0, TTX_EVAL_MFMA, 0); print_ev(T, ncu, EV_HOST_INDEX, 300, 0, TTX_EVAL_EXACT, 0);
            print_bs(T, ncu, BS_X_HOST, 300, TTX_EVAL_MFMA, 0); print_bs(T, ncu, BS_X_HOST, 300, TTX_EVAL_EXACT, 0);
            print_tk(T, ncu, 17, {}, TTX_EVAL_MFMA); print_tk(T, ncu, 17, {}, TTX_EVAL_EXACT);
            if (ncu != ncus[0]) continue;                                       // these two ask the device nothing
            print_ma(T, {5, 0, 17, 0}, TTX_EVAL_AUTO); print_rs(T, 2, 17, TTX_EVAL_AUTO);
        }
        print_ev(U, ncu, EV_HOST_INDEX, 300, 0, TTX_EVAL_MFMA, 0); print_bs(U, ncu, BS_X_DEV, 300, TTX_EVAL_MFMA, 0); print_tk(U, ncu, 17, {}, TTX_EVAL_MFMA);
        // top-K: K, one mode held fixed, K times the largest mode at and past TTX_TK_SHEET
        for (int K : {1, 17, 100}) { print_tk(D, ncu, K, {}, TTX_EVAL_EXACT); print_tk(D, ncu, K, {}, TTX_EVAL_AUTO); }
        print_tk(D, ncu, 17, {0, 2, 0}, TTX_EVAL_MFMA);
        print_tk(train({2, 4096, 2}, {1, 2, 2, 1}), ncu, 4096, {}, TTX_EVAL_EXACT); print_tk(train({2, 4097, 2}, {1, 2, 2, 1}), ncu, 4096, {}, TTX_EVAL_EXACT);
        // the batches: point counts, chunks, the entries
        for (long long npts : {0, 1, 63, 64, 65, 300})
            for (size_t chunk : {(size_t)7, (size_t)64, (size_t)0}) { print_ev(D, ncu, EV_HOST_INDEX, npts, 0, TTX_EVAL_MFMA, chunk); print_bs(D, ncu, BS_TAB_HOST, npts, TTX_EVAL_MFMA, chunk); }
        print_ev(D, ncu, EV_ON_DEVICE, 300, 0, TTX_EVAL_EXACT, 64); print_ev(D, ncu, EV_HOST_COORD, 300, 5, TTX_EVAL_MFMA, 64);
        print_bs(D, ncu, BS_X_DEV, 300, TTX_EVAL_EXACT, 64); print_bs(D, ncu, BS_TAB_DEV, 300, TTX_EVAL_MFMA, 64);
        print_bs(train({3, 3, 3}, {1, 129, 4, 1}), ncu, BS_X_HOST, 10, TTX_EVAL_EXACT, 0); print_bs(train({3, 3, 3}, {2, 4, 4, 1}), ncu, BS_X_HOST, 10, TTX_EVAL_EXACT, 0);
        // AUTO on either side of each break-even.  ev on D: w = 4224, saving 5.28e-9 + 0.858e-9 s per point against 69e-6 + 13.5168e-6 s
        print_ev(D, ncu, EV_HOST_INDEX, 13443, 0, TTX_EVAL_AUTO, 0); print_ev(D, ncu, EV_HOST_INDEX, 13444, 0, TTX_EVAL_AUTO, 0);
        // bs on D: 2 npts 16896 flops against 4e8; tk on equal ranks 128, n = 5000: 1.6512e8 + 3.2897e8 K flops against 3e9
        print_bs(D, ncu, BS_X_DEV, 11837, TTX_EVAL_AUTO, 0); print_bs(D, ncu, BS_X_DEV, 11838, TTX_EVAL_AUTO, 0);
        print_tk(equal_ranks(3, 5000, 128), ncu, 8, {}, TTX_EVAL_AUTO); print_tk(equal_ranks(3, 5000, 128), ncu, 9, {}, TTX_EVAL_AUTO);
    }
    // mode_apply: no mode applied, all applied, m of 1, 16, 17 and 130; its AUTO break-even (2 r0 r1 n m flops against 1e7)
    print_ma(U, {0, 0, 0, 0, 0, 0, 0, 0}, TTX_EVAL_MFMA); print_ma(U, {1, 16, 17, 130, 1, 16, 17, 130}, TTX_EVAL_EXACT);
    print_ma(D, {0, 76, 0}, TTX_EVAL_AUTO); print_ma(D, {0, 77, 0}, TTX_EVAL_AUTO);
    print_ma(train({2, 32000, 2}, {1, 128, 128, 1}), {32000, 32000, 32000}, TTX_EVAL_MFMA);
    print_ma(equal_ranks(3, 2, 128), {0, 2000000000, 0}, TTX_EVAL_MFMA);            // more workgroups than a launch takes: refused
    // lincomb_round: 1, 2 and 5 terms at sketch ranks 1, 17 and 128
    for (int m : {1, 2, 5}) for (int L : {1, 17, 128}) { print_rs(U, m, L, TTX_EVAL_MFMA); print_rs(D, m, L, TTX_EVAL_AUTO); }
    print_ct(U, std::vector<char>(8, 1)); print_ct(U, {1, 0, 1, 1, 0, 0, 1, 1}); print_ct(equal_ranks(4, 3, 128), {0, 1, 1, 0});

    long plans = 0;
    for (int rank = 1; rank <= 128; rank++)
        for (int n : {2, 5, 33})
            for (int mode : {TTX_EVAL_EXACT, TTX_EVAL_MFMA, TTX_EVAL_AUTO})
                for (int ncu : ncus) plans += check_plans(rank, n, mode, ncu);
    if (bad) printf("op plan: %d checks FAILED\n", bad);
    else printf("op plan: ok (%ld plans)\n", plans);
    return bad != 0;
}
