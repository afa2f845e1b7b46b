// The plan of a call of ttx_sq_lognorm_grad (sqn_plan, ttcross_amd/csrc/ttx_op_plan.h) and the scalars its host code forms from the
// chains' results, as a stand-alone host program: no GPU, nothing loaded into Python.  Built by tests/test_sq_norm_cpu.py with the host
// compiler, plain and under the address and undefined-behaviour sanitizers.  Every rule is restated here independently of the header's
// code and compared; prints "sq norm plan: ok (N plans)".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ttx_op_plan.h"

static long long nplans = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s fails (d=%d mode=%d host=%d)\n", __LINE__, #c, d, mode, (int)host_g); exit(1); } } while (0)

static void check(const std::vector<int> &n, const std::vector<int> &r, bool host_g, int mode)
{
    const int d = (int)n.size();
    const SqnPlan p = sqn_plan(d, n.data(), r.data(), host_g, mode);
    nplans++;
    int rmax = 0;
    for (int v : r) rmax = std::max(rmax, v);
    if (rmax > 128) { CHECK(p.refusal == BS_RANK); return; }
    if (r[0] != 1 || r[d] != 1) { CHECK(p.refusal == BS_BOUNDARY); return; }
    CHECK(p.refusal == BS_OK && p.rmax == rmax);
    size_t g = 0, ns = 0, pr = 0, ymax = 1, pmax = 1;
    long long wg = 0;
    double fl = 0.0;
    int r1max = 1;
    for (int k = 0; k < d; k++) {
        CHECK(p.goff[k] == g && p.noff[k] == ns && p.proff[k] == pr);
        CHECK(p.first_e[k] == (long long)g && p.first_wg[k] == wg);
        const size_t rows = (size_t)r[k] * n[k], sz = rows * r[k + 1];
        const long long nw = (long long)((rows + 127) / 128);                   // 128 rows (a, i) per workgroup: 4 waves x 2 tiles of 16
        CHECK(nw >= 1 && (size_t)nw * TTX_SQN_ROWS >= rows && (size_t)(nw - 1) * TTX_SQN_ROWS < rows);
        wg += nw; g += sz; ns += (size_t)n[k]; pr += (size_t)r[k] * r[k];
        ymax = std::max(ymax, sz);
        pmax = std::max(pmax, (size_t)n[k] * std::max((size_t)r[k] * r[k], (size_t)r[k + 1] * r[k + 1]));   // one r x r matrix per index of the mode, either chain
        r1max = std::max(r1max, r[k + 1]);
        fl += 4.0 * r[k] * r[k] * (double)n[k] * r[k + 1] + 6.0 * r[k] * (double)n[k] * r[k + 1] * r[k + 1];
    }
    CHECK(p.goff[d] == g && p.gsize == g && p.nsum == ns && p.noff[d] == ns && p.tot_wg == wg && wg <= 0x7fffffffll);
    CHECK(p.proff[d] == pr && p.proff[d + 1] == pr + 1);                        // PR_d = [1] is stored like the others
    CHECK(p.tier == (r1max <= 16 ? 1 : r1max <= 32 ? 2 : r1max <= 64 ? 4 : 8) && 16 * p.tier >= r1max);
    CHECK(p.grid_exact >= 1 && p.grid_exact <= 4096 && ((size_t)p.grid_exact * 256 >= g || p.grid_exact == 4096));
    CHECK(p.b_w == 8 * g && p.b_pr == 8 * (pr + 1) && p.b_pl == 16 * (size_t)rmax * rmax && p.b_y == 8 * ymax && p.b_part == 8 * pmax && p.b_ex == 4 * 2 * (size_t)(d + 1));
    CHECK(p.b_g == (host_g ? 8 * g : 0));
    CHECK(p.lds_asm == 8u * 16 * 144 && p.lds_asm <= 64 * 1024 && TTX_SQN_LDA % 32 == 16 && TTX_SQN_LDA >= 128);
    CHECK(p.flops == fl);
    CHECK(p.eff == (mode == TTX_EVAL_AUTO ? (fl >= TTX_SQN_AUTO_FLOPS ? TTX_EVAL_MFMA : TTX_EVAL_EXACT) : mode));
}

int main()
{
    const int modes[3] = {TTX_EVAL_EXACT, TTX_EVAL_MFMA, TTX_EVAL_AUTO};
    const int ranks[] = {1, 2, 3, 15, 16, 17, 31, 32, 33, 64, 65, 113, 127, 128, 129};
    const int sizes[] = {1, 2, 3, 17, 51, 129};
    for (int mode : modes)
        for (int host = 0; host < 2; host++) {
            for (int ra : ranks)
                for (int rb : ranks)
                    for (int na : sizes)
                        for (int nb : sizes) {
                            check({na, nb, 2}, {1, ra, rb, 1}, host != 0, mode);
                            check({na, nb}, {1, ra, rb}, host != 0, mode);      // a boundary rank that is not 1 (unless rb is)
                        }
            check({5}, {1, 1}, host != 0, mode);
            check(std::vector<int>(255, 3), [] { std::vector<int> r(256, 8); r[0] = r[255] = 1; return r; }(), host != 0, mode);
        }
    // the scalars: den, logz and s_k from the definition's formulas, the exponent clamp, a Z far outside the double range
    {
        const int d = 0, mode = 0; const bool host_g = false;
        CHECK(sqn_clamp_exp(5) == 5 && sqn_clamp_exp(-200000) == -100000 && sqn_clamp_exp(1ll << 40) == 100000);
        CHECK(sqn_den(0.75, 0, 0.25) == 1.0 && sqn_den(0.5, 4000, 1e300) == 0.5 && sqn_den(0.5, -2, 1.0) == 0.5 + 4.0);
        CHECK(sqn_logz(0.5, 1, 0.0) == 1.0 * 0.6931471805599453 + log(0.5));
        CHECK(std::isfinite(sqn_logz(0.75, 5000, 0.0)) && std::fabs(sqn_logz(0.75, 5000, 0.0) - (5000 * 0.6931471805599453 + log(0.75))) < 1e-9);
        CHECK(sqn_scale(0.5, 10, 0.0, 1.0, 4, 6) == 4.0);                       // (2 * 1) / 0.5 = 4, exponent 4 + 6 - 10 = 0
        CHECK(sqn_scale(0.5, 10, 0.0, 3.0, 4, 5) == 6.0);                       // 12 * 2^-1
        CHECK(sqn_scale(0.5, 5000, 0.0, 1.0, 2600, 2410) == ldexp(4.0, 10));
        CHECK(std::isnan(sqn_scale(NAN, 0, 0.0, 1.0, 0, 0)) && std::isinf(sqn_scale(0.0, 0, 0.0, 1.0, 0, 0)));
    }
    printf("sq norm plan: ok (%lld plans)\n", nplans);
    return 0;
}
