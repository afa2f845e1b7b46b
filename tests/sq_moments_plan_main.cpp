// The plan of a call of ttx_sq_moments (sqm_plan, ttcross_amd/csrc/ttx_op_plan.h) as a stand-alone host program: no GPU, nothing loaded into
// Python.  Built by tests/test_sq_moments_cpu.py with the host compiler, plain and under the address and undefined-behaviour sanitizers.
// The rules are restated here independently of the header's code and compared; prints "sq moments plan: ok (N plans)".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ttx_op_plan.h"

static long long nplans = 0;
#define CHECK(c) do { if (!(c)) { printf("line %d: %s fails (d=%d mode=%d batch_env=%lld)\n", __LINE__, #c, d, mode, batch_env); exit(1); } } while (0)

static SqmPlan check(const std::vector<int> &n, const std::vector<int> &r, const std::vector<unsigned char> &s, bool band, bool mom, bool z, int mode, long long batch_env)
{
    const int d = (int)n.size();
    const SqmPlan p = sqm_plan(d, n.data(), r.data(), s.empty() ? nullptr : s.data(), band, mom, z, mode, batch_env);
    nplans++;
    int rmax = 0, nmax = 1;
    for (int v : r) rmax = std::max(rmax, v);
    for (int v : n) nmax = std::max(nmax, v);
    if (rmax > 128) { CHECK(p.refusal == SQM_RANK); return p; }
    if (r[0] != 1 || r[d] != 1) { CHECK(p.refusal == SQM_BOUNDARY); return p; }
    if (!band && !mom && !z) { CHECK(p.refusal == SQM_NOTHING); return p; }
    CHECK(p.refusal == SQM_OK && p.rmax == rmax && p.nmax == nmax);
    std::vector<int> sel;
    if (mom) for (int k = 0; k < (int)s.size(); k++) if (s[k]) sel.push_back(k);
    CHECK(p.sel == sel);
    // the carried steps: every selected k below the largest selected mode is carried from bond k to bond l_max - 1
    long long steps = 0;
    size_t ndots = 0;
    for (size_t x = 0; x < sel.size(); x++) { steps += sel.back() - sel[x]; ndots += 2 + x; }
    CHECK(p.steps == steps && p.ndots == ndots);
    CHECK(p.members == (sel.size() > 1 ? (int)sel.size() - 1 : 0));
    size_t ymax = 1, pn = 1, p1 = 1, ns = 0, pr = 0;
    for (int k = 0; k < d; k++) {
        CHECK(p.noff[k] == ns && p.proff[k] == pr);
        ymax = std::max(ymax, (size_t)r[k] * n[k] * r[k + 1]);
        pn = std::max(pn, (size_t)n[k] * std::max((size_t)r[k] * r[k], (size_t)r[k + 1] * r[k + 1]));
        p1 = std::max(p1, (size_t)r[k + 1] * r[k + 1]);
        ns += (size_t)n[k]; pr += (size_t)r[k] * r[k];
    }
    CHECK(p.nsum == ns && p.proff[d] == pr && p.proff[d + 1] == pr + 1);
    CHECK(p.eff == (mode == TTX_EVAL_AUTO ? (p.flops >= TTX_SQM_AUTO_FLOPS ? TTX_EVAL_MFMA : TTX_EVAL_EXACT) : mode) && p.flops > 0.0);
    const size_t per = 8 * (ymax + (p.eff == TTX_EVAL_MFMA ? p1 : pn));
    CHECK(p.per_member == per);
    // the cut: the work space of a launch stays under the cap unless a single member is above it; the grid's z axis holds n members
    CHECK(p.batch >= 1 && (p.batch == 1 || (size_t)p.batch * per <= TTX_SQM_CAP_BYTES));
    CHECK((long long)p.batch * nmax <= 65535 || p.batch == 1);
    CHECK(p.batch <= std::max(1, p.members));
    if (batch_env >= 1) CHECK(p.batch <= batch_env);
    if (p.members) {
        CHECK(p.b_w == (size_t)p.batch * 8 * ymax && p.b_w + p.b_cpart == (size_t)p.batch * per);
        CHECK(p.b_w + p.b_cpart <= TTX_SQM_CAP_BYTES || p.batch == 1);
        // the batch is not smaller than it has to be: one more member would break a limit
        const long long b1 = (long long)p.batch + 1;
        CHECK(b1 > p.members || (size_t)b1 * per > TTX_SQM_CAP_BYTES || b1 * nmax > 65535 || (batch_env >= 1 && b1 > batch_env));
        for (int m = 1; m <= p.members; m++) CHECK(p.cuts(m) == (m + p.batch - 1) / p.batch && (long long)p.cuts(m) * p.batch >= m);
    } else CHECK(p.b_w == 0 && p.b_cpart == 0);
    CHECK(p.b_carry == 16 * (size_t)p.members * rmax * rmax + 4 * (size_t)std::max(1, p.members));
    CHECK(p.b_band == (band ? 16 * ns : 0) && p.b_ra == 16 * (size_t)rmax * rmax && p.b_dots == 12 * std::max<size_t>(1, ndots));
    CHECK(p.b_pr == 8 * (pr + 1) && p.b_pl == p.b_pr && p.b_ex == 8 * (size_t)(d + 1) && p.b_y == 16 * ymax && p.b_part == 8 * pn);
    return p;
}

int main()
{
    const int modes[3] = {TTX_EVAL_EXACT, TTX_EVAL_MFMA, TTX_EVAL_AUTO};
    const long long envs[] = {0, 1, 3, 1000};
    for (int mode : modes)
        for (long long batch_env : envs) {
            const int d = 0;
            // the D_64 shape and the D_256 shape, all modes selected
            {
                std::vector<int> r(64, 16); r[0] = r[63] = 1;
                const SqmPlan p = check(std::vector<int>(63, 51), r, std::vector<unsigned char>(63, 1), true, true, true, mode, batch_env);
                CHECK(p.steps == 63 * 62 / 2 && p.members == 62);
                if (!batch_env) CHECK(p.batch == 62);                           // the whole train fits under the cap
            }
            {
                std::vector<int> r(256, 64); r[0] = r[255] = 1;
                const SqmPlan p = check(std::vector<int>(255, 101), r, std::vector<unsigned char>(255, 1), true, true, true, mode, batch_env);
                CHECK(p.steps == 255 * 254 / 2 && p.members == 254);
                if (!batch_env) CHECK(p.batch < 254 && p.batch >= 32 && (size_t)p.batch * p.per_member <= TTX_SQM_CAP_BYTES);   // W alone would be 0.84 GB
                // six selected modes: first, two adjacent, the middle, the last two
                std::vector<unsigned char> s(255, 0);
                s[0] = s[7] = s[8] = s[127] = s[253] = s[254] = 1;
                const SqmPlan q = check(std::vector<int>(255, 101), r, s, false, true, false, mode, batch_env);
                CHECK(q.steps == 254 + 247 + 246 + 127 + 1 && q.members == 5);
            }
            // ragged shapes, every selection of a five-mode train, every set of outputs
            const std::vector<int> n = {7, 2, 51, 1, 9}, r = {1, 3, 17, 5, 128, 1};
            for (int bits = 0; bits < 32; bits++) {
                std::vector<unsigned char> s(5);
                for (int k = 0; k < 5; k++) s[k] = (bits >> k) & 1;
                for (int o = 0; o < 8; o++) check(n, r, s, o & 1, o & 2, o & 4, mode, batch_env);
            }
            check(n, r, {}, true, false, true, mode, batch_env);                // no observable at all
            check({5}, {1, 1}, {1}, true, true, true, mode, batch_env);
            // the refusals of the plan: ranks above 128, boundary ranks, every output null
            CHECK(check({3, 3}, {1, 129, 1}, {1, 1}, true, true, true, mode, batch_env).refusal == SQM_RANK);
            CHECK(check({3, 3}, {2, 3, 1}, {1, 1}, true, true, true, mode, batch_env).refusal == SQM_BOUNDARY);
            CHECK(check({3, 3}, {1, 3, 2}, {1, 1}, true, true, true, mode, batch_env).refusal == SQM_BOUNDARY);
            CHECK(check({3, 3}, {1, 3, 1}, {1, 1}, false, false, false, mode, batch_env).refusal == SQM_NOTHING);
            // a mode so large that one member is above the cap: the batch is 1, nothing is refused
            CHECK(check({40000, 2}, {1, 128, 1}, {1, 1}, true, true, true, mode, batch_env).batch == 1);
        }
    {
        const int d = 0, mode = 0; const long long batch_env = 0;
        CHECK(sqm_ratio(0.25, 0.5, 4, 6, 10) == 0.5 && sqm_ratio(0.25, 0.5, 2600, 2410, 5000) == ldexp(0.5, 10));
        CHECK(std::isnan(sqm_ratio(NAN, 0.5, 0, 0, 0)) && sqm_ratio(1.0, 0.5, 1ll << 40, 0, 0) == INFINITY);
    }
    printf("sq moments plan: ok (%lld plans)\n", nplans);
    return 0;
}
