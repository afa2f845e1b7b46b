// The controller of the Gauss-Newton solver (fit_run, ttcross_amd/csrc/ttx_fit_plan.h) on a dense CPU backend: a small tensor train
// evaluated by plain loops, J V by replacing one core at a time, J^T c by linearity (one evaluation per unit block).  No GPU, nothing
// loaded into Python.  Built by tests/test_basis_jvp_cpu.py with the host compiler, plain and under the address and undefined-behaviour
// sanitizers.  Checks: every stop reason occurs, every output array is filled, the lambda schedule is followed, a rejected step leaves
// the parameters bit-identical, a zero gradient at entry stops with reason 3, and a start near the truth converges.  Prints "fit plan: ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ttx_fit_plan.h"

namespace {
const int D = 3, N[D] = {3, 4, 2}, R[D + 1] = {1, 2, 2, 1}, P = 40;
struct Rng { unsigned long long s; double next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0 * 2.0 - 1.0; } };

struct Dense {
    std::vector<double> theta, snap, y, w, phi[D], val, res, c, q, vec[FIT_NVEC];
    size_t off[D + 1];
    int hostile = 0;                            // > 0: every trial loss is reported as worse than the current one
    double last_loss = 0.0;
    long n_jvp = 0, n_cg = 0, n_restore = 0;
    Dense()
    {
        off[0] = 0;
        for (int i = 0; i < D; i++) off[i + 1] = off[i] + (size_t)R[i] * N[i] * R[i + 1];
        theta.assign(off[D], 0.0);
        for (auto &v : vec) v.assign(off[D], 0.0);
        val.assign(P, 0.0); res = c = q = val;
    }
    // f(x_p) of the train whose cores are taken from t, core `swap` (if >= 0) from s instead
    double eval(int p, const std::vector<double> &t, int swap, const std::vector<double> &s) const
    {
        double x[4] = {1.0, 0.0, 0.0, 0.0};
        for (int i = D - 1; i >= 0; i--) {
            const double *U = (i == swap ? s.data() : t.data()) + off[i];
            double z[4] = {0.0, 0.0, 0.0, 0.0};
            for (int a = 0; a < R[i]; a++)
                for (int j = 0; j < N[i]; j++) {
                    double tj = 0.0;
                    for (int k = 0; k < R[i + 1]; k++) tj += U[a + R[i] * (j + N[i] * k)] * x[k];
                    z[a] += phi[i][(size_t)p * N[i] + j] * tj;
                }
            memcpy(x, z, sizeof(x));
        }
        return x[0];
    }
    int loss(double *l)
    {
        double s = 0.0;
        for (int p = 0; p < P; p++) { val[p] = eval(p, theta, -1, theta); res[p] = val[p] - y[p]; c[p] = w[p] * res[p]; s += c[p] * res[p]; }
        *l = 0.5 * s;
        if (hostile && hostile++ > 1) *l = last_loss + 1.0;                    // the loss at entry is honest, every trial is worse
        else last_loss = *l;
        return 0;
    }
    int core_grad(int from_q, int dst)
    {
        n_cg++;
        std::vector<double> unit(off[D], 0.0), &g = vec[dst];
        for (int i = 0; i < D; i++)
            for (size_t e = off[i]; e < off[i + 1]; e++) {
                unit[e] = 1.0;
                double s = 0.0;
                for (int p = 0; p < P; p++) s += (from_q ? w[p] * q[p] : c[p]) * eval(p, theta, i, unit);
                g[e] = s;
                unit[e] = 0.0;
            }
        return 0;
    }
    int jvp(int v)
    {
        n_jvp++;
        for (int p = 0; p < P; p++) { double s = 0.0; for (int i = 0; i < D; i++) s += eval(p, theta, i, vec[v]); q[p] = s; }
        return 0;
    }
    int dot(int a, int b, double *s) { double t = 0.0; for (size_t e = 0; e < off[D]; e++) t += vec[a][e] * vec[b][e]; *s = t; return 0; }
    int axpby(double al, int x, double be, int yv) { for (size_t e = 0; e < off[D]; e++) vec[yv][e] = (al * vec[x][e]) + (be * vec[yv][e]); return 0; }
    int zero(int v) { vec[v].assign(off[D], 0.0); return 0; }
    int copy(int dst, int s) { vec[dst] = vec[s]; return 0; }
    int snapshot() { snap = theta; return 0; }
    int restore() { theta = snap; n_restore++; return 0; }
    int apply(int s) { for (size_t e = 0; e < off[D]; e++) theta[e] = theta[e] + 1.0 * vec[s][e]; return 0; }
};

struct Run { std::vector<double> loss, lambda; std::vector<int32_t> cg, acc; ttx_fit_result res; };
const double SENT = -12345.0;
Run run(Dense &b, const ttx_fit_opts &o)
{
    Run r;
    r.loss.assign(o.max_iter + 1, SENT); r.lambda.assign(o.max_iter, SENT); r.cg.assign(o.max_iter, -7); r.acc.assign(o.max_iter, -7);
    r.res.iters = r.res.stop = -1;
    FitHistory h;
    h.loss = r.loss.data(); h.lambda = r.lambda.data(); h.cg_iters = r.cg.data(); h.accepted = r.acc.data();
    if (fit_run(b, o, h, &r.res)) { printf("fit_run failed\n"); exit(1); }
    return r;
}
#define CHECK(c) do { if (!(c)) { printf("line %d: %s fails\n", __LINE__, #c); exit(1); } } while (0)
// what holds for every run: all arrays filled, the schedule followed, the loss never rises, the counts consistent
void common(const Dense &b, const ttx_fit_opts &o, const Run &r)
{
    CHECK(r.res.iters >= 0 && r.res.iters <= o.max_iter && r.res.stop >= 1 && r.res.stop <= 5);
    long passes = 0, accepted = 0;
    for (int i = 0; i < o.max_iter; i++) {
        CHECK(r.lambda[i] != SENT && r.loss[i + 1] != SENT && r.cg[i] >= 0 && (r.acc[i] == 0 || r.acc[i] == 1));
        if (i < r.res.iters) {
            CHECK(r.cg[i] >= 1 && r.cg[i] <= o.cg_max);
            CHECK(r.acc[i] ? r.loss[i + 1] < r.loss[i] : (r.loss[i + 1] == r.loss[i] || (std::isnan(r.loss[i]) && std::isnan(r.loss[i + 1]))));
            const double next = r.acc[i] ? r.lambda[i] * o.lambda_down : r.lambda[i] * o.lambda_up;     // the schedule, bit for bit
            if (i + 1 < o.max_iter) CHECK(r.lambda[i + 1] == next);
            passes += r.cg[i]; accepted += r.acc[i];
        } else {
            CHECK(r.cg[i] == 0 && r.acc[i] == 0 && (r.loss[i + 1] == r.loss[r.res.iters] || std::isnan(r.loss[i + 1])));
            if (i > r.res.iters) CHECK(r.lambda[i] == r.lambda[i - 1]);
        }
    }
    CHECK(r.loss[0] != SENT);
    if (o.max_iter > 0 && r.res.iters > 0) CHECK(r.lambda[0] == o.lambda0);
    CHECK(b.n_jvp == passes);
    CHECK(b.n_cg >= passes && b.n_cg <= passes + 1 + accepted);
}
Dense problem(double rel, unsigned long long seed)
{
    Dense b;
    Rng g{seed};
    std::vector<double> truth(b.off[D]);
    for (auto &t : truth) t = g.next();
    for (int i = 0; i < D; i++) { b.phi[i].resize((size_t)P * N[i]); for (auto &v : b.phi[i]) v = g.next(); }
    b.y.resize(P); b.w.assign(P, 1.0);
    for (int p = 0; p < P; p++) b.y[p] = b.eval(p, truth, -1, truth);
    for (size_t e = 0; e < b.off[D]; e++) b.theta[e] = rel < 0.0 ? g.next() : truth[e] * (1.0 + rel * g.next());
    return b;
}
}

int main()
{
    const ttx_fit_opts base = {12, 60, 8, TTX_EVAL_EXACT, 1e-2, 0.3, 4.0, 1e-3, 0.0};
    bool seen[6] = {false, false, false, false, false, false};
    {   // near the truth: converges, stops at max_iter (loss_tol = 0 is never met by a positive loss)
        Dense b = problem(0.1, 1);
        const Run r = run(b, base);
        common(b, base, r);
        CHECK(r.res.stop == FIT_MAX_ITER && r.res.iters == 12 && r.acc[0] == 1);
        CHECK(r.loss.back() <= 1e-20 * r.loss[0]);
        seen[r.res.stop] = true;
    }
    {   // a random start, a strict budget: accepted and rejected steps both occur somewhere along twenty iterations
        ttx_fit_opts o = base;
        o.max_iter = 20; o.lambda0 = 1e-6; o.cg_max = 40; o.cg_tol = 1e-2; o.max_reject = 20;
        Dense b = problem(-1.0, 2);
        const Run r = run(b, o);
        common(b, o, r);
        CHECK(r.loss.back() < r.loss[0]);
        seen[r.res.stop] = true;
    }
    {   // loss_tol: at entry, and after an accepted step
        ttx_fit_opts o = base;
        o.loss_tol = 1e300;
        Dense b = problem(0.1, 3);
        Run r = run(b, o);
        common(b, o, r);
        CHECK(r.res.stop == FIT_LOSS_TOL && r.res.iters == 0 && b.n_cg == 0 && r.lambda[0] == o.lambda0);
        Dense b2 = problem(0.1, 3);
        double l0 = 0.0;
        b2.loss(&l0);
        o.loss_tol = 1e-3 * l0;
        r = run(b2, o);
        common(b2, o, r);
        CHECK(r.res.stop == FIT_LOSS_TOL && r.res.iters >= 1 && r.res.iters < 12 && r.loss[r.res.iters] <= o.loss_tol && r.loss[r.res.iters - 1] > o.loss_tol);
        seen[r.res.stop] = true;
    }
    {   // a zero gradient at entry with a loss that is not zero: two zero cores
        Dense b = problem(0.1, 4);
        for (size_t e = b.off[0]; e < b.off[1]; e++) b.theta[e] = 0.0;
        for (size_t e = b.off[2]; e < b.off[3]; e++) b.theta[e] = 0.0;
        const std::vector<double> before = b.theta;
        const Run r = run(b, base);
        common(b, base, r);
        CHECK(r.res.stop == FIT_ZERO_GRADIENT && r.res.iters == 0 && r.loss[0] > 0.0 && b.n_cg == 1 && b.n_jvp == 0);
        CHECK(memcmp(before.data(), b.theta.data(), sizeof(double) * before.size()) == 0);
        seen[r.res.stop] = true;
    }
    {   // every trial rejected: max_reject consecutive rejections, lambda climbs by lambda_up each time, the parameters keep their bits
        ttx_fit_opts o = base;
        o.max_reject = 3;
        Dense b = problem(0.1, 5);
        b.hostile = 1;
        const std::vector<double> before = b.theta;
        const Run r = run(b, o);
        common(b, o, r);
        CHECK(r.res.stop == FIT_MAX_REJECT && r.res.iters == 3 && b.n_restore == 3 && b.n_cg == r.cg[0] + r.cg[1] + r.cg[2] + 1);     // the gradient is formed once
        CHECK(r.lambda[0] == 1e-2 && r.lambda[1] == 1e-2 * 4.0 && r.lambda[2] == (1e-2 * 4.0) * 4.0 && r.lambda[3] == ((1e-2 * 4.0) * 4.0) * 4.0);
        CHECK(memcmp(before.data(), b.theta.data(), sizeof(double) * before.size()) == 0);
        seen[r.res.stop] = true;
    }
    {   // a loss that is not finite at entry
        Dense b = problem(0.1, 6);
        b.y[7] = NAN;
        const std::vector<double> before = b.theta;
        const Run r = run(b, base);
        common(b, base, r);
        CHECK(r.res.stop == FIT_NONFINITE && r.res.iters == 0 && std::isnan(r.loss[0]) && b.n_cg == 0);
        CHECK(memcmp(before.data(), b.theta.data(), sizeof(double) * before.size()) == 0);
        seen[r.res.stop] = true;
    }
    {   // max_iter = 0 and null history pointers
        ttx_fit_opts o = base;
        o.max_iter = 0;
        Dense b = problem(0.1, 7);
        ttx_fit_result res = {-1, -1};
        CHECK(fit_run(b, o, FitHistory(), &res) == 0 && res.iters == 0 && res.stop == FIT_MAX_ITER);
        CHECK(fit_run(b, base, FitHistory(), nullptr) == 0);
    }
    for (int s = 1; s <= 5; s++) CHECK(seen[s]);
    // the options the engine refuses
    ttx_fit_opts o = base;
    CHECK(!fit_opts_problem(o));
    o = base; o.max_iter = -1; CHECK(fit_opts_problem(o));
    o = base; o.cg_max = 0; CHECK(fit_opts_problem(o));
    o = base; o.max_reject = 0; CHECK(fit_opts_problem(o));
    o = base; o.mode = 3; CHECK(fit_opts_problem(o));
    o = base; o.lambda0 = 0.0; CHECK(fit_opts_problem(o));
    o = base; o.lambda0 = INFINITY; CHECK(fit_opts_problem(o));
    o = base; o.lambda_down = 0.0; CHECK(fit_opts_problem(o));
    o = base; o.lambda_down = 1.5; CHECK(fit_opts_problem(o));
    o = base; o.lambda_up = 0.5; CHECK(fit_opts_problem(o));
    o = base; o.cg_tol = -1.0; CHECK(fit_opts_problem(o));
    o = base; o.loss_tol = NAN; CHECK(fit_opts_problem(o));
    printf("fit plan: ok\n");
    return 0;
}
