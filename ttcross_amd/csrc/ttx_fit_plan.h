// ttx_fit_plan.h -- the controller of ttx_basis_fit_batch / ttx_basis_fit_tab (host only, no HIP): a matrix-free Levenberg-Marquardt
// iteration on loss = 1/2 sum_p w_p (f(x_p) - y_p)^2 over all cores, written against a small backend so that the engine (device calls,
// ttx_engine.hip) and a CPU program with dense loops (tests/fit_plan_main.cpp) run the same lambda schedule, stop reasons, CG
// recurrences and bookkeeping.  Every scalar operation here is one double operation in the order written, which is what makes the
// exact mode restatable (tests/basis_jvp_ref.py: fit_numpy).
//
// The backend B owns five core-space vectors (FitVec), the point vectors and the parameters.  All calls return 0 or an error code:
//   loss(&l)            val = f(x_p) at the current parameters, res = val - y, c = w * res;  l = 0.5 * dot_n(c, res)
//   core_grad(0, dst)   dst = J^T c, c of the last loss();   core_grad(1, dst)   dst = J^T (w * q), q of the last jvp()
//   jvp(v)              q = J v
//   dot(a, b, &s)       the fixed-order dot product of two core-space vectors
//   axpby(al, x, be, y) y <- (al * x) + (be * y);   zero(v);   copy(dst, src)
//   snapshot()          keeps the parameters;   restore()   puts them back bit for bit;   apply(s)   parameters += 1.0 * s
// One iteration: the gradient g (kept across rejected steps: the parameters, and so its bits, have not changed); CG on
// (J^T W J + lambda I) s = -g from s = 0, left where p^T A p is not a positive finite number, after cg_max passes, or where
// |r|^2 <= (cg_tol * cg_tol) * |g|^2; then the trial step.  It is accepted where the trial loss is finite and strictly smaller
// (lambda *= lambda_down), otherwise the snapshot is restored (lambda *= lambda_up).  A loop that ended with s = 0 is a rejection.
// History: loss[0] is the loss at entry, loss[i + 1] the loss after iteration i (unchanged by a rejection); lambda[i] the lambda
// iteration i solved with; cg_iters[i] its J V products; accepted[i] 0 or 1.  Entries past the iterations that ran repeat the
// last loss and lambda, with cg_iters = accepted = 0, so every array is filled whatever the stop.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/ttx.h"      // ttx_fit_opts, ttx_fit_result, TTX_EVAL_*

enum FitVec { FIT_G, FIT_S, FIT_R, FIT_P, FIT_AP, FIT_NVEC };
enum FitStop { FIT_MAX_ITER = 1, FIT_LOSS_TOL = 2, FIT_ZERO_GRADIENT = 3, FIT_MAX_REJECT = 4, FIT_NONFINITE = 5 };
struct FitHistory { double *loss = nullptr, *lambda = nullptr; int32_t *cg_iters = nullptr, *accepted = nullptr; };     // max_iter + 1, then max_iter entries; each may be null

// what is wrong with the options, or null
inline const char *fit_opts_problem(const ttx_fit_opts &o)
{
    if (o.max_iter < 0) return "max_iter < 0";
    if (o.cg_max < 1) return "cg_max < 1";
    if (o.max_reject < 1) return "max_reject < 1";
    if (o.mode != TTX_EVAL_EXACT && o.mode != TTX_EVAL_MFMA && o.mode != TTX_EVAL_AUTO) return "unknown mode";
    if (!(o.lambda0 > 0.0) || !isfinite(o.lambda0)) return "lambda0 is not a positive finite number";
    if (!(o.lambda_down > 0.0) || !(o.lambda_down <= 1.0)) return "lambda_down outside (0, 1]";
    if (!(o.lambda_up >= 1.0) || !isfinite(o.lambda_up)) return "lambda_up is not a finite number >= 1";
    if (!(o.cg_tol >= 0.0) || !isfinite(o.cg_tol)) return "cg_tol is not a finite number >= 0";
    if (!(o.loss_tol >= 0.0) || !isfinite(o.loss_tol)) return "loss_tol is not a finite number >= 0";
    return nullptr;
}

template <class B> int fit_run(B &b, const ttx_fit_opts &o, const FitHistory &hist, ttx_fit_result *res)
{
    int rc, it = 0, stop = FIT_MAX_ITER, rejects = 0;
    double lambda = o.lambda0, cur = 0.0, rho0 = 0.0;
    bool have_g = false;
    if ((rc = b.loss(&cur))) return rc;
    if (hist.loss) hist.loss[0] = cur;
    if (!isfinite(cur)) stop = FIT_NONFINITE;
    else if (cur <= o.loss_tol) stop = FIT_LOSS_TOL;
    else
        while (it < o.max_iter) {
            if (!have_g) {
                if ((rc = b.core_grad(0, FIT_G)) || (rc = b.dot(FIT_G, FIT_G, &rho0))) return rc;
                have_g = true;
                if (rho0 == 0.0) { stop = FIT_ZERO_GRADIENT; break; }
            }
            const double lam = lambda;
            // CG on (J^T W J + lam I) s = -g
            if ((rc = b.zero(FIT_S)) || (rc = b.zero(FIT_R)) || (rc = b.axpby(-1.0, FIT_G, 1.0, FIT_R)) || (rc = b.copy(FIT_P, FIT_R))) return rc;
            double rho = rho0;
            int passes = 0, updates = 0;
            for (int k = 0; k < o.cg_max; k++) {
                double pAp = 0.0, rho_new = 0.0;
                if ((rc = b.jvp(FIT_P))) return rc;
                passes++;
                if ((rc = b.core_grad(1, FIT_AP)) || (rc = b.axpby(lam, FIT_P, 1.0, FIT_AP)) || (rc = b.dot(FIT_P, FIT_AP, &pAp))) return rc;
                if (!(pAp > 0.0) || !isfinite(pAp)) break;
                const double alpha = rho / pAp;
                if ((rc = b.axpby(alpha, FIT_P, 1.0, FIT_S))) return rc;
                updates++;
                if ((rc = b.axpby(-alpha, FIT_AP, 1.0, FIT_R)) || (rc = b.dot(FIT_R, FIT_R, &rho_new))) return rc;
                if (rho_new <= (o.cg_tol * o.cg_tol) * rho0) break;
                if ((rc = b.axpby(1.0, FIT_R, rho_new / rho, FIT_P))) return rc;
                rho = rho_new;
            }
            bool accepted = false;
            if (updates > 0) {
                double trial = 0.0;
                if ((rc = b.snapshot()) || (rc = b.apply(FIT_S)) || (rc = b.loss(&trial))) return rc;
                if (isfinite(trial) && trial < cur) { accepted = true; cur = trial; }
                else if ((rc = b.restore())) return rc;
            }
            if (accepted) { lambda = lambda * o.lambda_down; rejects = 0; have_g = false; }
            else { lambda = lambda * o.lambda_up; rejects++; }
            if (hist.lambda) hist.lambda[it] = lam;
            if (hist.cg_iters) hist.cg_iters[it] = passes;
            if (hist.accepted) hist.accepted[it] = accepted ? 1 : 0;
            if (hist.loss) hist.loss[it + 1] = cur;
            it++;
            if (accepted && cur <= o.loss_tol) { stop = FIT_LOSS_TOL; break; }
            if (rejects >= o.max_reject) { stop = FIT_MAX_REJECT; break; }
        }
    for (int k = it; k < o.max_iter; k++) {
        if (hist.loss) hist.loss[k + 1] = cur;
        if (hist.lambda) hist.lambda[k] = lambda;
        if (hist.cg_iters) hist.cg_iters[k] = 0;
        if (hist.accepted) hist.accepted[k] = 0;
    }
    if (res) { res->iters = it; res->stop = stop; }
    return 0;
}
