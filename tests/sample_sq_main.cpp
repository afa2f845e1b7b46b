// The host-side part of ttx_sample_sq.h as a program of its own (also built with the address and undefined-behaviour sanitizers by
// tests/test_sample_sq_cpu.py): the plan of the factor rows and table offsets, the weight check and the effective weights, on random
// shapes against their definitions.  Prints "bad plans checks" on its last line.
#include <cstdio>
#include <cstdint>
#include <random>
#include "ttx_sample_sq.h"

int main()
{
    std::mt19937_64 rng(20221);
    long long bad = 0, plans = 0, checks = 0;
    for (int it = 0; it < 4000; it++) {
        const int d = 1 + (int)(rng() % 12);
        std::vector<int> n(d), r(d + 1, 1), fx(d, 0);
        for (int k = 0; k < d; k++) { n[k] = 1 + (int)(rng() % (it % 7 == 0 ? 1100 : 9)); if (rng() % 4 == 0) fx[k] = 1 + (int)(rng() % n[k]); }
        for (int k = 1; k < d; k++) r[k] = 1 + (int)(rng() % 128);
        SqPlan P;
        sq_plan(d, n.data(), r.data(), fx.data(), P);
        plans++;
        double fl = 0.0;
        size_t ho = 0, fo = 0, wo = 0;
        int rmax = 1, nmax = 1;
        for (int k = 0; k <= d; k++) {
            bad += P.hoff[k] != ho || P.foff[k] != fo || P.woff[k] != wo; checks += 3;
            bad += P.l[k] < 1 || P.l[k] > r[k] || (k == 0 && P.l[k] != 1); checks++;
            rmax = r[k] > rmax ? r[k] : rmax;
            if (k == d) break;
            const long long ln = (long long)P.l[k] * n[k];
            bad += P.l[k + 1] != (int)(ln < r[k + 1] ? ln : r[k + 1]); checks++;
            ho += (size_t)P.l[k] * n[k] * ((r[k + 1] + 3) / 4 * 4); fo += (size_t)P.l[k] * r[k]; wo += n[k];
            if (!fx[k]) fl += 2.0 * n[k] * P.l[k] * r[k + 1];
            nmax = n[k] > nmax ? n[k] : nmax;
        }
        bad += P.flops != fl || P.rmax != rmax || P.nmax != nmax; checks += 3;
        // weights: the check, then the effective weights and the products of the sums
        std::vector<double> w(wo);
        for (auto &v : w) v = (double)(rng() % 1000) / 64.0;
        bad += sq_bad_weight(w.data(), w.size()) != -1; checks++;
        if (!w.empty()) {
            static const double evil[] = {-1e-300, -1.0, -0.0 - 1.0, NAN, INFINITY, -INFINITY};
            const size_t j = rng() % w.size();
            const double keep = w[j];
            for (double e : evil) { w[j] = e; bad += sq_bad_weight(w.data(), w.size()) != (long long)j; checks++; }
            w[j] = -0.0; bad += sq_bad_weight(w.data(), w.size()) != -1; checks++;      // -0.0 is a zero
            w[j] = keep;
        }
        const double gamma = (double)(rng() % 5) * 0.25;
        for (int pass = 0; pass < 2; pass++) {
            std::vector<double> eff, gw;
            sq_effective(d, n.data(), fx.data(), pass ? nullptr : w.data(), gamma, eff, gw);
            bad += eff.size() != wo || gw.size() != (size_t)d + 1 || gw[0] != gamma; checks += 3;
            size_t o = 0;
            double g = gamma;
            for (int k = 0; k < d; k++) {
                double W = 0.0;
                for (int i = 0; i < n[k]; i++) {
                    const double want = fx[k] ? (i == fx[k] - 1 ? 1.0 : 0.0) : (pass ? 1.0 : w[o + i]);
                    bad += eff[o + i] != want; checks++;
                    W = W + want;
                }
                g = g * (fx[k] ? 1.0 : W);
                bad += gw[k + 1] != g; checks++;
                o += n[k];
            }
        }
    }
    printf("%lld %lld %lld\n", bad, plans, checks);
    return bad ? 1 : 0;
}
