// Stand-alone host program for the two rules of ttcross_amd/csrc/ttx_bondstep.h that the end of a sweep runs on (built and run by
// test_sweep_tail_cpu.py, plain and under -fsanitize=address,undefined): stop_rule against a plain restatement of the reference's
// lines over generated runs, boundary_neval against the conditions of k_exch_boundary's corner blocks.
// Prints "<failures> <runs compared> <sweeps compared> <boundary cases>".
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>
#include "ttx_bondstep.h"

static long bad = 0, nrun = 0, nsweep = 0, nbnd = 0;
#define CHECK(c, ...) do { if (!(c)) { if (bad++ < 10) { printf("line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// lib/dmrgg.f90:1011-1019 as the sweep loop has it: a counter that lives across the sweeps of one run
struct Plain {
    int strike = 0;
    bool sweep(int it, int maxrank, double accuracy, double pmax, double amax)
    {
        bool ready = false;
        if (it + 1 >= maxrank) ready = true;
        if (accuracy >= 0.0) {
            if (pmax <= accuracy * amax) strike = strike + 1;
            else strike = 0;
            if (strike >= 3) ready = true;
        }
        return ready;
    }
};

// one run: sweep it = 1, 2, ... takes entry (it - 1) % len of the pattern; kind 0: pivot above the bound, 1: at or below it (equality
// included), 2: pmax a NaN, 3: amax a NaN.  Runs until either side says ready (they must say so in the same sweep) or `cap` sweeps.
static void run(const std::vector<int> &pat, int maxrank, double accuracy, int cap)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    Plain ref;
    int strikes = 0;
    nrun++;
    for (int it = 1; it <= cap; it++) {
        const int kind = pat[(it - 1) % pat.size()];
        const double amax = (kind == 3) ? nan : 4.0 + it;
        const double bound = fabs(accuracy) * (4.0 + it);
        const double pmax = (kind == 2) ? nan : (kind == 0) ? bound * 1.5 + 1e-300 : (it % 2 ? bound : bound * 0.25);
        const bool want = ref.sweep(it, maxrank, accuracy, pmax, amax);
        const StopRule s = stop_rule(it, maxrank, accuracy, pmax, amax, strikes);
        nsweep++;
        CHECK((s.ready != 0) == want, "ready %d vs %d at sweep %d (maxrank %d accuracy %g)", s.ready, (int)want, it, maxrank, accuracy);
        CHECK(accuracy < 0.0 ? s.strikes == strikes : s.strikes == ref.strike, "strikes %d vs %d at sweep %d", s.strikes, ref.strike, it);
        CHECK(s.ready == 0 || s.ready == 1, "ready is %d", s.ready);
        if ((kind == 2 || kind == 3) && accuracy >= 0.0) CHECK(s.strikes == 0, "a NaN sweep must reset the strikes (got %d)", s.strikes);
        if (it + 1 == maxrank) CHECK(s.ready == 1, "the rank limit must end the run at sweep %d", it);
        strikes = s.strikes;
        if (want || s.ready) break;
    }
}

// k_exch_boundary's corner blocks of one group, as launched behind k_exch_max_apply (which has copied the neighbours' flags u_r /
// u_l into upd[last + 1] / upd[first - 1]): 2 NM blocks, each adds under its own conditions
static long long corner_blocks(int NM, bool has_r, int u_r, int upd_last, int n_r, bool has_l, int u_l, int upd_first, int n_l)
{
    long long neval = 0;
    const int upd_br = u_r, upd_bl = u_l;
    for (int bx = 0; bx < 2 * NM; bx++) {
        if (bx < NM) {
            const int k = bx;
            if (!has_r || !upd_br || k >= n_r) continue;
            if (upd_last) { if (k == 0) neval += n_r; }
        } else {
            const int j = bx - NM;
            if (!has_l || !upd_bl || j >= n_l) continue;
            if (upd_first) { if (j == 0) neval += n_l; }
        }
    }
    return neval;
}

int main()
{
    // every pattern of length 1..6 over the four kinds, at four accuracies and rank limits around the pattern's length
    for (int len = 1; len <= 6; len++) {
        int total = 1;
        for (int k = 0; k < len; k++) total *= 4;
        for (int code = 0; code < total; code++) {
            std::vector<int> pat(len);
            for (int k = 0, c = code; k < len; k++, c /= 4) pat[k] = c % 4;
            for (double acc : {-1.0, 0.0, 1e-3, 0.5})
                for (int maxrank : {2, 3, 5, 9, 40}) run(pat, maxrank, acc, 48);
        }
    }
    for (int NM : {1, 2, 9})
        for (int bits = 0; bits < 64; bits++)
            for (int n_r : {1, 2, 9})
                for (int n_l : {1, 3, 9}) {
                    if (n_r > NM || n_l > NM) continue;
                    const bool has_r = bits & 1, has_l = bits & 8;
                    const int u_r = (bits >> 1) & 1, upd_last = (bits >> 2) & 1, u_l = (bits >> 4) & 1, upd_first = (bits >> 5) & 1;
                    nbnd++;
                    const long long want = corner_blocks(NM, has_r, u_r, upd_last, n_r, has_l, u_l, upd_first, n_l);
                    const long long got = boundary_neval(has_r, u_r, upd_last, n_r, has_l, u_l, upd_first, n_l);
                    CHECK(got == want, "boundary_neval %lld vs %lld (bits %d, n %d %d)", got, want, bits, n_r, n_l);
                }
    printf("%ld %ld %ld %ld\n", bad, nrun, nsweep, nbnd);
    return bad ? 1 : 0;
}
