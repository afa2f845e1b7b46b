"""ttx_lottery_index2 (ttx_cdf.h: both lottery indices of a candidate as one dependent chain, used by the cluster sweep
kernel) against two calls of ttx_lottery_index, as a stand-alone host program.

For every K in 1..4096 (x side; the y side takes an unrelated K' so that the two searches need different step counts):
  * draws at, just below and just above a_k for up to CAP values of k per K (the first and last ones, a stride in between,
    and every k at which a segment starts or ends), plus 0 and the largest double below 1;
  * zero lists that are empty, a single entry, dense at the front, dense at the back, spread, and at the list capacity;
  * x and y take their draw and their list shape independently of each other.
Both capacities in use are instantiated: <64, 64> (the cluster kernel: TTX_TABSEG segments, RM <= 64 pivots) and
<128, 128> (TTX_MAXSEG, the size of the kernels' list arrays).  The same program runs once more under
-fsanitize=address,undefined: the lists are heap blocks of exactly their length (one element for an empty list, which
the function may read and must ignore: it holds INT_MAX), so a read past a list is reported."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cmath>
#include <vector>
#include "%s/ttcross_amd/csrc/ttx_cdf.h"

static const int CAP = 40;            // values of k per K around which draws are placed
static uint64_t rs = 88172645463325252ULL;
static uint32_t rnd() { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 16); }

struct Side {
    int K = 0, ns = 0;
    ttx_cdfseg *seg = nullptr;                 // exactly ns segments
    std::vector<double> draws;
    void build(int K_) {
        static ttx_cdfseg tmp[TTX_MAXSEG];
        K = K_; ns = ttx_cdf_build(K, tmp);
        free(seg); seg = (ttx_cdfseg *)malloc(sizeof(ttx_cdfseg) * ns);
        for (int s = 0; s < ns; s++) seg[s] = tmp[s];
        std::vector<double> a(K + 1); double c = 1.0 / K, x = 0; a[0] = 0;
        for (int k = 1; k <= K; k++) { x = x + c; a[k] = x; }
        std::vector<int> ks;
        for (int k = 0; k <= K && k < CAP / 4; k++) ks.push_back(k);
        for (int k = K; k >= 0 && k > K - CAP / 4; k--) ks.push_back(k);
        for (int t = 1; t < CAP / 2; t++) ks.push_back((int)((long long)K * t / (CAP / 2)));
        for (int s = 0; s < ns; s++) { ks.push_back(seg[s].k0); ks.push_back(seg[s].k0 + seg[s].cnt - 1); }
        draws.clear();
        draws.push_back(0.0); draws.push_back(nextafter(1.0, 0.0));
        for (int k : ks) {
            const double v[3] = {a[k], nextafter(a[k], 0.0), nextafter(a[k], 2.0)};
            for (double y : v) { if (y < 0) y = 0; if (y >= 1) y = nextafter(1.0, 0.0); draws.push_back(y); }
        }
    }
};

// zero list of shape sh for K non-zero weights: nz ascending distinct positions in 1..K+nz, a heap block of exactly max(nz, 1) ints
static int32_t *zlist(int sh, int K, int zcap, int *nz_)
{
    int nz = sh == 0 ? 0 : sh == 1 ? 1 : sh == 5 ? zcap : 1 + (int)(rnd() %% (unsigned)(zcap - 1));
    const int m = K + nz;
    int32_t *z = (int32_t *)malloc(sizeof(int32_t) * (nz ? nz : 1));   // an empty list is readable at index 0
    z[0] = 0x7fffffff;
    if (sh == 1) z[0] = 1 + (int)(rnd() %% (unsigned)m);
    else if (sh == 2) for (int t = 0; t < nz; t++) z[t] = t + 1;                 // dense at the front
    else if (sh == 3) for (int t = 0; t < nz; t++) z[t] = m - nz + 1 + t;        // dense at the back
    else if (nz) {                                                                // spread: every position equally likely
        int t = 0;
        for (int pos = 1; pos <= m && t < nz; pos++) if (rnd() %% (unsigned)(m - pos + 1) < (unsigned)(nz - t)) z[t++] = pos;
    }
    *nz_ = nz;
    return z;
}

template <int SEGCAP, int ZCAP>
static long run(int klo, int khi, long *ncmp, int *steps_differ)
{
    long bad = 0;
    Side X, Y;
    for (int K = klo; K <= khi; K++) {
        X.build(K); Y.build(1 + (int)(rnd() %% 4096u));
        if (X.ns > SEGCAP || Y.ns > SEGCAP) { printf("K=%%d or %%d needs more than %%d segments\n", X.K, Y.K, SEGCAP); return -1; }
        for (int shx = 0; shx < 6; shx++) {
            int nzx, nzy;
            int32_t *zx = zlist(shx, X.K, ZCAP, &nzx), *zy = zlist((int)(rnd() %% 6u), Y.K, ZCAP, &nzy);
            if (X.ns != Y.ns || nzx != nzy) (*steps_differ)++;
            const int mx = X.K + nzx, my = Y.K + nzy;
            for (size_t a = 0; a < X.draws.size(); a++) {
                const double dx = X.draws[a], dy = Y.draws[rnd() %% Y.draws.size()];
                const int wx = ttx_lottery_index(X.seg, X.ns, X.K, mx, zx, nzx, dx);
                const int wy = ttx_lottery_index(Y.seg, Y.ns, Y.K, my, zy, nzy, dy);
                const ttx_pair g = ttx_lottery_index2<SEGCAP, ZCAP>(X.seg, X.ns, X.K, mx, zx, nzx, dx, Y.seg, Y.ns, Y.K, my, zy, nzy, dy);
                // and with the sides exchanged: y takes the systematic draws
                const ttx_pair h = ttx_lottery_index2<SEGCAP, ZCAP>(Y.seg, Y.ns, Y.K, my, zy, nzy, dy, X.seg, X.ns, X.K, mx, zx, nzx, dx);
                (*ncmp)++;
                if (g.x != wx || g.y != wy || h.x != wy || h.y != wx) {
                    if (bad++ < 5) printf("K=%%d/%%d nz=%%d/%%d dx=%%a dy=%%a: want %%d %%d, pair %%d %%d, exchanged %%d %%d\n", X.K, Y.K, nzx, nzy, dx, dy, wx, wy, g.x, g.y, h.y, h.x);
                }
            }
            free(zx); free(zy);
        }
    }
    free(X.seg); free(Y.seg);
    return bad;
}

int main(int argc, char **argv)
{
    const int klo = argc > 2 ? atoi(argv[1]) : 1, khi = argc > 2 ? atoi(argv[2]) : 4096;
    long ncmp = 0; int differ = 0;
    const long b1 = run<64, 64>(klo, khi, &ncmp, &differ);
    const long b2 = run<128, 128>(klo, khi, &ncmp, &differ);
    printf("%%ld %%ld %%ld %%d\n", b1, b2, ncmp, differ);
    return (b1 != 0 || b2 != 0);
}
'''


def _build(tmp_path, name, extra):
    src = tmp_path / "pair.cpp"
    src.write_text(SRC % ROOT)
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, str(src), "-o", str(exe)], check=True)
    return exe


def _check(out, kcount):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    b1, b2, ncmp, differ = (int(x) for x in out.stdout.strip().splitlines()[-1].split())
    assert b1 == 0 and b2 == 0
    assert ncmp >= 2 * 6 * 60 * kcount, "every K meets six list shapes and at least 60 draws per capacity"
    assert differ > kcount, "x and y must meet lists of different lengths"


def test_pair_equals_two_single_calls(tmp_path):
    exe = _build(tmp_path, "pair", [])
    _check(subprocess.run([str(exe)], capture_output=True, text=True), 4096)


def test_pair_under_address_and_undefined_sanitizers(tmp_path):
    """The same program as a stand-alone host binary with -fsanitize=address,undefined (every K again: out-of-range shift
    counts and reads past a list depend on the segment tables)."""
    exe = _build(tmp_path, "pair_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    _check(subprocess.run([str(exe)], capture_output=True, text=True, env=env), 4096)
