// Stand-alone host program for ttcross_amd/csrc/ttx_cluster_rules.h (built and run by test_cluster_diet_cpu.py, plain and
// under -fsanitize=address,undefined): the integer key of the cluster kernel's wave maxima against < and == on doubles, and
// its slice bounds against floor(c n / NB).  Prints "<failures> <key comparisons> <slice tables> <other checks>".
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "ttx_cluster_rules.h"

static long bad = 0, ncmp = 0, ntab = 0, nchk = 0;
#define CHECK(c, ...) do { nchk++; if (!(c)) { if (bad++ < 10) { printf("line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static uint64_t bits(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }
static double from_bits(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
// a non-negative double that is no NaN: any bit pattern from +0.0 to +inf
static double rnd_nonneg() { return from_bits(rng() % 0x7ff0000000000001ull); }
// x with another low word (+inf stays: under its high word every other low word is a NaN)
static double with_low(double x, uint32_t lo) { return std::isinf(x) ? x : from_bits((bits(x) & 0xffffffff00000000ull) | lo); }

// the order the two integer maxima of the kernel impose on keys: the high word as a signed int, then the low word as an unsigned one
static bool cl_key_less(ClKey a, ClKey b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
static bool cl_key_eq(ClKey a, ClKey b) { return a.hi == b.hi && a.lo == b.lo; }

// the key orders and equates two values exactly as the doubles do, and gives back the double's bits
static void pair(double a, double b)
{
    const ClKey ka = cl_key(a), kb = cl_key(b);
    ncmp++;
    CHECK(cl_key_less(ka, kb) == (a < b), "less %a %a", a, b);
    CHECK(cl_key_less(kb, ka) == (b < a), "less %a %a", b, a);
    CHECK(cl_key_eq(ka, kb) == (a == b), "eq %a %a", a, b);
    CHECK(bits(cl_unkey(ka)) == bits(a) && bits(cl_unkey(kb)) == bits(b), "bits %a %a", a, b);
}

// the kernel's reduction over the lanes of a wave: the largest high word, then the largest low word among its holders
static double max_by_key(const double *x, int n)
{
    int hmax = cl_key(x[0]).hi;
    for (int l = 1; l < n; l++) { const int h = cl_key(x[l]).hi; if (h > hmax) hmax = h; }
    unsigned lmax = 0;
    for (int l = 0; l < n; l++) { const unsigned lo = cl_key_lo_at(cl_key(x[l]), hmax); if (lo > lmax) lmax = lo; }
    return cl_unkey(ClKey{hmax, lmax});
}

static void keys()
{
    const double lo_a = from_bits(0x3fe5555500000001ull), lo_b = from_bits(0x3fe55555fffffffeull);     // differ only in the low word
    const double hi_a = from_bits(0x3fe5555412345678ull), hi_b = from_bits(0x40e5555512345678ull);     // differ only in the high word
    const double special[] = {0.0, from_bits(1), lo_a, lo_b, hi_a, hi_b, 1.0, DBL_MAX, INFINITY, -1.0, DBL_MIN, from_bits(0x00000000ffffffffull),
                              from_bits(0x0000000100000000ull), from_bits(0x7fefffff00000000ull)};
    const int ns = (int)(sizeof special / sizeof special[0]);
    for (int a = 0; a < ns; a++)
        for (int b = 0; b < ns; b++) pair(special[a], special[b]);
    CHECK(cl_key(-1.0).hi < 0 && cl_key(0.0).hi == 0 && cl_key(0.0).lo == 0u, "the start value has the only negative high word");
    std::vector<double> x(1000000);
    for (size_t i = 0; i < x.size(); i++) x[i] = rnd_nonneg();
    for (size_t i = 0; i < x.size(); i++) {
        pair(x[i], x[(i + 1) % x.size()]);
        pair(x[i], special[i % ns]);
        // a neighbour in the same high word, and the same low word under another high word
        pair(x[i], with_low(x[i], (uint32_t)rng()));
        pair(x[i], from_bits((rng() % 0x7ff00000ull) << 32 | (uint32_t)bits(x[i])));
    }
    // waves of 64: the two integer maxima give the bits of the plain maximum; start values and ties among them
    for (size_t w = 0; w + 64 <= x.size(); w += 64) {
        double v[64];
        for (int l = 0; l < 64; l++) v[l] = x[w + l];
        const unsigned kind = (unsigned)(w / 64) % 4;
        if (kind == 1) for (int l = 0; l < 64; l += 3) v[l] = -1.0;                                   // lanes that own nothing
        if (kind == 2) for (int l = 1; l < 64; l++) v[l] = with_low(v[0], (uint32_t)bits(v[l]));   // one high word
        if (kind == 3) for (int l = 0; l < 64; l++) v[l] = (l % 5 == 0) ? v[0] : -1.0;                   // ties
        double m = v[0];
        for (int l = 1; l < 64; l++) m = (v[l] > m) ? v[l] : m;
        CHECK(bits(max_by_key(v, 64)) == bits(m), "wave %zu: %a vs %a", w / 64, max_by_key(v, 64), m);
    }
    double all_start[64];
    for (int l = 0; l < 64; l++) all_start[l] = -1.0;
    CHECK(bits(max_by_key(all_start, 64)) == bits(-1.0), "a wave of start values");
}

static void slices()
{
    for (int NB = 2; NB <= 16; NB++)
        for (int n = 1; n <= 200; n++) {
            ntab++;
            int covered = 0;
            for (int c = 0; c <= NB; c++) {
                const int s = cl_slice(c, n, NB);
                CHECK(s == (int)(((long long)c * n) / NB), "slice NB %d n %d c %d: %d", NB, n, c, s);
                if (c < NB) {
                    const int e = cl_slice(c + 1, n, NB);
                    CHECK(s == covered && e >= s && e <= n, "tiling NB %d n %d c %d: [%d, %d) after %d", NB, n, c, s, e, covered);
                    covered = e;
                }
            }
            CHECK(cl_slice(0, n, NB) == 0 && covered == n, "ends NB %d n %d: covered %d", NB, n, covered);
        }
    // waves at work: the larger of the two fiber slices in units of 64 elements, between 1 and the waves of a workgroup
    const int shapes[][4] = {{0, 0, 8, 8}, {1, 1, 1, 1}, {8, 0, 8, 8}, {8, 8, 8, 8}, {9, 2, 8, 8}, {2, 9, 8, 8}, {5, 5, 40, 40}, {4, 4, 64, 64}, {1, 0, 64, 1}, {3, 7, 21, 10}};
    for (const auto &s : shapes) {
        const int e = s[2] * s[0] > s[1] * s[3] ? s[2] * s[0] : s[1] * s[3];
        int w = (e + 63) / 64; w = w < 1 ? 1 : (w > 4 ? 4 : w);
        CHECK(cl_wact(s[0], s[1], s[2], s[3], 4) == w, "wact nj %d nk %d r0 %d r2 %d", s[0], s[1], s[2], s[3]);
    }
}

int main()
{
    keys();
    slices();
    printf("%ld %ld %ld %ld\n", bad, ncmp, ntab, nchk);
    return bad != 0;
}
