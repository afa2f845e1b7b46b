// ttx_cdf.h -- exact O(#binades) evaluation of the lottery's cumulative weights (host + device).
//
// lottery2 (reference lib/rnd.f90:116-119) builds pcol(i) = pcol(i-1) + |w_i|/sum(w) by SEQUENTIAL fp64
// accumulation and bisects it with find_d (lib/rnd.f90:128-143).  In dtt_dmrgg the weights are 1 except 0
// at the rows/columns that already hold a pivot (lib/dmrgg.f90:425-439), so the sequence over the K
// non-zero weights is a_k = fl(a_{k-1} + c), a_0 = 0, c = fl(1/K).  A serial K-step chain (K up to r*n =
// 6464) would sit on the critical path of every bond step, so it is evaluated in closed form per binade:
// inside one binade [2^e, 2^(e+1)) every a_k is a multiple of u = 2^(e-52) and fl(a + c) = a + delta with
// a CONSTANT delta once two additions have been made inside the binade (round-to-nearest-even: a tie
// c/u = q + 1/2 yields even multiples from the first in-binade addition on, after which the increment is
// the even one of q, q+1).  Real fp64 additions are made only for the <= 3 values after each binade
// crossing; the rest are arithmetic progressions.  tests/test_cdf.py checks this against the plain
// sequential loop for every K in 1..8192.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TTX_HD __host__ __device__ inline
#else
#define TTX_HD static inline
#endif

#define TTX_MAXSEG 128

struct ttx_cdfseg {
    double a0;     // a_{k0}
    double alast;  // a_{k0+cnt-1}
    double delta;  // a_{k0+t} = a0 + t*delta (exact), t in [0, cnt)
    int32_t k0;
    int32_t cnt;
};

TTX_HD uint64_t ttx_dbits(double x) { uint64_t b; memcpy(&b, &x, 8); return b; }
TTX_HD double ttx_bitsd(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }
TTX_HD int ttx_bexp(double x) { return (int)((ttx_dbits(x) >> 52) & 0x7ff); }  // biased exponent
// x / 2^(be-1075) as integer, x a positive normal multiple of ulp(be)
TTX_HD int64_t ttx_units(double x, int be)
{
    uint64_t b = ttx_dbits(x);
    int xe = (int)((b >> 52) & 0x7ff);
    int64_t mant = (int64_t)((b & 0xFFFFFFFFFFFFFULL) | (1ULL << 52));
    return (xe >= be) ? (mant << (xe - be)) : (mant >> (be - xe));
}
TTX_HD double ttx_from_units(int64_t v, int be)
{
    // v * 2^(be-1075), v < 2^54, result normal
    double d = (double)v;                        // exact for v < 2^53; v == 2^53 exact too
    uint64_t b = ttx_dbits(d);
    int de = (int)((b >> 52) & 0x7ff);           // biased exponent of (double)v : value = mant*2^(de-1075)
    b = (b & ~(0x7ffULL << 52)) | ((uint64_t)(de + be - 1075) << 52);
    return ttx_bitsd(b);
}

// floor(N / D) for 0 <= N < 2^54, 0 < D < 2^54 without 64-bit integer division (slow on the device): fp64
// quotient, then exact correction with integer multiplies
TTX_HD int64_t ttx_divfloor(int64_t N, int64_t D)
{
    int64_t q = (int64_t)((double)N / (double)D);
    while (q * D > N) q--;
    while ((q + 1) * D <= N) q++;
    return q;
}

// segments covering k = 1..K of a_k = fl(a_{k-1} + c), a_0 = 0, c = 1.0/K; returns their number
TTX_HD int ttx_cdf_build(int K, ttx_cdfseg *seg)
{
    if (K <= 0) return 0;
    const double c = 1.0 / (double)K;
    double a = 0.0, am1 = 0.0;                   // a_k, a_{k-1}
    int k = 0, ns = 0, inb = 0, lastexp = -1;
    while (k < K && ns < TTX_MAXSEG - 2) {
        double x = a + c;                        // the real sequential step
        k++;
        int xe = ttx_bexp(x);
        inb = (xe == lastexp) ? inb + 1 : 1;     // consecutive values inside binade xe
        lastexp = xe;
        seg[ns].a0 = x; seg[ns].alast = x; seg[ns].delta = 0.0; seg[ns].k0 = k; seg[ns].cnt = 1; ns++;
        am1 = a; a = x;
        if (inb >= 3 && k < K) {
            // a_{k-2}, a_{k-1}, a_k share the binade: the increment D = a_k - a_{k-1} is steady until 2^(e+1)
            int64_t Z = ttx_units(a, xe), D = Z - ttx_units(am1, xe);
            const int64_t B = (int64_t)1 << 53;  // 2^(e+1) in units of u = 2^(e-52)
            if (D > 0) {
                int64_t tmax = ttx_divfloor(B - Z - 1, D);  // number of t >= 1 with Z + t*D < B
                if (tmax > (int64_t)(K - k)) tmax = K - k;
                if (tmax > 0) {
                    seg[ns].a0 = ttx_from_units(Z + D, xe);
                    seg[ns].alast = ttx_from_units(Z + tmax * D, xe);
                    seg[ns].delta = ttx_from_units(D, xe);
                    seg[ns].k0 = k + 1; seg[ns].cnt = (int32_t)tmax; ns++;
                    am1 = ttx_from_units(Z + (tmax - 1) * D, xe);
                    a = ttx_from_units(Z + tmax * D, xe);
                    k += (int)tmax;
                }
            }
        }
    }
    return ns;
}

// largest k in [0, K] with a_k <= y  (binary search over the segments, then exact integer arithmetic)
TTX_HD int ttx_cdf_kmax(const ttx_cdfseg *seg, int ns, double y)
{
    int lo = -1, hi = ns;                         // last segment with a0 <= y
    while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (seg[mid].a0 <= y) lo = mid; else hi = mid; }
    if (lo < 0) return 0;
    const ttx_cdfseg sg = seg[lo];
    if (sg.cnt == 1 || y >= sg.alast) return sg.k0 + sg.cnt - 1;
    int be = ttx_bexp(sg.a0);
    int64_t A = ttx_units(y, be) - ttx_units(sg.a0, be);   // y in [a0, alast): same binade, exact
    int64_t D = ttx_units(sg.delta, be);
    return sg.k0 + (int)ttx_divfloor(A, D);
}

// 1-based position of the kth (1-based) non-zero weight, given the ascending distinct 1-based zero positions:
// kth + #{t : zeros[t] - t <= kth} (zeros[t] - t is non-decreasing, so the count is a binary search)
TTX_HD int ttx_select_nonzero(int kth, const int32_t *zeros, int nz)
{
    int lo = 0, hi = nz;                          // first t with zeros[t] - t > kth
    while (lo < hi) { int mid = (lo + hi) >> 1; if (zeros[mid] - mid <= kth) lo = mid + 1; else hi = mid; }
    return kth + lo;
}

// lottery index (1-based in 1..m) for uniform draw y: lib/rnd.f90:122-123 incl. the clamp to m
TTX_HD int ttx_lottery_index(const ttx_cdfseg *seg, int ns, int K, int m, const int32_t *zeros, int nz, double y)
{
    int kmax = ttx_cdf_kmax(seg, ns, y);
    if (kmax >= K) return m;
    return ttx_select_nonzero(kmax + 1, zeros, nz);
}

// Both lottery indices of one candidate: x = ttx_lottery_index(segx, ...), y = ttx_lottery_index(segy, ...), equal to the two
// calls for every input, but written as ONE dependent chain with as few instructions as the two could be made to share.  A
// lone wave pays an LDS round trip per step of a binary search and runs the integer code of ttx_units / ttx_divfloor at one
// instruction per issue slot; here
//   * the two searches advance together, every step tests x and y side by side, and no branch depends on a lane: a search is
//     a descent by powers of two over the count of leading entries that satisfy a monotone predicate (a0 <= draw for the
//     segments, zeros[t] - t <= kth for the zero list).  The first stride is the largest power of two not above the longer of
//     the two lists (at most SEGCAP / ZCAP, the capacities the caller guarantees: ns <= SEGCAP, nz <= ZCAP), so the trip
//     count is the same for x and y and for every lane that passes the same list lengths;
//   * the quotient inside a segment is taken in fp64 without the detour through integer units: with the draw d in [a0, alast)
//     of a segment, d, a0 and delta are multiples of the binade's ulp u, A = d - a0 is exact (same binade), and A / delta is
//     the same real number as ttx_cdf_kmax's N / D (N = A / u, D = delta / u).  floor(N / D) < 2^53 is a double and rounding
//     is monotone, so trunc(fl(A / delta)) is floor(N / D) or one more (never less: no upward step); the sign of A - q delta, which decides, is exact from
//     one fused multiply-add (a single rounding never changes the sign of a non-zero multiple of u >= 2^-1074).  Where
//     ttx_cdf_kmax does not divide, the operands are 0 / 1.
// A precondition ttx_lottery_index does not have: every list must be readable at index 0 even when it is empty (the value is
// then ignored), because the loads carry no test.  The LDS arrays of the cluster kernel are.
struct ttx_pair { int x, y; };
TTX_HD int ttx_pow2floor(int v) { return v > 0 ? 1 << (31 - __builtin_clz((unsigned)v)) : 0; }   // 0 for an empty list: no step
template <int SEGCAP, int ZCAP>
TTX_HD ttx_pair ttx_lottery_index2(const ttx_cdfseg *segx, int nsx, int Kx, int mx, const int32_t *zx, int nzx, double dx,
                                   const ttx_cdfseg *segy, int nsy, int Ky, int my, const int32_t *zy, int nzy, double dy)
{
    static_assert((SEGCAP & (SEGCAP - 1)) == 0 && (ZCAP & (ZCAP - 1)) == 0, "capacities are powers of two");
    // number of segments with a0 <= draw
    int px = 0, py = 0;
    const int nsm = nsx > nsy ? nsx : nsy;
    for (int st = nsm >= SEGCAP ? SEGCAP : ttx_pow2floor(nsm); st >= 1; st >>= 1) {
        const int tx = px + st, ty = py + st;
        const int ux = (tx <= nsx ? tx : nsx) - 1, uy = (ty <= nsy ? ty : nsy) - 1;
        const double ax = segx[ux > 0 ? ux : 0].a0, ay = segy[uy > 0 ? uy : 0].a0;
        px = (tx <= nsx && ax <= dx) ? tx : px;
        py = (ty <= nsy && ay <= dy) ? ty : py;
    }
    const ttx_cdfseg sx = segx[px > 0 ? px - 1 : 0], sy = segy[py > 0 ? py - 1 : 0];
    const bool vx = px > 0 && sx.cnt != 1 && dx < sx.alast, vy = py > 0 && sy.cnt != 1 && dy < sy.alast;   // divide
    const double Ax = vx ? dx - sx.a0 : 0.0, Ay = vy ? dy - sy.a0 : 0.0, Ex = vx ? sx.delta : 1.0, Ey = vy ? sy.delta : 1.0;
    int qx = (int)(Ax / Ex), qy = (int)(Ay / Ey);
    qx -= (__builtin_fma(-(double)qx, Ex, Ax) < 0.0); qy -= (__builtin_fma(-(double)qy, Ey, Ay) < 0.0);
    const int kx = vx ? sx.k0 + qx : (px > 0 ? sx.k0 + sx.cnt - 1 : 0);
    const int ky = vy ? sy.k0 + qy : (py > 0 ? sy.k0 + sy.cnt - 1 : 0);
    // position of non-zero weight number k + 1: k + 1 + #{t : zeros[t] - t <= k + 1}
    const int ex = kx + 1, ey = ky + 1;
    int cx = 0, cy = 0;
    const int nzm = nzx > nzy ? nzx : nzy;
    for (int st = nzm >= ZCAP ? ZCAP : ttx_pow2floor(nzm); st >= 1; st >>= 1) {
        const int tx = cx + st, ty = cy + st;
        const int ux = (tx <= nzx ? tx : nzx) - 1, uy = (ty <= nzy ? ty : nzy) - 1;
        const int wx = ux > 0 ? ux : 0, wy = uy > 0 ? uy : 0;
        const int fx = zx[wx] - wx, fy = zy[wy] - wy;
        cx = (tx <= nzx && fx <= ex) ? tx : cx;
        cy = (ty <= nzy && fy <= ey) ? ty : cy;
    }
    ttx_pair r;
    r.x = (kx >= Kx) ? mx : ex + cx;
    r.y = (ky >= Ky) ? my : ey + cy;
    return r;
}

// minstd power 48271^e mod (2^31-1)
TTX_HD uint64_t ttx_minstd_pow(uint64_t e)
{
    uint64_t base = 48271ULL, w = 1;
    // (mulmod31 is declared below; forward use is fine inside the header's single translation unit)
    while (e) {
        if (e & 1) { uint64_t x = w * base; x = (x & 2147483647ULL) + (x >> 31); x = (x & 2147483647ULL) + (x >> 31); w = (x >= 2147483647ULL) ? x - 2147483647ULL : x; }
        uint64_t y = base * base; y = (y & 2147483647ULL) + (y >> 31); y = (y & 2147483647ULL) + (y >> 31); base = (y >= 2147483647ULL) ? y - 2147483647ULL : y;
        e >>= 1;
    }
    return w;
}
// the double made from the generator word w1 = 48271^(2k+1) (and its successor), as ttx_flang_draw(k)
TTX_HD double ttx_flang_from_word(uint64_t w1)
{
    uint64_t x = w1 * 48271ULL; x = (x & 2147483647ULL) + (x >> 31); x = (x & 2147483647ULL) + (x >> 31);
    uint64_t w2 = (x >= 2147483647ULL) ? x - 2147483647ULL : x;
    uint64_t f = ((w1 << 30) | ((w2 - 1) & ((1ULL << 30) - 1))) >> 7;
    return (double)f * 5.5511151231257827e-17;
}

// flang run-time random_number (unseeded): minstd 48271 mod 2^31-1 from seed 1, two words per double
TTX_HD uint64_t ttx_mulmod31(uint64_t a, uint64_t b)
{   // (a*b) mod (2^31-1) for a,b < 2^31, by Mersenne folding (no 64-bit division on the device)
    uint64_t x = a * b;
    x = (x & 2147483647ULL) + (x >> 31);
    x = (x & 2147483647ULL) + (x >> 31);
    return (x >= 2147483647ULL) ? x - 2147483647ULL : x;
}
TTX_HD double ttx_flang_draw(uint64_t k)
{
    uint64_t e = 2 * k + 1, base = 48271ULL, w1 = 1;
    while (e) { if (e & 1) w1 = ttx_mulmod31(w1, base); base = ttx_mulmod31(base, base); e >>= 1; }
    uint64_t w2 = ttx_mulmod31(w1, 48271ULL);
    uint64_t f = ((w1 << 30) | ((w2 - 1) & ((1ULL << 30) - 1))) >> 7;   // 54 significant bits
    // (double)f * 2^-54 with round-to-nearest-even of the 54-bit integer, as ldexp((double)f, -54)
    return (double)f * 5.5511151231257827e-17;
}
