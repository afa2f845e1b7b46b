// ttx_algebra.h -- sums and elementwise products of resident tensor trains assembled on the device (ttx_lincomb / ttx_hadamard).
//
// Both results are block assemblies of the operands' cores; every element of a new core is a copy, a zero or one rounded product:
//   lincomb   sum_t coef(t) x_t (lib/tt.f90:928-946 for m terms, with 989-998): the first new core is the terms' first cores side by
//             side, each times its coef(t) (the only multiply); an interior core is block diagonal in term order with explicit
//             zeros off the blocks; the last core is the terms' last cores stacked
//   hadamard  Z(ib rx0 + ia, j, kb rx1 + ka) = X(ia, j, ka) Y(ib, j, kb): the x index runs fastest on both bonds
// Element (a, j, b) of a core lies at a + RM j + SS b (ttx_contract.h); every operand and the result have their own RM / SS.
// One launch per operation for all d cores, driven by a table of blocks (AlgBlk) uploaded in one copy; a workgroup finds its
// block by bisection over the blocks' first tiles.  Every element inside r'(k-1) x n(k) x r'(k) of every new core is written
// exactly once, zeros included: no memset pass, no atomics; the padding of the new storage is left alone and no padding of a
// source is read.  256 threads = ta lanes along a, the contiguous index, x 256 / ta columns.  A block whose addresses allow it
// (vec: bases on 16-byte boundaries, even leading dimensions, even row offset; hadamard: even rx0, so that a pair of rows shares
// its y value) moves two rows per lane in one 16-byte access; every other block goes row by row in 8-byte accesses.
#pragma once
#include <hip/hip_runtime.h>

typedef double dbl2 __attribute__((ext_vector_type(2)));

struct AlgBlk {
    const double *x, *y;            // lincomb: the term's core (y unused); hadamard: the two cores
    double *dst;                    // lincomb: row 0 of the first column of the term's band in the new core; hadamard: the new core
    double coef;                    // lincomb, first core: the term's coefficient
    long long first;                // first tile (workgroup) of this block
    size_t xSS, ySS;
    int xRM, yRM;
    int R0;                         // rows of the new core, r'(k-1)
    int ro, r0, n, r1;              // lincomb: rows ro .. ro + r0 - 1 of the band are the source's; hadamard: r0 = rx0, r1 = rx1
    int ry0, ry1;                   // hadamard
    int ta, vec;                    // lanes along a (a power of two <= 64); 16-byte accesses
    int scale, fill;                // lincomb: multiply by coef; write the zeros above and below the source's rows (not on the last core, where the terms share one column)
    int ntk;                        // hadamard: tiles along ka
};

#define TTX_ALG_U 4                 // lincomb: columns per thread
#define TTX_ALG_KC 8                // hadamard: x columns ka per tile

__device__ inline AlgBlk alg_find(const AlgBlk *blks, int nblk)
{
    int lo = 0, hi = nblk - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (blks[mid].first <= (long long)blockIdx.x) lo = mid; else hi = mid - 1; }
    return blks[lo];
}

// columns c = j + n b of the term's band, 256 / ta * TTX_ALG_U of them per workgroup
__global__ __launch_bounds__(256) void k_alg_lincomb(const AlgBlk *blks, int nblk, int RMd, size_t SSd)
{
    const AlgBlk B = alg_find(blks, nblk);
    const int tile = (int)((long long)blockIdx.x - B.first), al = (int)threadIdx.x & (B.ta - 1), cl = (int)threadIdx.x / B.ta, cpw = 256 / B.ta;
    const unsigned ncol = (unsigned)B.n * (unsigned)B.r1;
    const int lo = B.fill ? 0 : B.ro, hi = B.fill ? B.R0 : B.ro + B.r0, top = B.ro + B.r0;
    for (int u = 0; u < TTX_ALG_U; u++) {
        const unsigned c = ((unsigned)tile * TTX_ALG_U + u) * cpw + cl;
        if (c >= ncol) return;
        const unsigned b = c / (unsigned)B.n, j = c - b * (unsigned)B.n;
        const double *s = B.x + (size_t)B.xRM * j + B.xSS * b;
        double *d = B.dst + (size_t)RMd * j + SSd * b;
        if (B.vec) {                                                            // ro is even: a pair never straddles the block's first row
            for (int a = lo + 2 * al; a < hi; a += 2 * B.ta) {
                const bool e0 = a >= B.ro && a < top, e1 = a + 1 >= B.ro && a + 1 < top;
                dbl2 v = {0.0, 0.0};
                if (e0 && e1) v = *(const dbl2 *)(s + (a - B.ro));
                else if (e0) v.x = s[a - B.ro];
                if (B.scale) { v.x = B.coef * v.x; v.y = B.coef * v.y; }
                if (a + 1 < hi) *(dbl2 *)(d + a) = v; else d[a] = v.x;
            }
        } else {
            for (int a = lo + al; a < hi; a += B.ta) {
                double v = (a >= B.ro && a < top) ? s[a - B.ro] : 0.0;
                if (B.scale) v = B.coef * v;
                d[a] = v;
            }
        }
    }
}

// a workgroup takes 256 / ta pairs g = j + n kb and TTX_ALG_KC x columns ka: a thread keeps the y value of its rows in a register
// and streams the x column(s) X(ia, j, ka) past it
__global__ __launch_bounds__(256) void k_alg_hadamard(const AlgBlk *blks, int nblk, int RMd, size_t SSd)
{
    const AlgBlk B = alg_find(blks, nblk);
    const int tile = (int)((long long)blockIdx.x - B.first), tk = tile % B.ntk, tg = tile / B.ntk;
    const int al = (int)threadIdx.x & (B.ta - 1), cl = (int)threadIdx.x / B.ta, cpw = 256 / B.ta;
    const unsigned g = (unsigned)tg * cpw + cl;
    if (g >= (unsigned)B.n * (unsigned)B.ry1) return;
    const unsigned kb = g / (unsigned)B.n, j = g - kb * (unsigned)B.n;
    const int ka0 = tk * TTX_ALG_KC, ka1 = min(B.r1, ka0 + TTX_ALG_KC);
    const double *xp = B.x + (size_t)B.xRM * j, *yp = B.y + (size_t)B.yRM * j + B.ySS * kb;
    double *d = B.dst + (size_t)RMd * j + SSd * ((size_t)kb * B.r1);
    if (B.vec) {                                                                // rx0 is even: rows a, a + 1 share ib
        for (int a = 2 * al; a < B.R0; a += 2 * B.ta) {
            const int ib = a / B.r0, ia = a - ib * B.r0;
            const double yv = yp[ib];
#pragma unroll 4
            for (int ka = ka0; ka < ka1; ka++) {
                const dbl2 xv = *(const dbl2 *)(xp + ia + B.xSS * ka);
                dbl2 z; z.x = xv.x * yv; z.y = xv.y * yv;
                *(dbl2 *)(d + a + SSd * ka) = z;
            }
        }
    } else {
        for (int a = al; a < B.R0; a += B.ta) {
            const int ib = a / B.r0, ia = a - ib * B.r0;
            const double yv = yp[ib];
#pragma unroll 4
            for (int ka = ka0; ka < ka1; ka++) d[a + SSd * ka] = xp[ia + B.xSS * ka] * yv;
        }
    }
}
