// ttx_cluster_rules.h -- the rules of the cluster sweep kernel (ttx_cluster.h) that a host program can check: the slice of
// the mode index a workgroup owns and the integer key under which the kernel takes wave maxima of its non-negative doubles
// (tests/cluster_diet_main.cpp), and the batched form of its ordered residual sums (tests/cluster_resid_main.cpp).
#pragma once
#include "ttx_cdf.h"     // TTX_HD, ttx_dbits, ttx_bitsd

// Workgroup c of NB owns the mode indices [cl_slice(c, n, NB), cl_slice(c + 1, n, NB)) of a mode of size n: floor(c n / NB).
// c <= NB <= 16 and n <= NM, so the product fits 32 bits (a 64-bit division is a long per-lane instruction sequence).
TTX_HD int cl_slice(int c, int n, int NB) { return (int)((unsigned)c * (unsigned)n / (unsigned)NB); }

// Waves of a workgroup that own fiber elements of a bond step, from the widths nj, nk of its two slices: the largest fiber
// slice in units of 64 elements, at least wave 0, at most nw waves.
TTX_HD int cl_wact(int nj, int nk, int r0, int r2, int nw)
{
    const int a = r0 * nj, b = nk * r2, e = a > b ? a : b, w = (e + 63) >> 6;
    return w < 1 ? 1 : (w > nw ? nw : w);
}

// The key of a double that is >= +0.0 (+inf included) or the start value -1.0, never -0.0 and never a NaN: its high word
// as a SIGNED int, then its low word as an unsigned one.  Among such values the pair orders exactly like the double:
// a non-negative double's bit pattern grows with its value and its high word is >= 0, -1.0 has the only negative high
// word (0xbff00000), and equal keys are equal bit patterns.  A maximum over a wave is then two integer trees of one
// DPP instruction per step (the high words, then the low words of the lanes that hold the largest high word) instead
// of one tree of six instructions per step on register pairs.
struct ClKey { int hi; unsigned lo; };
TTX_HD ClKey cl_key(double x) { const uint64_t b = ttx_dbits(x); return ClKey{(int)(uint32_t)(b >> 32), (unsigned)b}; }
TTX_HD double cl_unkey(ClKey k) { return ttx_bitsd(((uint64_t)(uint32_t)k.hi << 32) | k.lo); }
// the low word a lane puts into the second tree once the largest high word hmax of the wave is known
TTX_HD unsigned cl_key_lo_at(ClKey k, int hmax) { return k.hi == hmax ? k.lo : 0u; }

// The ordered sum of a lane's residual: tm(s, ld()) for s = 0 .. n-1 in ASCENDING s, each exactly once and none for s >= n, so a
// functor that accumulates performs the operations of the plain loop in its order (no padding term: a 0 * inf or a -0 would
// change bits).  ld() returns the memory operand(s) of the next term and steps its own running address; tm() adds the term.
// The plain loop around a lane read (a convergent operation) with a run-time trip count is not unrolled by the compiler, and
// every trip then waits for its own load: n DEPENDENT round trips to the L2.  Here the loads of a piece are all issued before
// its first add, and every loop has a constant trip count: whole batches of B terms while they last, then pieces of B/2 .. 1
// chosen by the bits of the wave-uniform remainder -- at most log2(B) further round trips and never a load that is not used.
// n must be wave-uniform where tm() reads lanes.
#if defined(__clang__)      // (the host check is built by a compiler that does not know the pragma)
#define CL_UNROLL _Pragma("unroll")
#define CL_NO_UNROLL _Pragma("unroll 1")
#else
#define CL_UNROLL
#define CL_NO_UNROLL
#endif
template <int N, class LD, class TM>
TTX_HD void cl_sum_piece(int s0, LD &ld, TM &tm)
{
    decltype(ld()) v[N];
    CL_UNROLL
    for (int k = 0; k < N; k++) v[k] = ld();
    CL_UNROLL
    for (int k = 0; k < N; k++) tm(s0 + k, v[k]);
}
template <int B, class LD, class TM>
TTX_HD void cl_ordered_sum(int n, LD ld, TM tm)
{
    static_assert(B == 16 || B == 8, "batches of 16 or 8 terms");
    int s = 0;
    CL_NO_UNROLL
    for (; s + B <= n; s += B) cl_sum_piece<B>(s, ld, tm);
    const int rem = n - s;
    if constexpr (B > 8) if (rem & 8) { cl_sum_piece<8>(s, ld, tm); s += 8; }
    if (rem & 4) { cl_sum_piece<4>(s, ld, tm); s += 4; }
    if (rem & 2) { cl_sum_piece<2>(s, ld, tm); s += 2; }
    if (rem & 1) cl_sum_piece<1>(s, ld, tm);
}

// ---- what the kernel carries from launch to launch instead of recomputing it at its entry (tests/cluster_entry_main.cpp) ----
// Powers of the lottery's generator, 48271^e mod (2^31 - 1): ttx_minstd_pow's rule (ttx_cdf.h) as a constant expression, and the
// table of 48271^(2 t), t = 0 .. CL_POWTAB_N - 1, made from it by the compiler.  Thread t's first lottery candidate jumps by entry
// t, lane l keeps entry l for the generator step of a bond step, and entry 64 is 48271^128, the factor of cl_stepmul.
#define CL_POWTAB_N 256
constexpr uint64_t cl_mulmod31_c(uint64_t a, uint64_t b)
{
    uint64_t x = a * b;
    x = (x & 2147483647ULL) + (x >> 31);
    x = (x & 2147483647ULL) + (x >> 31);
    return (x >= 2147483647ULL) ? x - 2147483647ULL : x;
}
constexpr uint64_t cl_minstd_pow_c(uint64_t e)
{
    uint64_t base = 48271ULL, w = 1;
    while (e) { if (e & 1) w = cl_mulmod31_c(w, base); base = cl_mulmod31_c(base, base); e >>= 1; }
    return w;
}
struct ClPowTab { uint32_t v[CL_POWTAB_N]; };
constexpr ClPowTab cl_make_powtab()
{
    ClPowTab t{};
    for (int k = 0; k < CL_POWTAB_N; k++) t.v[k] = (uint32_t)cl_minstd_pow_c(2ULL * (uint64_t)k);
    return t;
}

// The generator step of a bond step, 48271^(2 nlot): below 512 candidates from lane(b) = 48271^(2 b), b < 64, and
// c64 = 48271^128 as 48271^(2 (64 a + b)) = 48271^(2 b) * (48271^128)^a -- one lookup and a <= 7 products (the same residue:
// modular products are exact); the square-and-multiply loop from there on.
template <class LANE>
TTX_HD uint64_t cl_stepmul(int nlot, LANE lane, uint64_t c64)
{
    if (nlot >= 512) return ttx_minstd_pow(2ull * (uint64_t)nlot);
    uint64_t s = lane(nlot & 63);
    for (int a = 0; a < (nlot >> 6); a++) s = ttx_mulmod31(s, c64);
    return s;
}

// The generator word 48271^(2 rngpos + 1) a launch leaves next to the position it belongs to (GroupState::rngword, rngword_pos):
// the next launch takes it where the word is one (a power of 48271 is never 0 modulo a prime: a zeroed state and a reset hold
// none) and its position is still the group's -- a kernel that advances rngpos without knowing of the word invalidates it.
TTX_HD bool cl_word_valid(uint64_t word, uint64_t wpos, uint64_t rngpos) { return word != 0 && wpos == rngpos; }
// The sorted pivot lists a launch leaves in global memory carry the number of the launch that wrote them (GroupState::zk_epoch;
// 0 after a reset: launches count from 1).  Launch `epoch` of a run takes them only from launch epoch - 1 of the same run.
TTX_HD bool cl_lists_valid(int tag, int epoch) { return tag != 0 && tag == epoch - 1; }
// Who packs what at the exit of a launch (tests/sweep_gap_main.cpp).  Everything the pack reads was published in front of the closing
// cluster_sync of the last bond step, which every workgroup has passed, so any of them may pack.  Part CL_PACK_RIGHT is red[] with
// the right-going message (exch_pack_right), part CL_PACK_LEFT the left-going message (exch_pack_left): workgroup 0 writes the group
// scalars red[] reads and packs the right part, workgroup 1 -- where the cluster has one and `split` (TTX_CL_PACK2) allows -- the left.
#define CL_PACK_RIGHT 0
#define CL_PACK_LEFT 1
TTX_HD int cl_pack_block(int part, int NB, bool split) { return (part == CL_PACK_LEFT && split && NB >= 2) ? 1 : 0; }
// ints of one group's image: [nsteps][2][RM] keys and [nsteps][2] counts, as they lie in LDS, rounded up to 16 bytes
TTX_HD size_t cl_zimage_ints(int nsteps, int RM) { return ((size_t)nsteps * 2 * (size_t)RM + 2 * (size_t)nsteps + 3) & ~(size_t)3; }
