// Host check of what the cluster sweep kernel (ttcross_amd/csrc/ttx_cluster.h) carries from launch to launch instead of
// recomputing it at its entry (ttcross_amd/csrc/ttx_cluster_rules.h):
//   * the compile-time table of generator powers: entry t is ttx_minstd_pow(2 t) for t = 0 .. 255, entry 64 is ttx_minstd_pow(128);
//   * the generator step of a bond step from the table (cl_stepmul) is ttx_minstd_pow(2 nlot) for nlot = 0 .. 1200 (the table
//     form below 512 candidates, the loop from there on), and the word carried over sequences of such steps -- two steps per
//     bond step, as the kernel takes them -- stays ttx_minstd_pow(2 rngpos + 1) at every step, for sequences of small nlot, of
//     nlot >= 64, of nlot >= 512 and of a mix;
//   * the validity rules: a carried word is taken only where it is non-zero and its position is the group's (a zeroed state, a
//     reset, and a position advanced by a kernel that knows nothing of the word are all refused); the carried lists are taken
//     only by launch tag + 1 of a run, never on a cleared tag.
// Prints "<bad> <checks>".
#include <cstdint>
#include <cstdio>
#include "ttx_cluster_rules.h"

static long bad = 0, nchk = 0;
static void check(bool ok) { nchk++; if (!ok) bad++; }

static constexpr ClPowTab TAB = cl_make_powtab();
static_assert(TAB.v[0] == 1 && TAB.v[1] == 48271ull * 48271ull % 2147483647ull, "the first entries by hand");

static uint64_t lane_lookup(int l) { return TAB.v[l]; }      // the kernel reads lane l's register, which holds entry l

static void sequence(const int *nlots, int n, int rounds)
{
    uint64_t rngpos = 0, word = ttx_minstd_pow(1);
    const uint64_t c64 = TAB.v[64];
    for (int r = 0; r < rounds; r++)
        for (int k = 0; k < n; k++) {
            const int nlot = nlots[k];
            const uint64_t stepmul = cl_stepmul(nlot, lane_lookup, c64);
            const uint64_t w1 = ttx_mulmod31(word, stepmul);                 // the second draw column of this bond step
            check(w1 == ttx_minstd_pow(2 * (rngpos + (uint64_t)nlot) + 1));
            word = ttx_mulmod31(w1, stepmul); rngpos += 2ull * (uint64_t)nlot;
            check(word == ttx_minstd_pow(2 * rngpos + 1));
            check(word != 0 && word < 2147483647ull);
            check(cl_word_valid(word, rngpos, rngpos));
        }
}

int main()
{
    for (int t = 0; t < CL_POWTAB_N; t++) check(TAB.v[t] == ttx_minstd_pow(2ull * (uint64_t)t));
    check(TAB.v[64] == ttx_minstd_pow(128));
    for (uint64_t e = 0; e < 3000; e++) check(cl_minstd_pow_c(e) == ttx_minstd_pow(e));
    for (uint64_t e = 1; e < (1ull << 40); e = e * 3 + 1) check(cl_minstd_pow_c(e) == ttx_minstd_pow(e));
    for (int nlot = 0; nlot <= 1200; nlot++) check(cl_stepmul(nlot, lane_lookup, (uint64_t)TAB.v[64]) == ttx_minstd_pow(2ull * (uint64_t)nlot));

    const int small[] = {4, 20, 23, 37, 52, 63, 1, 2};
    const int mid[] = {64, 65, 127, 128, 166, 191, 192, 300, 448, 511};
    const int big[] = {512, 513, 600, 1023, 1024, 1101};
    const int mix[] = {20, 166, 512, 63, 64, 511, 700, 5, 128};
    sequence(small, 8, 200); sequence(mid, 10, 100); sequence(big, 6, 100); sequence(mix, 9, 100);

    // the carried word
    check(!cl_word_valid(0, 0, 0));                         // a zeroed state and a reset: no word
    check(!cl_word_valid(0, 5, 5));
    check(cl_word_valid(48271, 0, 0));
    check(!cl_word_valid(48271, 0, 40));                    // the position has been advanced by someone else
    check(!cl_word_valid(48271, 40, 0));                    // ... or set back
    // the carried lists: launch `epoch` takes what launch epoch - 1 of the same run left; a reset clears the tag to 0
    for (int epoch = 1; epoch <= 40; epoch++)
        for (int tag = 0; tag <= 41; tag++) check(cl_lists_valid(tag, epoch) == (tag >= 1 && tag == epoch - 1));
    check(!cl_lists_valid(0, 1));                           // the first launch of a run always rebuilds
    std::printf("%ld %ld\n", bad, nchk);
    return bad != 0;
}
