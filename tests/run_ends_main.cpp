// Stand-alone host program for the decisions about the two ends of a run in ttcross_amd/csrc/ttx_loop_plan.h and for the switches
// and launch shapes behind them in ttx_create_plan.h (built and run by test_run_ends_cpu.py, plain and under -fsanitize=address,undefined):
// loop_plan() over every combination of its inputs, the fields head_direct, fin_early, fin_skip_exch and final_exchange() against
// the rules stated here in plain words, the old fields untouched by the new switches, and the named configurations.
// Prints "<failures> <combinations walked>".
#include <cstdio>
#include <cstring>
#include "ttx_create_plan.h"
#include "ttx_loop_plan.h"

static long bad = 0, ncomb = 0;
#define CHECK(c, ...) do { if (!(c)) { if (bad++ < 10) { printf("line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

static void walk()
{
    const int ranks[3] = {1, 2, 5};
    for (int kernel = 0; kernel < 3; kernel++)          // none, fused, cluster
        for (int bits = 0; bits < 512; bits++)
            for (int W = 1; W <= 2; W++)
                for (int nproc = 1; nproc <= 3; nproc++)
                    for (int maxrank : ranks) {
                        LoopIn in;
                        in.whole = kernel != 0; in.cluster = kernel == 2;
                        in.profile = bits & 1; in.pipeline_off = bits & 2; in.has_quad = bits & 4; in.host_pass = bits & 8;
                        in.sweep_tail = bits & 16; in.sweep_tail_side = bits & 32;
                        in.head_direct = bits & 64; in.fin_early = bits & 128; in.fin_skip_exch = bits & 256;
                        in.W = W; in.nproc = nproc; in.maxrank = maxrank;
                        const LoopPlan p = loop_plan(in);
                        ncomb++;
                        // the new switches change none of the old decisions
                        LoopIn o = in;
                        o.head_direct = o.fin_early = o.fin_skip_exch = false;
                        const LoopPlan q = loop_plan(o);
                        CHECK(p.pipe == q.pipe && p.head == q.head && p.forkq == q.forkq && p.tail == q.tail && p.side == q.side, "a new switch moved an old field (kernel %d bits %d)", kernel, bits);
                        CHECK(!q.head_direct && !q.fin_early && !q.fin_skip_exch, "all switches off: the old form");
                        // head: only the single-process pipelined loop with a sweep to run has a summary copy in front of sweep kernel 1
                        const bool single_pipe = in.whole && !in.profile && !in.pipeline_off && W == 1;
                        CHECK(p.head_direct == (in.head_direct && single_pipe && maxrank > 1), "head_direct (kernel %d bits %d W %d maxrank %d)", kernel, bits, W, maxrank);
                        CHECK(!p.head_direct || p.head, "head_direct without head");
                        // end: only a forked quadrature makes the finalisation wait
                        CHECK(p.fin_early == (in.fin_early && single_pipe && in.has_quad), "fin_early (kernel %d bits %d W %d)", kernel, bits, W);
                        CHECK(!p.fin_early || p.forkq, "fin_early without a forked quadrature");
                        if (in.profile) CHECK(!p.head_direct && !p.fin_early, "profile mode keeps the plain loop");
                        // the final exchange: never with one group; always without a sweep and with several processes
                        for (int sweeps = 0; sweeps <= 3; sweeps++) {
                            const bool x = p.final_exchange(sweeps);
                            if (nproc == 1) CHECK(!x, "one group has no neighbour");
                            else if (sweeps == 0 || W > 1 || !in.fin_skip_exch) CHECK(x, "the final exchange is needed (W %d nproc %d sweeps %d bits %d)", W, nproc, sweeps, bits);
                            else CHECK(!x, "the final exchange repeats the last sweep's (W %d nproc %d sweeps %d bits %d)", W, nproc, sweeps, bits);
                            CHECK(q.final_exchange(sweeps) == (nproc > 1), "switch off: the exchange whenever there are neighbours");
                        }
                    }
}

static void named()
{
    LoopIn b;       // the bench default: one process, cluster kernel, 8 groups, a quadrature, device integrand, every switch on
    b.whole = b.cluster = true; b.W = 1; b.nproc = 8; b.has_quad = true; b.sweep_tail = b.sweep_tail_side = true; b.maxrank = 64;
    b.head_direct = b.fin_early = b.fin_skip_exch = true;
    LoopPlan p = loop_plan(b);
    CHECK(p.head_direct && p.fin_early && !p.final_exchange(16) && p.final_exchange(0), "bench default: all three");
    LoopIn x = b;
    x.maxrank = 1; p = loop_plan(x);
    CHECK(!p.head_direct && p.final_exchange(0), "maxrank 1: no sweep, readback() and the final exchange");
    x = b; x.has_quad = false; p = loop_plan(x);
    CHECK(p.head_direct && !p.fin_early && !p.final_exchange(3), "no quadrature: nothing to wait for");
    x = b; x.W = 2; p = loop_plan(x);
    CHECK(!p.head_direct && !p.fin_early && p.final_exchange(3), "two processes keep today's order");
    x = b; x.whole = x.cluster = false; p = loop_plan(x);
    CHECK(!p.head_direct && !p.fin_early && !p.final_exchange(3) && p.final_exchange(0), "chain path: readback(); its sweep ends exchange too");
    x = b; x.pipeline_off = true; p = loop_plan(x);
    CHECK(!p.head_direct && !p.fin_early, "TTX_PIPELINE=0: the plain loop");
}

// the switches as create_env_from reads them: on unless set to 0
static void switches()
{
    const char *names[6] = {"TTX_HEAD_DIRECT", "TTX_INIT_WAVE", "TTX_FIN_EARLY", "TTX_FIN_SKIP_EXCH", "TTX_INIT_WIDE", "TTX_QUAD_LDS"};
    for (int set = -1; set < 6; set++)
        for (const char *value : {"0", "1"}) {
            const CreateEnv e = create_env_from([&](const char *n) -> const char * { return set >= 0 && !strcmp(n, names[set]) ? value : nullptr; });
            const bool off[6] = {e.head_direct_off, e.init_wave_off, e.fin_early_off, e.fin_skip_exch_off, e.init_wide_off, e.quad_lds_off};
            for (int k = 0; k < 6; k++) CHECK(off[k] == (k == set && value[0] == '0'), "%s=%s: switch %d", set >= 0 ? names[set] : "(none)", value, k);
            CHECK(!e.tail_off && !e.tail_side_off, "the tail switches are not touched");
        }
    const CreatePlan dflt;
    CHECK(dflt.head_direct && dflt.init_wave && dflt.init_wide && dflt.fin_early && dflt.fin_skip_exch, "the new forms are the default");
}

// the launch of k_init_samples: the old form where the switch is off or the kernel does not walk its own rows, the generic accessor
// where 256 rows do not fit, else whole waves for all samples between 256 and 512 threads with room for the mode sizes
static void samples()
{
    const long counts[7] = {8, 255, 256, 257, 408, 512, 5000};
    for (int d = 2; d <= 2100; d += (d < 70 ? 1 : 97))
        for (long ns : counts)
            for (int bits = 0; bits < 4; bits++) {
                const size_t VS = ((d + 7) & ~7) + 8, lds_par = sizeof(double) * (2 * 51 + 3);
                const bool own = bits & 1, wide = bits & 2;
                const InitSamplesPlan p = init_samples_plan(lds_par, VS, d, ns, own, wide);
                ncomb++;
                const size_t lds1 = lds_par + 16 + sizeof(short) * 256 * VS;
                CHECK(p.lds <= TTX_LDS_WORK && p.threads % 64 == 0 && p.threads >= 256 && p.threads <= 512, "d %d ns %ld: shape", d, ns);
                if (lds1 > TTX_LDS_WORK) { CHECK(p.rows == 0 && p.threads == 256 && p.lds == lds_par, "d %d: the rows do not fit", d); continue; }
                if (!own || !wide) { CHECK(p.rows == 1 && p.threads == 256 && p.lds == lds1, "d %d ns %ld bits %d: the old form", d, ns, bits); continue; }
                if (p.rows == 1) { CHECK(p.threads == 256 && p.lds == lds1, "d %d ns %ld: fallback to the old form", d, ns); continue; }
                CHECK(p.rows == 2, "d %d ns %ld: rows", d, ns);
                // the rows of all threads, aligned, then the d mode sizes, aligned
                CHECK(p.lds >= lds_par + 15 + sizeof(short) * (size_t)p.threads * VS + 15 + sizeof(int) * (size_t)d, "d %d ns %ld: room for rows and mode sizes", d, ns);
                if (ns <= 512) CHECK(p.threads >= ns, "d %d ns %ld threads %d: one pass", d, ns, p.threads);
                CHECK(p.threads == 256 || p.threads - ns < 64, "d %d ns %ld: no wave without a sample", d, ns);
            }
    const InitSamplesPlan b = init_samples_plan(sizeof(double) * 105, 72, 63, 408, true, true);     // the bench default: d = 63, 8 x 51 samples
    CHECK(b.rows == 2 && b.threads == 448, "bench default: 448 threads, one pass");
    // the quadrature's tree in LDS: two regions of nproc matrices where they fit, never with one group or with the switch off
    for (int nproc = 1; nproc <= 16; nproc++)
        for (size_t RM = 1; RM <= 128; RM++) {
            const size_t need = sizeof(double) * 2 * nproc * RM * RM, got = quad_tree_lds(nproc, RM, true);
            ncomb++;
            CHECK(quad_tree_lds(nproc, RM, false) == 0, "switch off");
            CHECK(got == (nproc > 1 && need <= TTX_LDS_WORK ? need : 0), "nproc %d RM %zu", nproc, RM);
        }
    CHECK(quad_tree_lds(8, 32, true) == 131072 && quad_tree_lds(8, 40, true) == 0 && quad_tree_lds(4, 40, true) == 102400, "the bench default fits; r = 40 with four groups, not with eight");
}

int main()
{
    walk();
    named();
    switches();
    samples();
    printf("%ld %ld\n", bad, ncomb);
    return bad ? 1 : 0;
}
