// Stand-alone host program for ttcross_amd/csrc/ttx_loop_plan.h (built and run by test_loop_plan_cpu.py, plain and under
// -fsanitize=address,undefined): loop_plan() over every combination of its inputs against a plain restatement of the expressions
// run_impl had before the plan existed, the implications between the fields, and the named configurations.
// Prints "<failures> <combinations walked>".
#include <cstdio>
#include "ttx_loop_plan.h"

static long bad = 0, ncomb = 0;
#define CHECK(c, ...) do { if (!(c)) { if (bad++ < 10) { printf("line %d: ", __LINE__); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// run_impl before the plan, in its own names: cluster = cluster_nb(), fused = sel.fused (at most one is set), env_off = TTX_PIPELINE=0,
// fun_host = (FUN == FUN_HOST).  `head` is the one rule that is new: pipe0 (which did not honour env_off) and maxrank > 1 gave head1,
// which only the pipelined branch read; now the head implies pipe.
struct Plain { bool pipe, forkq, tail, side, head; };
static Plain plain(int cluster, int fused, bool profile, bool env_off, int W, int nproc, bool has_quad, bool fun_host, int sweep_tail, int sweep_tail_side, int maxrank)
{
    Plain p;
    p.pipe = (cluster || fused) && !profile && !env_off;
    p.forkq = p.pipe && has_quad && W == 1;
    p.tail = p.pipe && cluster && W == 1 && nproc > 1 && !fun_host && sweep_tail;
    p.side = p.tail && p.forkq && sweep_tail_side;
    p.head = p.pipe && W == 1 && maxrank > 1;
    return p;
}

static void walk()
{
    const int ranks[3] = {1, 2, 5};
    for (int kernel = 0; kernel < 3; kernel++)          // none, fused, cluster
        for (int bits = 0; bits < 64; bits++)
            for (int W = 1; W <= 2; W++)
                for (int nproc = 1; nproc <= 3; nproc++)
                    for (int maxrank : ranks) {
                        LoopIn in;
                        in.whole = kernel != 0; in.cluster = kernel == 2;
                        in.profile = bits & 1; in.pipeline_off = bits & 2; in.has_quad = bits & 4; in.host_pass = bits & 8;
                        in.sweep_tail = bits & 16; in.sweep_tail_side = bits & 32;
                        in.W = W; in.nproc = nproc; in.maxrank = maxrank;
                        const LoopPlan p = loop_plan(in);
                        const Plain q = plain(kernel == 2 ? 8 : 0, kernel == 1, in.profile, in.pipeline_off, W, nproc, in.has_quad, in.host_pass, in.sweep_tail, in.sweep_tail_side, maxrank);
                        ncomb++;
                        CHECK(p.pipe == q.pipe && p.forkq == q.forkq && p.tail == q.tail && p.side == q.side && p.head == q.head,
                              "kernel %d bits %d W %d nproc %d maxrank %d: plan %d%d%d%d%d, restated %d%d%d%d%d (pipe head forkq tail side)", kernel, bits, W, nproc, maxrank,
                              p.pipe, p.head, p.forkq, p.tail, p.side, q.pipe, q.head, q.forkq, q.tail, q.side);
                        CHECK(!p.side || p.tail, "side without tail");
                        CHECK(!p.tail || p.pipe, "tail without pipe");
                        CHECK(!p.forkq || p.pipe, "forkq without pipe");
                        CHECK(!p.head || p.pipe, "head without pipe");
                        if (in.profile) CHECK(!p.pipe && !p.head && !p.forkq && !p.tail && !p.side, "profile mode must give the plain loop");
                    }
}

static void named()
{
    LoopIn b;       // the bench default: one process, cluster kernel, 8 groups, a quadrature, device integrand, both tail switches on
    b.whole = b.cluster = true; b.W = 1; b.nproc = 8; b.has_quad = true; b.sweep_tail = b.sweep_tail_side = true; b.maxrank = 64;
    LoopPlan p = loop_plan(b);
    CHECK(p.pipe && p.head && p.forkq && p.tail && p.side, "bench default: all five");
    LoopIn x = b;
    x.nproc = 1; p = loop_plan(x);
    CHECK(p.pipe && p.head && p.forkq && !p.tail && !p.side, "one group: no tail, no side");
    x = b; x.cluster = false; p = loop_plan(x);
    CHECK(p.pipe && p.head && p.forkq && !p.tail && !p.side, "fused: no tail");
    x = b; x.W = 2; p = loop_plan(x);
    CHECK(p.pipe && !p.head && !p.forkq && !p.tail && !p.side, "two processes: the pipelined loop and nothing else");
    x = b; x.pipeline_off = true; p = loop_plan(x);
    CHECK(!p.pipe && !p.head && !p.forkq && !p.tail && !p.side, "TTX_PIPELINE=0 with one process: the plain loop, no head");
}

int main()
{
    walk();
    named();
    printf("%ld %ld\n", bad, ncomb);
    return bad ? 1 : 0;
}
