// ttx_loop_plan.h -- the form of one run's sweep loop, decided before anything is enqueued (host only, no HIP in here).
//
// loop_plan() is a pure function of what run_impl knows at the start of a run (LoopIn): which whole-sweep kernel the run uses after
// the retirements of ttx_run's fallbacks, the switches, the shape of the job.  It returns every decision the sweep driver of
// ttx_engine.hip (SweepRun) makes about the form of the loop; the driver computes none of its own.  tests/loop_plan_main.cpp walks
// all inputs on the CPU.
#pragma once

// what a run reads from the engine and the environment, filled per run (TTX_PIPELINE is read on every run, not at creation)
struct LoopIn {
    bool whole = false;             // a whole-sweep kernel is in use (k_sweep_cluster or k_sweep_fused), read after retirements ...
    bool cluster = false;           // ... and it is the cluster kernel (cluster_nb() != 0; else sel.fused)
    bool profile = false;           // profile mode: every launch bracketed by events, the host waits after every sweep
    bool pipeline_off = false;      // TTX_PIPELINE=0
    int W = 1;                      // processes (GPUs) of the job
    int nproc = 1;                  // bond groups of the job
    bool has_quad = false;          // a quadrature is reported per sweep
    bool host_pass = false;         // the integrand runs in two host passes around every evaluating kernel (FUN == FUN_HOST)
    bool sweep_tail = false;        // sel.sweep_tail (TTX_TAIL)
    bool sweep_tail_side = false;   // sel.sweep_tail_side (TTX_TAIL_SIDE)
    int maxrank = 1;
    bool head_direct = false;       // sel.head_direct (TTX_HEAD_DIRECT)
    bool fin_early = false;         // sel.fin_early (TTX_FIN_EARLY)
    bool fin_skip_exch = false;     // sel.fin_skip_exch (TTX_FIN_SKIP_EXCH)
};

struct LoopPlan {
    // Pipelined loop (whole-sweep kernels): the stopping rule also runs on the device (k_sweep_end), so sweep it+1 is enqueued BEFORE
    // the host has read the summary of sweep it -- the GPU never waits for the host.  Only the sweep kernel of it+1 is enqueued
    // speculatively (it keeps the GPU busy while the host reads the summary of sweep it); once the rule has fired that one launch
    // finds the stop flag and exits, and its tail is never enqueued.
    // With several processes the exchange and the summary travel by stream-ordered collectives (RCCL, or the host transport's host
    // functions), so the same loop applies; only the fork of the quadrature is single-process (one communicator must not be driven
    // from two streams at once).
    // The finalisation is enqueued once: in the pipelined loop as soon as the stopping rule has fired on the host, behind the ev_val
    // of the slot whose forked quadrature still reads the cores the finalisation overwrites -- a stream-side wait, the host does
    // not idle.
    // Off: profile mode, the chain path, TTX_PIPELINE=0 -- the host-synchronised loop, one readback per sweep.
    bool pipe = false;
    // Single-process pipelined loop with at least one sweep to run: the first sweep kernel is enqueued right behind the initial
    // cross, and the host waits only for the copy of the initial summary (an event, ev_sum[0]), not for the stream.  (The first
    // sweep kernel, already enqueued, runs with the same DevProb as the later ones: all of this is decided before the first launch.)
    bool head = false;
    // On a single GPU the per-sweep quadrature (only reported, never fed back) runs on its own stream next to the following sweep: it
    // reads a snapshot of the ranks and only slabs that already exist (appends are in place).
    bool forkq = false;
    // The end of a sweep as ONE exchange launch (k_exch_tail): single process, pipelined loop, cluster path, device integrand, at least
    // two groups (one group has no neighbour, its boundary launch never existed); k_sweep_end follows on the main stream.  Everything
    // else -- the chain path, k_sweep_fused, several processes, TTX_PIPELINE=0, profile mode, TTX_TAIL=0 -- keeps the launches it had.
    bool tail = false;
    // `tail` with the forked quadrature: the summary (k_sweep_summary) goes to the quadrature's stream as well, behind the tail launch
    // (ev_tail) and in front of the sweep's quadrature, and every block of the next sweep kernel applies the stopping rule itself
    // (DevProb::tail_side).  That side work is enqueued AFTER the next sweep kernel: at short sweeps (C_16) the host is what the
    // main stream waits for.
    bool side = false;
    // `head` without k_collect and the copy in front of sweep kernel 1, which reads nothing of either: k_init_final knows the whole
    // initial summary (ranks 1, tapes -1, the groups' counters and maxima final after k_init_fibers) and writes it into the pinned slot
    // itself, as k_sweep_end writes a sweep's.  A k_collect beside sweep kernel 1 would race with its writes of r and tape.  Every
    // other form keeps readback().
    bool head_direct = false;
    // The finalisation overwrites arg in place, and of the forked quadrature's kernels only k_quad_build reads arg (k_quad_chain reads
    // Tq, k_quad_tree qall): with `fin_early` the finalisation waits for an event behind the last quadrature's k_quad_build instead of
    // the value's copy, and runs beside the chain, the tree and the copy.  The clearing of ctl[0..2] no longer stands in front of the
    // LU kernels, which do not read ctl: it goes to the quadrature's stream behind k_quad_tree (which reads ctl[2]) and the value's
    // copy, in front of the final k_collect (which reads ctl[0]) and its copy on the same stream; the pack of a final exchange is
    // told to run behind the raised stop flag.  All of this is enqueued at once, the summary into the pinned slot the finished
    // sweep does not use, BEFORE the host blocks for the value: its last waits overlap.  Only where the quadrature is forked
    // (without it nothing waits, and with several processes it shares the main stream).
    bool fin_early = false;
    // The final exchange (k_exch_pack, k_exch_apply: dtt_lua shifts the rightmost inv of every group to its neighbour) repeats what
    // the end of the last sweep did: every sweep end packs inv(last) unconditionally and applies it, and nothing writes inv, r or upd
    // afterwards (the speculative sweep launch returns at its entry).  In one process it is left out behind at least one sweep --
    // final_exchange().  A run without a sweep needs it (the initial cross leaves inv(first-1) = 1), several processes keep it.
    bool fin_skip_exch = false;
    int nproc = 1;
    // does the finalisation of a run that made `sweeps` sweeps exchange first?
    bool final_exchange(int sweeps) const { return nproc > 1 && !(fin_skip_exch && sweeps >= 1); }
};

inline LoopPlan loop_plan(const LoopIn &in)
{
    LoopPlan p;
    p.pipe = in.whole && !in.profile && !in.pipeline_off;
    p.head = p.pipe && in.W == 1 && in.maxrank > 1;
    p.forkq = p.pipe && in.has_quad && in.W == 1;
    p.tail = p.pipe && in.cluster && in.W == 1 && in.nproc > 1 && !in.host_pass && in.sweep_tail;
    p.side = p.tail && p.forkq && in.sweep_tail_side;
    p.head_direct = p.head && in.head_direct;
    p.fin_early = p.forkq && in.fin_early;
    p.fin_skip_exch = in.W == 1 && in.fin_skip_exch;
    p.nproc = in.nproc;
    return p;
}
