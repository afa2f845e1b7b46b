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
};

inline LoopPlan loop_plan(const LoopIn &in)
{
    LoopPlan p;
    p.pipe = in.whole && !in.profile && !in.pipeline_off;
    p.head = p.pipe && in.W == 1 && in.maxrank > 1;
    p.forkq = p.pipe && in.has_quad && in.W == 1;
    p.tail = p.pipe && in.cluster && in.W == 1 && in.nproc > 1 && !in.host_pass && in.sweep_tail;
    p.side = p.tail && p.forkq && in.sweep_tail_side;
    return p;
}
