"""Worker of tests/test_gpu_sweep_gap.py: one problem in a fresh process under every form of the stretch between two sweeps,
everything each run leaves dumped to one .npz.

usage: sweep_gap_worker.py OUT.npz family m n r piv groups arith runs
  family: c | d (Ising); m: the Ising index; arith: exact | fast; runs: run() calls on the one engine.
The switches are read when an engine is created, so every form gets an engine of its own: `old` (all three in the form they had:
TTX_TAIL_EVENT=marker, the other two 0), `new` (none set: the defaults), and each switch alone (the other two in the old form).
The rest of the environment (TTX_SWEEP, TTX_CLUSTER_NB, ...) is the caller's.
Keys: <form>_run<k>_<what>; <form>_path, <form>_arith, <form>_launches_<kind>, <form>_gap (tail event by kernel, its fallbacks, lean,
pack2), <form>_entry<k> (launches of run k that took the carried lists, the carried word)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ttcross_amd import drivers as D  # noqa: E402
from ttcross_amd import engine as E  # noqa: E402

OLD = {"TTX_TAIL_EVENT": "marker", "TTX_TAIL_LEAN": "0", "TTX_CL_PACK2": "0"}
NEW = {"TTX_TAIL_EVENT": "kernel", "TTX_TAIL_LEAN": "1", "TTX_CL_PACK2": "1"}
FORMS = {"old": dict(OLD), "new": {}, **{"only_" + s[4:].lower(): {**OLD, s: NEW[s]} for s in OLD}}


def dump(tt, quad, tag, out):
    sw = tt.sweeps()
    for key in ("it", "dir", "erank", "neval", "val", "amax", "pivotmax", "pivotmin"):
        out[f"{tag}sw_{key}"] = np.array([a[key] for a in sw], dtype=np.float64 if key not in ("it", "dir", "neval") else np.int64)
    out[tag + "tapes"] = tt.tapes()
    out[tag + "ranks"] = tt.ranks()
    out[tag + "neval"] = np.array([tt.neval], dtype=np.int64)
    out[tag + "quad"] = np.array([tt.quad(quad)])
    for k in range(1, tt.d + 1):
        out[f"{tag}core{k}"] = tt.core(k)


def main():
    path, family, m, n, r, piv, groups, arith, runs = sys.argv[1:10]
    m, n, r, piv, groups, runs = int(m), int(n), int(r), int(piv), int(groups), int(runs)
    s = D.ising_setup(family, m, n)
    out = {}
    for form, env in FORMS.items():
        for name in OLD:
            os.environ.pop(name, None)
        os.environ.update(env)
        tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], aux=s["aux"], nproc=groups, arith=arith)
        for k in range(runs):
            tt.run()
            dump(tt, s["quad"], f"{form}_run{k}_", out)
            ce = tt.cluster_entry()
            out[f"{form}_entry{k}"] = np.array([ce["lists_taken"], ce["word_taken"]], dtype=np.int64)
        for kind, v in tt.kernel_stats().items():
            out[f"{form}_launches_{kind}"] = np.array([v["launches"]], dtype=np.int64)
        gap = tt.sweep_gap()
        out[form + "_gap"] = np.array([gap["tail_event"] == "kernel", gap["tail_event_fallbacks"], gap["tail_lean"], gap["cl_pack2"]], dtype=np.int64)
        out[form + "_path"] = np.array([tt.sweep_path()])
        out[form + "_arith"] = np.array([tt.arith])
        out[form + "_fallbacks"] = np.array([tt.cluster_fallbacks], dtype=np.int64)
        del tt
    np.savez(path, **out)
    print("WORKER OK")


if __name__ == "__main__":
    main()
