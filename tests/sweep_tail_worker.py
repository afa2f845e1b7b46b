"""Worker of tests/test_gpu_sweep_tail.py: one engine set-up in a fresh process, everything a run leaves dumped to an .npz.

usage: sweep_tail_worker.py OUT.npz m n r piv groups accuracy maxrank_runs arith [noquad]
  accuracy: `default` (the driver's) or a number; maxrank_runs: how many run() calls on the one engine (results of each are kept);
  arith: exact | fast; noquad: the engine is created without quadrature weights (no per-sweep value).  The environment (TTX_TAIL,
  TTX_CLUSTER_TEST_ABORT, ...) is the caller's.  Next to the results of each run (run<k>_...), what the last run launched:
  launches_<kind> from kernel_stats() and nsweeps = len(sweeps())."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ttcross_amd import drivers as D  # noqa: E402
from ttcross_amd import engine as E  # noqa: E402


def dump(tt, s, tag, out):
    sw = tt.sweeps()
    for key in ("it", "dir", "erank", "neval", "val", "amax", "pivotmax", "pivotmin"):
        out[f"{tag}sw_{key}"] = np.array([a[key] for a in sw], dtype=np.float64 if key not in ("it", "dir", "neval") else np.int64)
    out[tag + "tapes"] = tt.tapes()
    out[tag + "ranks"] = tt.ranks()
    out[tag + "neval"] = np.array([tt.neval], dtype=np.int64)
    out[tag + "quad"] = np.array([tt.quad(s["quad"])])
    for k in range(1, tt.d + 1):
        out[f"{tag}core{k}"] = tt.core(k)


def main():
    path, m, n, r, piv, groups, acc, runs, arith = sys.argv[1:10]
    noquad = sys.argv[10:11] == ["noquad"]
    s = D.ising_setup("c", int(m), int(n))
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], int(r), pivoting=int(piv), accuracy=s["acc"] if acc == "default" else float(acc),
                   quad=None if noquad else s["quad"], tru=s["tru"], nproc=int(groups), arith=arith)
    out = {"path_before": np.array([tt.sweep_path()]), "arith": np.array([tt.arith])}
    for k in range(int(runs)):
        tt.run()
        dump(tt, s, f"run{k}_", out)
    for kind, v in tt.kernel_stats().items():
        out["launches_" + kind] = np.array([v["launches"]], dtype=np.int64)
    out["nsweeps"] = np.array([len(tt.sweeps())], dtype=np.int64)
    out["path_after"] = np.array([tt.sweep_path()])
    out["cluster_fallbacks"] = np.array([tt.cluster_fallbacks], dtype=np.int64)
    np.savez(path, **out)
    print("WORKER OK")


if __name__ == "__main__":
    main()
