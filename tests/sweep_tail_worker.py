"""Worker of tests/test_gpu_sweep_tail.py: one engine set-up in a fresh process, everything a run leaves dumped to an .npz.

usage: sweep_tail_worker.py OUT.npz m n r piv groups accuracy maxrank_runs arith
  accuracy: `default` (the driver's) or a number; maxrank_runs: how many run() calls on the one engine (results of each are kept);
  arith: exact | fast.  The environment (TTX_TAIL, TTX_CLUSTER_TEST_ABORT, ...) is the caller's."""
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
    s = D.ising_setup("c", int(m), int(n))
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], int(r), pivoting=int(piv), accuracy=s["acc"] if acc == "default" else float(acc),
                   quad=s["quad"], tru=s["tru"], nproc=int(groups), arith=arith)
    out = {"path_before": np.array([tt.sweep_path()]), "arith": np.array([tt.arith])}
    for k in range(int(runs)):
        tt.run()
        dump(tt, s, f"run{k}_", out)
    out["path_after"] = np.array([tt.sweep_path()])
    out["cluster_fallbacks"] = np.array([tt.cluster_fallbacks], dtype=np.int64)
    np.savez(path, **out)
    print("WORKER OK")


if __name__ == "__main__":
    main()
