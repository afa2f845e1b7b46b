"""Worker of tests/test_gpu_run_ends.py: one problem in a fresh process under every form of the two ends of a run, everything each
run leaves dumped to one .npz.

usage: run_ends_worker.py OUT.npz family m n r piv groups arith runs quad [userfun.so]
  family: c | d (Ising), mvn, stdnorm, host (tests/userfun.c through ttx_set_integrand_host; userfun.so names its shared object);
  m: the Ising index or the dimension; arith: exact | fast; runs: run() calls on the one engine; quad: quad | noquad.
The switches are read when an engine is created, so every form gets an engine of its own: `old` (all six switches 0), `new` (none
set: the defaults), and each switch alone (the other five 0).  The rest of the environment (TTX_SWEEP, ...) is the caller's.
Keys: <form>_run<k>_<what>; <form>_path, <form>_launches_<kind>."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ttcross_amd import drivers as D  # noqa: E402
from ttcross_amd import engine as E  # noqa: E402

SWITCHES = ("TTX_HEAD_DIRECT", "TTX_INIT_WIDE", "TTX_INIT_WAVE", "TTX_FIN_EARLY", "TTX_FIN_SKIP_EXCH", "TTX_QUAD_LDS")
FORMS = {"old": (), "new": None, **{"only_" + s[4:].lower(): (s,) for s in SWITCHES}}


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
    path, family, m, n, r, piv, groups, arith, runs, quad = sys.argv[1:11]
    m, n, r, piv, groups, runs = int(m), int(n), int(r), int(piv), int(groups), int(runs)
    addr = None
    if family in "cd":
        s = D.ising_setup(family, m, n)
    elif family == "host":
        x, w = D.lgwt(n)
        par = np.concatenate([0.5 * (x + 1.0), 0.5 * w])
        s = dict(n=[n] * m, par=par, quad=[par[n:].copy()] * m, acc=500 * D.EPS, tru=None, aux=None, fun_id=E.TTX_FUN_HOST)
        lib = ctypes.CDLL(sys.argv[11])
        addr = ctypes.cast(lib.ttx_test_userfun, ctypes.c_void_p).value
    else:
        s = D.box_setup(family, m, n)
    out = {}
    for form, on in FORMS.items():
        for name in SWITCHES:
            os.environ.pop(name, None)
            if on is not None:
                os.environ[name] = "1" if name in on else "0"
        tt = E.TTCross(s["n"], s["fun_id"], [] if addr else s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"] if quad == "quad" else None,
                       tru=s["tru"], aux=s["aux"], nproc=groups, arith=arith)
        if addr:
            tt.set_integrand_host(addr, s["par"])
        for k in range(runs):
            tt.run()
            dump(tt, s["quad"], f"{form}_run{k}_", out)
        for kind, v in tt.kernel_stats().items():
            out[f"{form}_launches_{kind}"] = np.array([v["launches"]], dtype=np.int64)
        out[form + "_path"] = np.array([tt.sweep_path()])
        out[form + "_arith"] = np.array([tt.arith])
        del tt
    np.savez(path, **out)
    print("WORKER OK")


if __name__ == "__main__":
    main()
