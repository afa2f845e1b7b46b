"""Host overhead of the train operations: wall time of each call and the kernel figures the library reports.
usage: python profiles/trainops_measure.py LABEL OUTFILE   (TTX_LIB names the library: run the parent build and this tree alternately)"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

label, outfile = sys.argv[1], sys.argv[2]
rows = []


def timed(name, shape, reps, fn, fig=None):
    fn()                                            # warm-up
    ms, figs = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ms.append((time.perf_counter() - t0) * 1e3)
        if fig:
            figs.append(fig())
        if hasattr(r, "close"):
            r.close()
    row = dict(label=label, shape=shape, op=name, reps=reps, wall_ms_median=float(np.median(ms)), wall_ms_min=float(min(ms)), wall_ms_max=float(max(ms)))
    if figs:
        row["kernel_ms_median"] = [float(x) for x in np.median(np.asarray(figs, dtype=float), axis=0)]
    rows.append(row)
    print(json.dumps(row), flush=True)


def points(tt, npts, seed):
    n = np.asarray(tt._n, dtype=np.int64)
    return np.ascontiguousarray((np.random.default_rng(seed).integers(0, 2 ** 31 - 1, (npts, n.size)) % n + 1).astype(np.int32))


def measure(shape, tt, reps, big):
    d = tt.d
    w = [np.full(int(nk), 1.0 / int(nk)) for nk in tt._n]
    one = E.TTCross.from_cores([np.asarray(q).reshape(1, -1, 1) for q in w])           # rank-1 train: x o w
    for npts in (1000, 100000):
        ind = points(tt, npts, 7)
        timed(f"tijk_batch exact {npts}", shape, reps, lambda: tt.tijk_batch(ind, "exact"))
        timed(f"tijk_batch mfma {npts}", shape, reps, lambda: tt.tijk_batch(ind, "mfma"))
    x = np.random.default_rng(3).uniform(0.0, 1.0, (1000, 3 if d % 3 == 0 else 5))
    timed("value_batch exact 1000", shape, reps, lambda: tt.value_batch(x, "exact"))
    timed("marginals", shape, reps, lambda: tt.marginals(w), lambda: tt.contract_modesum()[:1])
    timed("contract ends", shape, reps, lambda: tt.contract(D.keep_flags("ends", d), w), lambda: tt.contract_modesum()[:1])
    timed("hadamard x o w", shape, reps, lambda: tt.hadamard(one), lambda: tt.algebra_last()[:1])
    if not big:
        timed("lincomb x + x", shape, reps, lambda: E.TTCross.lincomb([1.0, 1.0], [tt, tt]), lambda: tt.algebra_last()[:1])
    for npts in (1000, 100000):
        u = np.random.default_rng(5).random((npts, d))
        timed(f"sample {npts}", shape, reps, lambda: tt.sample(u, w), lambda: [tt.sample_last()[k] for k in ("ms_head", "ms_draw")])
    one.close()


rng = np.random.default_rng(64)
r = [1] + [32] * 62 + [1]
t64 = E.TTCross.from_cores([rng.uniform(0.0, 1.0, (r[k], 51, r[k + 1])) / (0.5 * r[k + 1]) for k in range(63)])
measure("d63_n51_r32", t64, 11, False)
t64.close()
t256 = D.tijk_train("rand256")
measure("d255_n101_r64", t256, 5, True)
t256.close()
with open(outfile, "w") as f:
    for row in rows:
        f.write(json.dumps(row) + "\n")
print("DONE", label)
