"""Results of the tt_lib utilities as bytes, for comparing two builds of the library (TTX_LIB names the build, see
ttcross_amd/engine.py): ort, svd at three (tol, rmax), norm, lognrm, dot, tijk, quad, zquad and accchk on the swept trains of
Ising C_6 (n = 33, r = 12) and C_9 (n = 51, r = 32) and on two uploaded trains with wide and tall unfoldings.

    python profiles/ttops_compare.py out.npz            every core, rank vector and scalar into out.npz
    python profiles/ttops_compare.py --time 25          svd(1e-8), norm(), dot(x, x) of the C_9 train: 25 timings each, in ms

Two .npz files of two builds are compared with  python profiles/ttops_compare.py --cmp a.npz b.npz  (byte for byte)."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import tt_ref as R                      # noqa: E402
from ttcross_amd import drivers as D    # noqa: E402
from ttcross_amd import engine as E     # noqa: E402

SVD = [(1e-4, 0), (1e-8, 0), (1e-12, 5)]


def swept(m, n, r):
    s = D.ising_setup("c", m, n)
    return s, E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=2, accuracy=s["acc"], quad=s["quad"]).run()


def record(out, name, t, s=None):
    def put(key, v):
        out[f"{name}/{key}"] = np.asarray(v)

    def train(key, u):
        put(key + "/ranks", u.ranks())
        for k in range(1, u.d + 1):
            put(f"{key}/core{k}", u.core(k))

    cores = [t.core(k) for k in range(1, t.d + 1)]
    n = [c.shape[1] for c in cores]
    train("in", t)
    put("norm", [t.norm(), t.norm(1e-8), t.lognorm(), t.lognorm(1e-8)])
    put("dot", t.dot(t))
    put("tijk", [t.tijk(i) for i in R.probe_indices(n, 4)])
    put("quad", t.quad([np.cos(np.arange(1, k + 1)) for k in n]))
    x = np.arange(sum(n))
    put("zquad", t.zquad(np.array([np.exp(1j * (k + 1) * 0.01 * x) / (1 + x) for k in range(2)])))
    if s is not None:
        a = t.accchk(500)
        put("accchk", [a["einf"], a["efro"], a["ainf"], a["afro"]] + list(a["pivot"]))
    train("ort", E.TTCross.from_cores(cores).ort())
    for i, (tol, rmax) in enumerate(SVD):
        u = E.TTCross.from_cores(cores).svd(tol, rmax)
        train(f"svd{i}", u)
        put(f"svd{i}/dot", t.dot(u))


def main():
    if sys.argv[1] == "--cmp":
        a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
        bad = [k for k in a.files if k not in b.files or a[k].tobytes() != b[k].tobytes()] + [k for k in b.files if k not in a.files]
        print(f"{len(a.files)} arrays, {len(bad)} differ", *bad[:20])
        sys.exit(1 if bad else 0)
    if sys.argv[1] == "--time":
        reps = int(sys.argv[2])
        _, t = swept(9, 51, 32)
        cores = [t.core(k) for k in range(1, t.d + 1)]
        ops = {"svd(1e-8)": lambda: E.TTCross.from_cores(cores).svd(1e-8), "norm()": t.norm, "dot(x,x)": lambda: t.dot(t)}
        for name, f in ops.items():
            f()
            ms = []
            for _ in range(reps):
                t0 = time.perf_counter()
                f()
                ms.append((time.perf_counter() - t0) * 1e3)
            q1, med, q3 = np.percentile(ms, [25, 50, 75])
            print(f"{name:10s} median {med:8.3f} ms  quartiles {q1:8.3f} {q3:8.3f}  min {min(ms):8.3f} max {max(ms):8.3f}  ({reps} calls)")
        return
    out = {}
    for name, (m, n, r) in {"c6": (6, 33, 12), "c9_r32": (9, 51, 32)}.items():
        s, t = swept(m, n, r)
        record(out, name, t, s)
    record(out, "two_branch", E.TTCross.from_cores(R.rand_train(7, [2, 2, 5], [1, 6, 2, 1])))
    record(out, "tall", E.TTCross.from_cores(R.rand_train(8, [5, 3, 2], [1, 5, 12, 1])))
    np.savez(sys.argv[1], **out)
    print(f"{len(out)} arrays -> {sys.argv[1]}")


if __name__ == "__main__":
    main()
