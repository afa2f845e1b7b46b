"""One run of an integrand of trains that meets non-finite values -- the ratio of two trains whose denominator has exact zeros --
in a process of its own with its own time limit (tests/test_gpu_trainfun.py), as tests/devfun_nan_worker.py does for loaded
integrands.  Ordinary arithmetic: Inf and NaN values, never addresses; the run must end like the host-callback engine's.

    python tests/trainfun_nan_worker.py PIV NPROC
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import trainfun_util as T
    from ttcross_amd import drivers as D
    from ttcross_amd import engine as E
    piv, nproc = int(sys.argv[1]), int(sys.argv[2])
    d, n, r = 5, 5, 4
    nn = [n] * d
    num = T.random_cores(nn, 2, seed=31)
    den = T.random_cores(nn, 1, seed=32, positive=True)
    den[1][:, 2, :] = 0.0                       # rank 1: every element with i_2 = 3 is an exact zero
    num[3][:, 1, :] = 0.0                       # ... and 0 / 0 where i_4 = 2 as well
    quad = T.box_quad(nn)
    x, y = E.TTCross.from_cores(num), E.TTCross.from_cores(den)
    tt = E.TTCross.of_trains([x, y], "ratio", r, accuracy=500 * D.EPS, pivoting=piv, quad=quad, nproc=nproc).run()
    T.twin_set([num, den])
    hh = E.TTCross(nn, E.TTX_FUN_HOST, [], r, pivoting=piv, accuracy=500 * D.EPS, quad=quad, nproc=nproc)
    hh.set_integrand_host(T.twin_addr("ratio"), [0.0]).run()
    tp = tt.tapes()
    same = np.array_equal(tp, hh.tapes()) and np.array_equal(tt.ranks(), hh.ranks())
    for f in ("neval", "val", "amax"):
        same = same and all((a[f] == b[f]) or (a[f] != a[f] and b[f] != b[f]) for a, b in zip(tt.sweeps(), hh.sweeps()))
    same = same and len(tt.sweeps()) == len(hh.sweeps())
    print(f"ratio with zeros piv={piv} nproc={nproc} sweeps={tp.shape[0]} same_as_host={same} {'OK' if same else 'BAD'}", flush=True)
    for e in (tt, hh, x, y):
        e.close()
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
