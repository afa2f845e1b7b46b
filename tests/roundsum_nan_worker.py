"""ttx_lincomb_round on a train with a NaN core, in a process of its own (tests/test_gpu_roundsum.py starts it, so that a GPU fault
would fail that test instead of taking the test runner down).  Exit code 0 and "OK": the call ended and the new train is NaN."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import roundsum_ref as RS
    from ttcross_amd import engine as E
    trains = [[g.copy() for g in RS.edge_train(x)] for x in ("r3", "r5", "r17")]
    trains[1][3][2, 0, 1] = np.nan
    eng = [E.TTCross.from_cores(x) for x in trains]
    ok = True
    for mode in ("exact", "mfma"):
        new = E.TTCross.lincomb_round([1.0, 2.0, -1.0], eng, rank=17, seed=1, mode=mode)
        ind = np.ones((1, new.d), dtype=np.int32)
        v = new.tijk_batch(ind, "exact")
        cores = [new.core(k) for k in range(1, new.d + 1)]
        ok = ok and bool(np.isnan(v).all()) and any(np.isnan(g).any() for g in cores)
        print(mode, "ranks", new.ranks().tolist(), "element", v, flush=True)
        new.close()
    print("OK" if ok else "BAD", flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
