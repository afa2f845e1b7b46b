"""Child of test_gpu_basis_core_grad.py: one NaN coordinate ("coord") or one NaN weight ("weight") among 300 points, in a process of
its own, so that whatever a NaN does to a kernel stays here.  What include/ttx.h documents: a point with a NaN table entry or a NaN
c[p] makes every entry of G it reaches NaN -- here every entry of every G_i, since the point's term reaches them all -- while val is
NaN at a point with a NaN coordinate only and does not see c.  A clean call afterwards gives the clean call's bits.  Prints one JSON
line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _eq(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)))


def main(what):
    import tt_ref as R
    from ttcross_amd import engine as E
    n, r = [7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]
    tt = E.TTCross.from_cores(R.rand_train(5, n, r))
    rng = np.random.default_rng(45)
    basis = [("cos", 0.0, 1.0), ("linear", [0.0, 1.0]), ("cos", 0.0, 1.0, True), ("cos", 0.0, 1.0), ("linear", np.linspace(0.0, 1.0, 9))]
    x, c = rng.uniform(0.0, 1.0, (300, 5)), rng.standard_normal(300)
    bx, bc = x.copy(), c.copy()
    hit = np.zeros(300, bool)
    if what == "coord":
        bx[261, 1] = np.nan                                                     # LINEAR: a NaN row; point 261 lies in the second segment of 256
        hit[261] = True
    else:
        bc[7] = np.nan
    res = {}
    for mode in ("exact", "mfma"):
        cv, cg = tt.basis_core_grad(x, basis, c, mode)
        bv, bg = tt.basis_core_grad(bx, basis, bc, mode)
        av, ag = tt.basis_core_grad(x, basis, c, mode)
        res[mode] = dict(clean_finite=bool(np.isfinite(cv).all() and all(np.isfinite(g).all() for g in cg)),
                         val_as_documented=bool(np.isnan(bv[hit]).all() and _eq(bv[~hit], cv[~hit])),
                         g_all_nan=bool(all(np.isnan(g).all() for g in bg)),
                         clean_again_equal=_eq(av, cv) and all(_eq(a, b) for a, b in zip(ag, cg)))
    print(json.dumps(res))


if __name__ == "__main__":
    main(sys.argv[1])
