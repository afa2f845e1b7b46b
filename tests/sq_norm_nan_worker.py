"""Child of test_gpu_sq_norm.py: one NaN entry in a core, in a process of its own, so that whatever a NaN does to a kernel stays here.
What include/ttx.h documents: a NaN core gives NaN -- z_mant, logz and every entry of every G_k, since no power of two is applied to a
matrix with an entry that is not finite and the NaN reaches Z -- and nothing faults.  A clean engine afterwards gives the clean bits.
Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _eq(a, b):
    return bool(np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64)))


def main():
    import tt_ref as R
    from ttcross_amd import engine as E
    n, r = [7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]
    cores = R.rand_train(5, n, r)
    rng = np.random.default_rng(46)
    md, mo = E.mass_tridiag([np.cumsum(rng.uniform(0.2, 1.0, nk)) for nk in n])
    bad = [c.copy() for c in cores]
    bad[2][1, 30, 2] = np.nan
    tt, tb = E.TTCross.from_cores(cores), E.TTCross.from_cores(bad)
    x = rng.uniform(0.3, 0.6, (20, 5))
    res = {}
    for mode in ("exact", "mfma"):
        c = tt.sq_lognorm_grad(md, mo, 0.1, 1.0, mode=mode)
        b = tb.sq_lognorm_grad(md, mo, 0.1, 1.0, mode=mode)
        a = tt.sq_lognorm_grad(md, mo, 0.1, 1.0, mode=mode)
        nodes = [np.linspace(0.0, 1.0, nk) if nk > 1 else np.array([0.5]) for nk in n]
        nb = tb.sq_nll(x, [("linear", t) for t in nodes], 0.01, md, mo, 0.1, mode=mode)
        res[mode] = dict(clean_finite=bool(np.isfinite(c["logz"]) and all(np.isfinite(g).all() for g in c["g"])),
                         z_nan=bool(np.isnan(b["z_mant"]) and np.isnan(b["logz"])),
                         g_all_nan=bool(all(np.isnan(g).all() for g in b["g"])),
                         nll_nan=bool(np.isnan(nb["nll"]) and all(np.isnan(g).all() for g in nb["g"])),
                         clean_again_equal=bool(a["z_mant"] == c["z_mant"] and a["z_exp"] == c["z_exp"] and all(_eq(p, q) for p, q in zip(a["g"], c["g"]))))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
