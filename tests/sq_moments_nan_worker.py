"""Child of test_gpu_sq_moments.py: one NaN entry in a core, in a process of its own, so that whatever a NaN does to a kernel stays here.
What include/ttx.h documents: a NaN core gives NaN by the arithmetic -- z_mant, every moment and every band entry, since the NaN reaches
Z and everything is divided by it -- and nothing faults.  A clean engine afterwards gives the clean bits.  Prints one JSON line."""
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
    nodes = [np.cumsum(rng.uniform(0.2, 1.0, nk)) for nk in n]
    md, mo = E.mass_tridiag(nodes)
    ad, ao = E.moment_tridiag(nodes, 1)
    a2d, a2o = E.moment_tridiag(nodes, 2)
    bad = [c.copy() for c in cores]
    bad[2][1, 30, 2] = np.nan
    tt, tb = E.TTCross.from_cores(cores), E.TTCross.from_cores(bad)
    res = {}
    for mode in ("exact", "mfma"):
        c = tt.sq_moments(md, mo, ad, ao, a2d, a2o, mode=mode)
        b = tb.sq_moments(md, mo, ad, ao, a2d, a2o, mode=mode)
        a = tt.sq_moments(md, mo, ad, ao, a2d, a2o, mode=mode)
        res[mode] = dict(clean_finite=bool(np.isfinite(c["m1"]).all() and np.isfinite(c["c2"]).all() and all(np.isfinite(v).all() for v in c["bd"] + c["bo"])),
                         z_nan=bool(np.isnan(b["z_mant"])),
                         moments_all_nan=bool(np.isnan(b["m1"]).all() and np.isnan(b["c2"]).all()),
                         band_all_nan=bool(all(np.isnan(v).all() for v in b["bd"]) and all(np.isnan(v[:-1]).all() and v[-1] == 0.0 for v in b["bo"])),
                         clean_again_equal=bool(_eq(a["m1"], c["m1"]) and _eq(a["c2"], c["c2"]) and all(_eq(p, q) for p, q in zip(a["bd"] + a["bo"], c["bd"] + c["bo"]))))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
