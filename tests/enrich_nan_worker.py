"""Child of test_gpu_enrich.py: one NaN weight c[p] among 300 points, in a process of its own, so that whatever a NaN does to a kernel
stays here.  What include/ttx.h documents: the point's term reaches every entry of every sketch Y_b, so every bond that could take
directions (k_b > 0) takes none -- added 0, its gain row NaN -- the bonds with k_b = 0 keep gain 0.0, the new train is a plain copy, the
source is untouched and a clean call afterwards gives the clean call's bits.  Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _eq(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64)))


def main():
    import tt_ref as R
    from ttcross_amd import engine as E
    n, r = [7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]
    cores = R.rand_train(5, n, r)
    tt = E.TTCross.from_cores(cores)
    rng = np.random.default_rng(45)
    tab, c = rng.standard_normal((300, sum(n))), rng.standard_normal(300)
    bc = c.copy()
    bc[261] = np.nan                                                            # in the second segment of 256
    res = {}
    for mode in ("exact", "mfma"):
        cn, ci = tt.enrich_tab(tab, c, 20, 3, mode, want_sketch=True)
        bn, bi = tt.enrich_tab(tab, bc, 20, 3, mode, want_sketch=True)
        an, ai = tt.enrich_tab(tab, c, 20, 3, mode, want_sketch=True)
        k = ci["k"]
        res[mode] = dict(clean_added=ci["added"] == k and k == [4, 0, 4, 1],
                         clean_finite=bool(all(np.isfinite(y).all() for y in ci["y"]) and all(np.isfinite(g).all() for g in ci["gain"])),
                         nan_added_none=bi["added"] == [0, 0, 0, 0],
                         nan_gain=bool(all(np.isnan(g).all() if kb else g.size == 0 for g, kb in zip(bi["gain"], k))),
                         nan_sketch=bool(all(np.isnan(y).all() for y in bi["y"])),
                         nan_train_is_a_copy=bool([int(v) for v in bn.ranks()] == r and all(_eq(bn.core(i + 1), cores[i]) for i in range(5))),
                         source_untouched=bool(all(_eq(tt.core(i + 1), cores[i]) for i in range(5))),
                         clean_again_equal=bool(all(_eq(a, b) for a, b in zip(ai["y"], ci["y"])) and _eq(ai["ynorm2"], ci["ynorm2"]) and
                                                all(_eq(an.core(i + 1)[:r[i], :, :r[i + 1]], cores[i]) for i in range(5))))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
