"""Child of test_gpu_topk.py, in a process of its own: ttx_topk on a train whose cores hold a NaN and an Inf.  One call per mode,
not a loop: the call must return without error, every index must lie in range and bound must be NaN.  Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import topk_ref as R
    from ttcross_amd import engine as E
    cores = [c.copy() for c in R.case("d4")]
    cores[1][2, 3, 1] = np.nan
    cores[2][0, 4, 2] = np.inf
    n = np.array([c.shape[1] for c in cores])
    tt = E.TTCross.from_cores(cores)
    out = {}
    for mode in ("exact", "mfma"):
        res = tt.topk(17, mode=mode)
        out[mode] = dict(rows=int(res["ind"].shape[0]), in_range=bool(np.all((res["ind"] >= 1) & (res["ind"] <= n[None, :]))),
                         distinct=len({tuple(r) for r in res["ind"]}), bound_is_nan=bool(np.isnan(res["bound"])), certified=res["certified"])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
