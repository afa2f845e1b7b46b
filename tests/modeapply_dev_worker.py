"""Child of test_gpu_modeapply.py: the device-pointer entry (ttx_mode_apply_dev) with torch tensors against the host-pointer entry,
in a process of its own -- torch brings a HIP runtime of its own and has to initialise its device before the engine's library
does.  Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    mode = sys.argv[1]
    import torch
    torch.cuda.init()
    import tt_ref as R
    from ttcross_amd import engine as E
    n, r, m = [9, 33, 10], [1, 17, 65, 1], [15, 0, 16]
    tt = E.TTCross.from_cores(R.rand_train(5, n, r))
    rng = np.random.default_rng(3)
    mats = [rng.standard_normal((mk, nk)) if mk else None for mk, nk in zip(m, n)]
    host = tt.mode_apply(mats, mode)
    tm = [None if a is None else torch.from_numpy(a).to("cuda:0") for a in mats]
    dev = tt.mode_apply(tm, mode)
    dct = tt.mode_apply({1: tm[0], 3: tm[2]}, mode)
    res = dict(ranks=dev.ranks().tolist(), modes=dev._n.tolist(), ran=tt.mode_apply_last()["mode"],
               equal=all(dev.core(k).tobytes() == host.core(k).tobytes() == dct.core(k).tobytes() for k in range(1, 4)))
    try:
        tt.mode_apply([tm[0].to(torch.float32), None, None], mode)
        res["float32_refused"] = False
    except ValueError:
        res["float32_refused"] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
