"""Child of test_gpu_basis.py: the device-pointer entries (ttx_basis_batch_dev, ttx_basis_tab_dev) with torch tensors against the
host-pointer entries, in a process of its own -- torch brings a HIP runtime of its own and has to initialise its device before
the engine's library does.  Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    torch.cuda.init()
    import tt_ref as R
    from ttcross_amd import engine as E
    n, r = [4, 5, 3, 2], [1, 16, 33, 65, 1]
    tt = E.TTCross.from_cores(R.rand_train(8, n, r))
    rng = np.random.default_rng(13)
    nodes = np.sort(rng.uniform(0.0, 1.0, 5))
    basis = [("cos", -1.0, 2.0, True), ("linear", nodes), ("cos", 0.0, 1.0), ("linear", [0.25, 0.5])]
    x = np.ascontiguousarray(rng.uniform(-0.1, 1.1, (300, 4)))
    tab = np.ascontiguousarray(np.hstack([E.basis_table(e, nk, x[:, k]) for k, (e, nk) in enumerate(zip(basis, n))]))
    xt, tabt = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(tab).to("cuda:0")
    res = {}
    for mode in ("exact", "mfma"):
        os.environ.pop("TTX_BASIS_CHUNK", None)
        hb, ht = tt.basis_batch(x, basis, mode), tt.basis_tab(tab, mode)
        db, dt = tt.basis_batch(xt, basis, mode), tt.basis_tab(tabt, mode)
        os.environ["TTX_BASIS_CHUNK"] = "64"
        dc = tt.basis_batch(xt, basis, mode)
        res[mode] = dict(batch_is_cuda=bool(db.is_cuda), batch_equal=bool(np.array_equal(db.cpu().numpy().view(np.int64), hb.view(np.int64))),
                         tab_is_cuda=bool(dt.is_cuda), tab_equal=bool(np.array_equal(dt.cpu().numpy().view(np.int64), ht.view(np.int64))),
                         chunked_equal=bool(np.array_equal(dc.cpu().numpy().view(np.int64), hb.view(np.int64))),
                         empty=list(tt.basis_tab(tabt[:0].contiguous(), mode).shape))
    for key, bad in (("float32_refused", xt.to(torch.float32)), ("shape_refused", xt[:, :3].contiguous())):
        try:
            tt.basis_batch(bad, basis, "exact")
            res[key] = False
        except ValueError:
            res[key] = True
    if torch.cuda.device_count() > 1:                  # a tensor on another device than the engine's is refused, not passed on
        try:
            tt.basis_batch(xt.to("cuda:1"), basis, "exact")
            res["other_device_refused"] = False
        except ValueError:
            res["other_device_refused"] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
