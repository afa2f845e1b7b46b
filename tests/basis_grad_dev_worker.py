"""Child of test_gpu_basis_grad.py: the device-pointer entries (ttx_basis_grad_batch_dev, ttx_basis_grad_tab_dev) with torch tensors
against the host-pointer entries, in a process of its own -- torch brings a HIP runtime of its own and has to initialise its device
before the engine's library does.  Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _eq(t, a):
    return bool(np.array_equal(t.cpu().numpy().view(np.int64), np.ascontiguousarray(a).view(np.int64)))


def main():
    import torch
    torch.cuda.init()
    import tt_ref as R
    from ttcross_amd import engine as E
    n, r = [4, 5, 3, 2], [1, 16, 33, 65, 1]
    tt = E.TTCross.from_cores(R.rand_train(8, n, r))
    rng = np.random.default_rng(14)
    nodes = np.sort(rng.uniform(0.0, 1.0, 5))
    basis = [("cos", -1.0, 2.0, True), ("linear", nodes), ("cos", 0.0, 1.0), ("linear", [0.25, 0.5])]
    x = np.ascontiguousarray(rng.uniform(-0.1, 1.1, (300, 4)))
    tab = np.ascontiguousarray(np.hstack([E.basis_table(e, nk, x[:, k]) for k, (e, nk) in enumerate(zip(basis, n))]))
    dtab = np.ascontiguousarray(np.hstack([E.basis_dtable(e, nk, x[:, k]) for k, (e, nk) in enumerate(zip(basis, n))]))
    xt, tabt, dtabt = (torch.from_numpy(a).to("cuda:0") for a in (x, tab, dtab))
    res = {}
    for mode in ("exact", "mfma"):
        os.environ.pop("TTX_BASIS_CHUNK", None)
        hb, ht = tt.basis_grad_batch(x, basis, mode), tt.basis_grad_tab(tab, dtab, mode)
        db, dt = tt.basis_grad_batch(xt, basis, mode), tt.basis_grad_tab(tabt, dtabt, mode)
        os.environ["TTX_BASIS_CHUNK"] = "64"
        dc = tt.basis_grad_batch(xt, basis, mode)
        em = tt.basis_grad_tab(tabt[:0].contiguous(), dtabt[:0].contiguous(), mode)
        res[mode] = dict(batch_is_cuda=bool(db[0].is_cuda and db[1].is_cuda), batch_equal=_eq(db[0], hb[0]) and _eq(db[1], hb[1]),
                         tab_is_cuda=bool(dt[0].is_cuda and dt[1].is_cuda), tab_equal=_eq(dt[0], ht[0]) and _eq(dt[1], ht[1]),
                         chunked_equal=_eq(dc[0], hb[0]) and _eq(dc[1], hb[1]), empty=[list(em[0].shape), list(em[1].shape)])
    os.environ.pop("TTX_BASIS_CHUNK", None)
    for key, call in (("float32_refused", lambda: tt.basis_grad_batch(xt.to(torch.float32), basis, "exact")),
                      ("shape_refused", lambda: tt.basis_grad_batch(xt[:, :3].contiguous(), basis, "exact")),
                      ("host_dphi_refused", lambda: tt.basis_grad_tab(tabt, dtab, "exact"))):      # one table on the device, the other on the host
        try:
            call()
            res[key] = False
        except ValueError:
            res[key] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
