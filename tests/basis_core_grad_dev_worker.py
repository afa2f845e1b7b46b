"""Child of test_gpu_basis_core_grad.py: the device-pointer entries (ttx_basis_core_grad_batch_dev, ttx_basis_core_grad_tab_dev,
ttx_cores_axpy_dev) with torch tensors against the host-pointer entries, in a process of its own -- torch brings a HIP runtime of its
own and has to initialise its device before the engine's library does.  Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _eq(t, a):
    return bool(np.array_equal(t.cpu().numpy().view(np.int64), np.ascontiguousarray(a).view(np.int64)))


def _flat(blocks):
    return np.concatenate([b.ravel(order="F") for b in blocks])


def main():
    import torch
    torch.cuda.init()
    import tt_ref as R
    from ttcross_amd import engine as E
    n, r = [4, 5, 3, 2], [1, 16, 33, 65, 1]
    cores = R.rand_train(8, n, r)
    tt = E.TTCross.from_cores(cores)
    rng = np.random.default_rng(14)
    nodes = np.sort(rng.uniform(0.0, 1.0, 5))
    basis = [("cos", -1.0, 2.0, True), ("linear", nodes), ("cos", 0.0, 1.0), ("linear", [0.25, 0.5])]
    x = np.ascontiguousarray(rng.uniform(-0.1, 1.1, (300, 4)))
    c = np.ascontiguousarray(rng.standard_normal(300))
    tab = np.ascontiguousarray(np.hstack([E.basis_table(e, nk, x[:, k]) for k, (e, nk) in enumerate(zip(basis, n))]))
    xt, tabt, ct = (torch.from_numpy(a).to("cuda:0") for a in (x, tab, c))
    total = int(tt.core_offsets()[-1])
    res = {}
    for mode in ("exact", "mfma"):
        os.environ.pop("TTX_BASIS_CHUNK", None)
        hb, ht = tt.basis_core_grad(x, basis, c, mode), tt.basis_core_grad_tab(tab, c, mode)
        db, dt = tt.basis_core_grad(xt, basis, ct, mode), tt.basis_core_grad_tab(tabt, ct, mode)
        os.environ["TTX_BASIS_CHUNK"] = "256"
        hc = tt.basis_core_grad(x, basis, c, mode)
        dc = tt.basis_core_grad(xt, basis, ct, mode)
        os.environ.pop("TTX_BASIS_CHUNK", None)
        # two calls on the halves, the second accumulates onto the first's tensor, against the same on the host
        h1 = tt.basis_core_grad_tab(tab[:150], c[:150], mode)[1]
        h2 = tt.basis_core_grad_tab(tab[150:], c[150:], mode, out=h1, accumulate=True)[1]
        d1 = tt.basis_core_grad_tab(tabt[:150].contiguous(), ct[:150].contiguous(), mode)[1]
        d2 = tt.basis_core_grad_tab(tabt[150:].contiguous(), ct[150:].contiguous(), mode, out=d1, accumulate=True)[1]
        # npts = 0 on the device: accumulate = 0 zeroes the tensor, accumulate = 1 leaves it
        seven = torch.full((total,), 7.0, dtype=torch.float64, device="cuda:0")
        tt.basis_core_grad_tab(tabt[:0].contiguous(), ct[:0].contiguous(), mode, out=seven, accumulate=True)
        keeps = bool((seven == 7.0).all().item())
        tt.basis_core_grad_tab(tabt[:0].contiguous(), ct[:0].contiguous(), mode, out=seven)
        res[mode] = dict(batch_is_cuda=bool(db[0].is_cuda and db[1].is_cuda), batch_equal=_eq(db[0], hb[0]) and _eq(db[1], _flat(hb[1])),
                         tab_is_cuda=bool(dt[0].is_cuda and dt[1].is_cuda), tab_equal=_eq(dt[0], ht[0]) and _eq(dt[1], _flat(ht[1])),
                         chunked_equal=_eq(dc[0], hc[0]) and _eq(dc[1], _flat(hc[1])), accumulated_equal=bool(d2.data_ptr() == d1.data_ptr()) and _eq(d2, _flat(h2)),
                         empty_zeroes=bool((seven == 0.0).all().item()), empty_keeps=keeps)
    # ttx_cores_axpy_dev against ttx_cores_axpy on a second engine of the same cores
    alpha = np.array([0.5, 0.0, -2.0, 1.0])
    g_host = tt.basis_core_grad_tab(tab, c, "exact")[1]
    g_dev = tt.basis_core_grad_tab(tabt, ct, "exact")[1]
    other = E.TTCross.from_cores(cores)
    other.cores_axpy(alpha, g_host)
    tt.cores_axpy(alpha, g_dev)
    res["axpy_equal"] = all(bool(np.array_equal(tt.core(k + 1).view(np.int64), other.core(k + 1).view(np.int64))) for k in range(4))
    res["axpy_equal"] = res["axpy_equal"] and all(bool(np.array_equal(tt.core(k + 1), cores[k] + alpha[k] * g_host[k])) for k in range(4))
    for key, call in (("float32_refused", lambda: tt.basis_core_grad(xt.to(torch.float32), basis, ct, "exact")),
                      ("host_c_refused", lambda: tt.basis_core_grad_tab(tabt, c, "exact")),           # the table on the device, the weights on the host
                      ("short_out_refused", lambda: tt.basis_core_grad_tab(tabt, ct, "exact", out=torch.zeros(total - 1, dtype=torch.float64, device="cuda:0")))):
        try:
            call()
            res[key] = False
        except ValueError:
            res[key] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
