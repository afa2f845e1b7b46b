"""Child of test_gpu_basis_jvp.py: the device-pointer entries (ttx_basis_jvp_batch_dev, ttx_basis_jvp_tab_dev, ttx_cores_dot_dev,
ttx_cores_axpby_dev, ttx_cores_get_dev, ttx_cores_set_dev, ttx_basis_fit_batch_dev, ttx_basis_fit_tab_dev) with torch tensors against
the host-pointer entries and the numpy restatements, and a NaN coordinate, in a process of its own -- torch brings a HIP runtime of
its own and has to initialise its device before the engine's library does; and whatever a NaN does to a kernel, it does not take the
test process with it.  Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _eq(t, a):
    t = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    t, a = np.ascontiguousarray(t), np.ascontiguousarray(a)
    return t.shape == a.shape and t.dtype == a.dtype and t.tobytes() == a.tobytes()


def _hist_eq(a, b):
    return all(_eq(a[k], b[k]) for k in ("loss", "lambda_", "cg_iters", "accepted")) and a["iters"] == b["iters"] and a["stop"] == b["stop"]


def main():
    import torch
    torch.cuda.init()
    import basis_jvp_ref as J
    import tt_ref as R
    from ttcross_amd import engine as E
    n, r = [4, 5, 3, 2], [1, 16, 33, 65, 1]
    cores = R.rand_train(8, n, r)
    tt = E.TTCross.from_cores(cores)
    rng = np.random.default_rng(15)
    nodes = np.sort(rng.uniform(0.0, 1.0, 5))
    basis = [("cos", -1.0, 2.0, True), ("linear", nodes), ("cos", 0.0, 1.0), ("linear", [0.25, 0.5])]
    x = np.ascontiguousarray(rng.uniform(-0.1, 1.1, (300, 4)))
    v = J.pack([rng.standard_normal(u.shape) for u in cores])
    tab = np.ascontiguousarray(np.hstack([E.basis_table(e, nk, x[:, k]) for k, (e, nk) in enumerate(zip(basis, n))]))
    xt, tabt, vt = (torch.from_numpy(a).to("cuda:0") for a in (x, tab, v))
    total = int(tt.core_offsets()[-1])
    xn = x.copy()
    xn[123, 2] = np.nan
    # a small least-squares problem for the two fit entries: targets from a second train, the start 5 % off it
    truth = R.rand_train(9, n, r)
    y = E.TTCross.from_cores(truth).basis_tab(tab, "exact")
    w = np.ascontiguousarray(rng.uniform(0.5, 1.5, 300))
    start = [u * (1.0 + 0.05 * rng.uniform(-1.0, 1.0, u.shape)) for u in truth]
    yt, wt = torch.from_numpy(y).to("cuda:0"), torch.from_numpy(w).to("cuda:0")
    opts = dict(max_iter=3, cg_max=8, lambda0=1e-2, cg_tol=1e-3)
    res = {}
    for mode in ("exact", "mfma"):
        os.environ.pop("TTX_BASIS_CHUNK", None)
        hb, ht = tt.basis_jvp(x, basis, v, mode), tt.basis_jvp_tab(tab, v, mode)
        db, dt = tt.basis_jvp(xt, basis, vt, mode), tt.basis_jvp_tab(tabt, vt, mode)
        os.environ["TTX_BASIS_CHUNK"] = "256"
        dc = tt.basis_jvp(xt, basis, vt, mode)
        os.environ.pop("TTX_BASIS_CHUNK", None)
        nv, nd = tt.basis_jvp(xn, basis, v, mode)
        keep = np.arange(300) != 123
        fits = {}
        for key, call in (("host_tab", lambda e: e.fit_tab(tab, y, w, mode=mode, **opts)), ("dev_tab", lambda e: e.fit_tab(tabt, yt, wt, mode=mode, **opts)),
                          ("host_batch", lambda e: e.fit(x, basis, y, None, mode=mode, **opts)), ("dev_batch", lambda e: e.fit(xt, basis, yt, None, mode=mode, **opts))):
            e = E.TTCross.from_cores(start)
            fits[key] = (call(e), e.cores_get())
        res[mode] = dict(batch_is_cuda=bool(db[0].is_cuda and db[1].is_cuda), batch_equal=_eq(db[0], hb[0]) and _eq(db[1], hb[1]) and _eq(hb[0], ht[0]) and _eq(hb[1], ht[1]),
                         tab_equal=_eq(dt[0], ht[0]) and _eq(dt[1], ht[1]), chunked_equal=_eq(dc[0], hb[0]) and _eq(dc[1], hb[1]),
                         nan_point_is_nan=bool(np.isnan(nv[123]) and np.isnan(nd[123])), nan_others_equal=_eq(nv[keep], hb[0][keep]) and _eq(nd[keep], hb[1][keep]),
                         fit_tab_equal=_hist_eq(fits["host_tab"][0], fits["dev_tab"][0]) and _eq(fits["host_tab"][1], fits["dev_tab"][1])
                         and bool(fits["host_tab"][0]["loss"][-1] < fits["host_tab"][0]["loss"][0]),
                         fit_batch_equal=_hist_eq(fits["host_batch"][0], fits["dev_batch"][0]) and _eq(fits["host_batch"][1], fits["dev_batch"][1]))
    # the vector operations on device tensors against the restatements
    a, b = rng.standard_normal(total), rng.standard_normal(total)
    at, bt = torch.from_numpy(a).to("cuda:0"), torch.from_numpy(b).to("cuda:0")
    dd = tt.cores_dot(at, bt)
    res["dot_equal"] = bool(np.float64(dd).view(np.int64) == np.float64(J.dot(a, b)).view(np.int64)) and bool(np.float64(tt.cores_dot(a, b)).view(np.int64) == np.float64(dd).view(np.int64))
    back = tt.cores_axpby(0.37, at, -2.5, bt)
    res["axpby_equal"] = bool(back.data_ptr() == bt.data_ptr()) and _eq(bt, J.axpby(0.37, a, -2.5, b)) and _eq(at, a)
    got = tt.cores_get(torch.empty(total, dtype=torch.float64, device="cuda:0"))
    res["get_equal"] = _eq(got, J.pack(cores))
    other = E.TTCross.from_cores(cores)
    other.cores_set(at)
    res["set_equal"] = _eq(other.cores_get(), a) and _eq(J.pack([other.core(k + 1) for k in range(4)]), a)
    for key, call in (("float32_refused", lambda: tt.basis_jvp(xt.to(torch.float32), basis, vt, "exact")),
                      ("host_v_refused", lambda: tt.basis_jvp_tab(tabt, v, "exact")),                  # the table on the device, the direction on the host
                      ("short_v_refused", lambda: tt.basis_jvp_tab(tabt, vt[:-1].contiguous(), "exact"))):
        try:
            call()
            res[key] = False
        except ValueError:
            res[key] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
