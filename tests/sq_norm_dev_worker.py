"""Child of test_gpu_sq_norm.py: what needs torch tensors on the device -- the device-pointer entries (ttx_sq_lognorm_grad_dev,
ttx_sq_nll_batch_dev) against the host-pointer entries ("dev"), and TTCross.fit_density on the pinned problem of sq_norm_ref ("fit") --
in a process of its own: torch brings a HIP runtime of its own and has to initialise its device before the engine's library does.
Prints one JSON line."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _eq(t, a):
    return bool(np.array_equal(t.cpu().numpy().view(np.int64), np.ascontiguousarray(a).view(np.int64)))


def dev():
    import torch
    torch.cuda.init()
    import sq_norm_ref as S
    import tt_ref as R
    from ttcross_amd import engine as E
    n, r = [7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]
    cores = R.rand_train(5, n, r)
    tt = E.TTCross.from_cores(cores)
    rng = np.random.default_rng(15)
    nodes = [np.cumsum(rng.uniform(0.2, 1.0, nk)) for nk in n]
    md, mo = E.mass_tridiag(nodes)
    basis = [("linear", t) for t in nodes]
    x = np.ascontiguousarray(np.stack([rng.uniform(t[0], t[-1], 40) for t in nodes], axis=1))
    w = rng.uniform(0.5, 1.5, 40)
    xt, wt = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(w).to("cuda:0")
    total = int(tt.core_offsets()[-1])
    res = {}
    for mode in ("exact", "mfma"):
        host = tt.sq_lognorm_grad(md, mo, 0.2, 1.5, mode=mode)
        out = torch.full((total,), 7.0, dtype=torch.float64, device="cuda:0")
        d1 = tt.sq_lognorm_grad(md, mo, 0.2, 1.5, out=out, mode=mode)
        first = bool(d1["g"] is out) and _eq(out, S.pack(host["g"])) and d1["logz"] == host["logz"] and d1["z_exp"] == host["z_exp"]
        twice = tt.sq_lognorm_grad(md, mo, 0.2, 1.5, out=host["g"], accumulate=True, mode=mode)["g"]
        hn, hn1 = tt.sq_nll(x, basis, 0.05, md, mo, 0.3, w, mode), tt.sq_nll(x, basis, 0.05, md, mo, 0.3, None, mode)
        dn, dn1 = tt.sq_nll(xt, basis, 0.05, md, mo, 0.3, wt, mode), tt.sq_nll(xt, basis, 0.05, md, mo, 0.3, None, mode, out=out)
        res[mode] = dict(lognorm_equal=first, nll_is_cuda=bool(dn["val"].is_cuda and dn["g"].is_cuda), nll_into_out=bool(dn1["g"] is out),
                         nll_equal=bool(dn["nll"] == hn["nll"] and dn["logz"] == hn["logz"]) and _eq(dn["val"], hn["val"]) and _eq(dn["g"], S.pack(hn["g"])),
                         nll_unweighted_equal=bool(dn1["nll"] == hn1["nll"]) and _eq(dn1["val"], hn1["val"]) and _eq(dn1["g"], S.pack(hn1["g"])))
        acc = torch.from_numpy(S.pack(host["g"])).to("cuda:0")
        tt.sq_lognorm_grad(md, mo, 0.2, 1.5, out=acc, accumulate=True, mode=mode)
        res[mode]["accumulated_equal"] = _eq(acc, S.pack(twice))
    for key, call in (("float32_refused", lambda: tt.sq_nll(xt.to(torch.float32), basis, 0.05, md, mo, 0.3)),
                      ("host_w_refused", lambda: tt.sq_nll(xt, basis, 0.05, md, mo, 0.3, w)),
                      ("short_out_refused", lambda: tt.sq_lognorm_grad(md, mo, out=torch.zeros(total - 1, dtype=torch.float64, device="cuda:0")))):
        try:
            call()
            res[key] = False
        except ValueError:
            res[key] = True
    print(json.dumps(res))


def fit():
    import torch
    torch.cuda.init()
    import sq_norm_ref as S
    from ttcross_amd import engine as E
    prob = S.fit_problem()
    basis = [("linear", t) for t in prob["nodes"]]
    res = {}
    for mode in ("exact", "mfma"):
        tt = E.TTCross.from_cores(prob["cores"])
        held = lambda: tt.sq_nll(prob["xh"], basis, prob["gamma"], prob["md"], prob["mo"], prob["gvol"], None, "exact")["nll"]     # noqa: E731
        before = held()
        got = tt.fit_density(prob["x"], basis, prob["gamma"], prob["md"], prob["mo"], prob["gvol"], prob["w"], mode, max_iter=6)
        res[mode] = dict(hist=[[float(h[0]), bool(h[1]), float(h[2])] for h in got["hist"]], nll=[float(v) for v in got["nll"]], iters=got["iters"],
                         held_before=before, held_after=held())
    print(json.dumps(res))


if __name__ == "__main__":
    dict(dev=dev, fit=fit)[sys.argv[1]]()
