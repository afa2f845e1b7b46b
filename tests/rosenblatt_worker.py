"""Child of test_gpu_rosenblatt.py, in a process of its own.
  chunk NAME MODE : the forward map of case NAME (signed) at the sampler's own points under whatever TTX_SAMPLE_CHUNK the parent set;
                    prints a digest of u, cell, logq, val
  dev             : the device-pointer entry (ttx_rosenblatt_sq_real_dev) with torch tensors against the host entry -- torch brings a HIP
                    runtime of its own and has to initialise its device before the engine's library does (tijk_dev_worker.py)
  nan             : a NaN and an Inf in a core, both modes: which rows fail, what they hold, the count, the range of the cells written
                    (the entry reaches every point's sums through the head pass: every point fails; numpy's SVD refuses such a train,
                    so the reference is not asked)
Prints one JSON line."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NAMES = ("u", "cell", "logq", "val")


def digest(res):
    return hashlib.sha256(b"".join(res[k].tobytes() for k in NAMES)).hexdigest()


def main():
    what = sys.argv[1]
    if what == "dev":
        import torch
        torch.cuda.init()
    import rosenblatt_cases as RC
    from ttcross_amd import engine as E
    if what == "chunk":
        cores, u, nodes = RC.case(sys.argv[2], True)
        tt = E.TTCross.from_cores(cores)
        x = tt.sample_sq_real(u, nodes, gamma=0.125, mode=sys.argv[3])["x"]
        print(json.dumps(dict(digest=digest(tt.rosenblatt_sq_real(x, nodes, gamma=0.125, mode=sys.argv[3])), failed=tt.rosenblatt_sq_real_last()["failed"])))
        return
    if what == "nan":
        cores, _, nodes = RC.case("d3", True)
        x = RC.cloud(nodes, 200, 17)
        ncell = np.array([c.shape[1] - 1 for c in cores])
        out = {}
        for tag, bad in (("nan", np.nan), ("inf", np.inf)):
            cs = [c.copy() for c in cores]
            cs[1][1, 4, 0] = bad
            tt = E.TTCross.from_cores(cs)
            for mode in ("exact", "mfma"):
                res = tt.rosenblatt_sq_real(x, nodes, mode=mode)
                failed = np.isnan(res["u"][:, 0])
                good = ~failed
                out[tag + "_" + mode] = dict(in_range=bool(np.all(res["cell"] >= 0) and np.all(res["cell"] <= ncell[None, :])),
                                             whole_rows=bool(np.all(np.isnan(res["u"][failed])) and np.all(res["cell"][failed] == 0) and np.all((res["cell"] > 0)[good])
                                                             and np.all((res["u"][good] >= 0.0) & (res["u"][good] <= 1.0))),
                                             failed=int(failed.sum()), counted=tt.rosenblatt_sq_real_last()["failed"],
                                             marked=bool(np.all(np.isnan(res["logq"][failed])) and np.all(res["val"][failed] == 0.0)))
        print(json.dumps(out))
        return
    cores, u, nodes = RC.case("d8_unequal", True)
    tt = E.TTCross.from_cores(cores)
    cond = [np.nan, np.nan, float(nodes[2][0]), np.nan, np.nan, np.nan, 0.5 * float(nodes[6][0] + nodes[6][1]), np.nan]
    res = {}
    for mode in ("exact", "mfma"):
        x = tt.sample_sq_real(u, nodes, cond, 0.125, mode)["x"].copy()
        x[7, 3] = np.nan
        host = tt.rosenblatt_sq_real(x, nodes, cond, 0.125, mode)
        t = torch.from_numpy(x).to("cuda:0")
        dev = tt.rosenblatt_sq_real(t, nodes, cond, 0.125, mode)
        same = all(np.array_equal(dev[k].cpu().numpy(), host[k], equal_nan=(k != "cell")) for k in NAMES)
        res[mode] = dict(is_cuda=all(bool(v.is_cuda) for v in dev.values()), dtypes=[str(dev[k].dtype) for k in NAMES], equal=bool(same),
                         failed=tt.rosenblatt_sq_real_last()["failed"], only_u=sorted(tt.rosenblatt_sq_real(t, nodes, cond, 0.125, mode, want=("u",))),
                         empty=list(tt.rosenblatt_sq_real(t[:0].contiguous(), nodes)["u"].shape))
    try:
        tt.rosenblatt_sq_real(t.to(torch.float32), nodes)
        res["float32_refused"] = False
    except ValueError:
        res["float32_refused"] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
