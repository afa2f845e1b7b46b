"""Child of test_gpu_sample_real.py, in a process of its own.
  chunk NAME : the samples of case NAME under whatever TTX_SAMPLE_CHUNK the parent set; prints a digest of x, cell, logq, val
  dev        : the device-pointer entry (ttx_sample_real_dev) with torch tensors against the host entry -- torch brings a HIP
               runtime of its own and has to initialise its device before the engine's library does (tijk_dev_worker.py)
  nonfinite  : trains with a NaN and with an Inf in a core: inputs with a defined result, the call returns
Prints one JSON line."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
NAMES = ("x", "cell", "logq", "val")


def digest(res):
    return hashlib.sha256(b"".join(res[k].tobytes() for k in NAMES)).hexdigest()


def main():
    what = sys.argv[1]
    if what == "dev":
        import torch
        torch.cuda.init()
    import sample_real_ref as SR
    from ttcross_amd import engine as E
    if what == "chunk":
        cores, u, nodes = SR.case(sys.argv[2])
        tt = E.TTCross.from_cores(cores)
        print(json.dumps(dict(digest=digest(tt.sample_real(u, nodes)), failed=tt.sample_real_last()["failed"])))
        return
    if what == "nonfinite":
        cores, u, nodes = SR.case("d3")
        u = u[:500]
        n = np.array([c.shape[1] for c in cores])
        out = {}
        for tag, bad in (("nan", np.nan), ("inf", np.inf)):
            cs = [c.copy() for c in cores]
            cs[1][1, 4, 0] = bad
            tt = E.TTCross.from_cores(cs)
            res = tt.sample_real(u, nodes)
            failed = np.isnan(res["x"][:, 0])
            lo, hi = np.array([t[0] for t in nodes]), np.array([t[-1] for t in nodes])
            out[tag] = dict(cells_in_range=bool(np.all(res["cell"] >= 0) and np.all(res["cell"] <= (n - 1)[None, :])),
                            failed_rows=bool(np.all(np.isnan(res["x"][failed])) and np.all(res["cell"][failed] == 0) and np.all(np.isnan(res["logq"][failed]))
                                             and np.all(res["val"][failed] == 0.0)),
                            others_drawn=bool(np.all(res["cell"][~failed] >= 1) and np.all((res["x"][~failed] >= lo) & (res["x"][~failed] <= hi))),
                            nfailed=int(failed.sum()), counted=tt.sample_real_last()["failed"])
        print(json.dumps(out))
        return
    cores, u, nodes = SR.case("d8_unequal")
    tt = E.TTCross.from_cores(cores)
    cond = [np.nan, np.nan, float(nodes[2][0]), np.nan, np.nan, np.nan, 0.5 * float(nodes[6][1] + nodes[6][2]), np.nan]
    u[7, 3] = np.nan
    host = tt.sample_real(u, nodes, cond)
    t = torch.from_numpy(u).to("cuda:0")
    dev = tt.sample_real(t, nodes, cond)
    lin = [("linear", q) for q in nodes]
    res = dict(is_cuda=all(bool(v.is_cuda) for v in dev.values()), dtypes=[str(dev[k].dtype) for k in NAMES],
               equal=all(dev[k].cpu().numpy().tobytes() == host[k].tobytes() for k in NAMES),
               failed=tt.sample_real_last()["failed"], only_x=sorted(tt.sample_real(t, nodes, cond, want=("x",))),
               chain=bool(np.array_equal(tt.basis_batch(dev["x"][:7].contiguous(), lin, "exact").cpu().numpy(), host["val"][:7])),
               empty=list(tt.sample_real(t[:0].contiguous(), nodes)["x"].shape))
    try:
        tt.sample_real(t.to(torch.float32), nodes)
        res["float32_refused"] = False
    except ValueError:
        res["float32_refused"] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
