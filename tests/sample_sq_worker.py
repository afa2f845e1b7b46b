"""Child of test_gpu_sample_sq.py, in a process of its own.
  chunk NAME MODE : the samples of case NAME (signed) under whatever TTX_SAMPLE_CHUNK the parent set; prints a digest of ind, logq, val
  dev             : the device-pointer entry (ttx_sample_sq_dev) with torch tensors against the host entry -- torch brings a HIP
                    runtime of its own and has to initialise its device before the engine's library does (tijk_dev_worker.py)
  nan             : a NaN and an Inf in a core, both modes: the range of the indices written and the count of failed samples
Prints one JSON line."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digest(res):
    return hashlib.sha256(res["ind"].tobytes() + res["logq"].tobytes() + res["val"].tobytes()).hexdigest()


def main():
    what = sys.argv[1]
    if what == "dev":
        import torch
        torch.cuda.init()
    import sample_sq_ref as Q
    from ttcross_amd import engine as E
    if what == "chunk":
        cores, u, w = Q.case(sys.argv[2], True)
        tt = E.TTCross.from_cores(cores)
        print(json.dumps(dict(digest=digest(tt.sample_sq(u, w, gamma=0.125, mode=sys.argv[3])), failed=tt.sample_sq_last()["failed"])))
        return
    if what == "nan":
        cores, u, w = Q.case("d3", True)
        u = u[:500]
        n = np.array([c.shape[1] for c in cores])
        out = {}
        for tag, bad in (("nan", np.nan), ("inf", np.inf)):
            cs = [c.copy() for c in cores]
            cs[1][1, 4, 0] = bad
            tt = E.TTCross.from_cores(cs)
            for mode in ("exact", "mfma"):
                res = tt.sample_sq(u, w, mode=mode)
                failed = np.all(res["ind"] == 0, axis=1)
                out[tag + "_" + mode] = dict(in_range=bool(np.all(res["ind"] >= 0) and np.all(res["ind"] <= n[None, :])),
                                             whole_rows=bool(np.all((res["ind"] > 0)[~failed])), failed=int(failed.sum()),
                                             counted=tt.sample_sq_last()["failed"],
                                             marked=bool(np.all(np.isnan(res["logq"][failed])) and np.all(res["val"][failed] == 0.0)))
        print(json.dumps(out))
        return
    cores, u, w = Q.case("d8_unequal", True)
    tt = E.TTCross.from_cores(cores)
    fixed = [0, 0, 1, 0, 0, 0, 2, 0]
    u[7, 3] = np.nan
    res = {}
    for mode in ("exact", "mfma"):
        host = tt.sample_sq(u, w, fixed, 0.125, mode)
        t = torch.from_numpy(u).to("cuda:0")
        dev = tt.sample_sq(t, w, fixed, 0.125, mode)
        res[mode] = dict(is_cuda=all(bool(v.is_cuda) for v in dev.values()), dtypes=[str(dev[k].dtype) for k in ("ind", "logq", "val")],
                         equal=all(dev[k].cpu().numpy().tobytes() == host[k].tobytes() for k in ("ind", "logq", "val")),
                         failed=tt.sample_sq_last()["failed"], only_ind=sorted(tt.sample_sq(t, w, fixed, 0.125, mode, want=("ind",))),
                         chain=bool(np.array_equal(tt.tijk_batch(dev["ind"][:7].contiguous(), "exact").cpu().numpy(), host["val"][:7])),
                         empty=list(tt.sample_sq(t[:0].contiguous(), w)["ind"].shape))
    try:
        tt.sample_sq(t.to(torch.float32), w)
        res["float32_refused"] = False
    except ValueError:
        res["float32_refused"] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
