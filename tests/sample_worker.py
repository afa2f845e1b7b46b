"""Child of test_gpu_sample.py, in a process of its own.
  chunk NAME : the samples of case NAME under whatever TTX_SAMPLE_CHUNK the parent set; prints a digest of ind, logq, val
  dev        : the device-pointer entry (ttx_sample_dev) with torch tensors against the host entry -- torch brings a HIP runtime
               of its own and has to initialise its device before the engine's library does (tijk_dev_worker.py)
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
    import sample_ref as S
    from ttcross_amd import engine as E
    if what == "chunk":
        cores, u, w = S.case(sys.argv[2])
        tt = E.TTCross.from_cores(cores)
        print(json.dumps(dict(digest=digest(tt.sample(u, w)), failed=tt.sample_last()["failed"])))
        return
    cores, u, w = S.case("d8_unequal")
    tt = E.TTCross.from_cores(cores)
    fixed = [0, 0, 1, 0, 0, 0, 2, 0]
    u[7, 3] = np.nan
    host = tt.sample(u, w, fixed)
    t = torch.from_numpy(u).to("cuda:0")
    dev = tt.sample(t, w, fixed)
    res = dict(is_cuda=all(bool(v.is_cuda) for v in dev.values()), dtypes=[str(dev[k].dtype) for k in ("ind", "logq", "val")],
               equal=all(dev[k].cpu().numpy().tobytes() == host[k].tobytes() for k in ("ind", "logq", "val")),
               failed=tt.sample_last()["failed"], only_ind=sorted(tt.sample(t, w, fixed, want=("ind",))),
               chain=bool(np.array_equal(tt.tijk_batch(dev["ind"][:7].contiguous(), "exact").cpu().numpy(), host["val"][:7])),
               empty=list(tt.sample(t[:0].contiguous(), w)["ind"].shape))
    try:
        tt.sample(t.to(torch.float32), w)
        res["float32_refused"] = False
    except ValueError:
        res["float32_refused"] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
