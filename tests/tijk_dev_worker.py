"""Child of test_gpu_tijk_batch.py: the device-pointer entry (ttx_ijk_batch_dev) with torch tensors against the host-pointer
entry, in a process of its own -- torch brings a HIP runtime of its own and has to initialise its device before the engine's
library does.  Prints one JSON line."""
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
    n, r = [4] * 5, [1, 65, 65, 65, 65, 1]
    tt = E.TTCross.from_cores(R.rand_train(8, n, r))
    rng = np.random.default_rng(13)
    ind = np.ascontiguousarray((rng.integers(0, 2 ** 31 - 1, (2002, 5)) % 4 + 1).astype(np.int32))
    ind[5, 2] = 0
    host = tt.tijk_batch(ind, mode)
    calls = tt.host_calls
    t = torch.from_numpy(ind).to("cuda:0")
    out = tt.tijk_batch(t, mode)
    res = dict(is_cuda=bool(out.is_cuda), dtype=str(out.dtype), equal=bool(np.array_equal(out.cpu().numpy(), host)), invalid=float(host[5]),
               host_calls_unchanged=tt.host_calls == calls, empty=list(tt.tijk_batch(t[:0].contiguous(), mode).shape),
               single=float(tt.tijk(ind[0])), first=float(host[0]))
    try:
        tt.tijk_batch(t.to(torch.int64), mode)
        res["int64_refused"] = False
    except ValueError:
        res["int64_refused"] = True
    if torch.cuda.device_count() > 1:                  # a tensor on another device than the engine's is refused, not passed on
        try:
            tt.tijk_batch(t.to("cuda:1"), mode)
            res["other_device_refused"] = False
        except ValueError:
            res["other_device_refused"] = True
    print(json.dumps(res))


if __name__ == "__main__":
    main()
