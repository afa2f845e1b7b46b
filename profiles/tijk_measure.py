"""Measurement of the batched element evaluation: python profiles/tijk_measure.py WORKLOAD [NPTS,NPTS,...]

Per workload (c64 | d64 | rand256, see ttcross_amd.drivers.tijk_train): every cell npts x {exact, mfma} through the
device-pointer entry (indices drawn on the device, outputs left there; one warm-up, 5 repeats, median), then the baselines on
the first 1000 points: a loop of single ttx_ijk calls (time per element) and the oracle's ttxo_tt_ijk on one host thread.
One JSON line per measurement."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import torch
    torch.cuda.init()
    from ttcross_amd import drivers as D
    workload = sys.argv[1]
    sizes = [int(float(x)) for x in (sys.argv[2] if len(sys.argv) > 2 else "1e3,1e5,1e6").split(",")]
    tt = D.tijk_train(workload)
    r = tt.ranks()
    first = None
    for npts in sizes:
        for mode in ("exact", "mfma"):
            _, ind, out, res = D.run_tijk([workload, str(npts), mode], tt=tt)
            # state traffic of the MFMA path (read + write of 8 r bytes per point and mode) and fp64 matrix work (2 r0 r1 per point and mode)
            if mode == "exact":           # the two rates below describe the MFMA path's traffic and work only
                if first is None:
                    first = ind[:1000].cpu().numpy()
                continue
            res["state_GBps"] = 16.0 * float(r[1:-1].sum()) * npts / (res["ms"] * 1e-3) / 1e9
            res["TFLOPs"] = 2.0 * float((r[:-2] * r[1:-1]).sum()) * npts / (res["ms"] * 1e-3) / 1e12
            print(json.dumps({k: res[k] for k in ("workload", "npts", "mode", "state_GBps", "TFLOPs")}))
    t0 = time.perf_counter()
    single = np.array([tt.tijk(row) for row in first])
    t_single = time.perf_counter() - t0
    t0 = time.perf_counter()
    batch = tt.tijk_batch(first, "exact")
    t_batch = time.perf_counter() - t0
    print(json.dumps(dict(workload=workload, baseline="1000 single ttx_ijk calls", ms=t_single * 1e3, us_per_element=t_single * 1e3,
                          batch_exact_host_entry_ms=t_batch * 1e3, ratio=t_single / t_batch,
                          max_rel_diff=float(np.max(np.abs(single - batch) / np.maximum(np.abs(batch), 1e-300))))))
    import oracle_lib as O
    ot = O.OracleTT([tt.core(k) for k in range(1, tt.d + 1)])
    t0 = time.perf_counter()
    ref = np.array([ot.ijk(row) for row in first])
    t_or = time.perf_counter() - t0
    print(json.dumps(dict(workload=workload, baseline="oracle ttxo_tt_ijk, one host thread, 1000 points", ms=t_or * 1e3, us_per_element=t_or * 1e3,
                          identical_to_exact=bool(np.array_equal(ref, batch)))))


if __name__ == "__main__":
    main()
