"""COS-coefficient tensor (test_crs_coscoeff.f90, n = 65, r = 20, piv = 1): the host callback (the C restatement
tests/coscoeff_fun.c on 16 threads, the path calc_coefficient took before TTX_FUN_COSCOEFF) against the device integrand.
Prints per d the wall time of each run (ttx_seconds), neval, the host calls, and whether both runs give identical cores.

    python profiles/probes/coscoeff_speed.py [d ...]          (default 6 8 10 12)
"""
import os
import sys

os.environ["TTX_HOST_THREADS"] = "16"         # the host pool is sized once per process
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import coscoeff_util as CU  # noqa: E402
from ttcross_amd import drivers as D  # noqa: E402
from ttcross_amd import engine as E  # noqa: E402


def main():
    ds = [int(x) for x in sys.argv[1:]] or [6, 8, 10, 12]
    n, r, piv = 65, 20, 1
    print("%3s %12s %12s %10s %12s %12s %8s %s" % ("d", "host_s", "device_s", "speedup", "neval", "host_calls", "sweeps", "identical"), flush=True)
    for d in ds:
        s = D.coscoeff_setup(d, n)
        dev = E.TTCross(s["n"], E.TTX_FUN_COSCOEFF, [], r, pivoting=piv, accuracy=s["acc"], aux=s["aux"])
        dev.run()          # first run: module load and allocations; the timed run follows
        dev.run()
        host = E.TTCross(s["n"], E.TTX_FUN_HOST, [], r, pivoting=piv, accuracy=s["acc"])
        host.set_integrand_host(CU.fun_addr(), s["aux"]).run()
        same = (dev.neval == host.neval and np.array_equal(dev.ranks(), host.ranks()) and
                all(np.array_equal(dev.core(k), host.core(k)) for k in range(1, d + 1)))
        print("%3d %12.4f %12.4f %10.1f %12d %12d %8d %s" % (d, host.seconds, dev.seconds, host.seconds / dev.seconds, dev.neval,
                                                          host.host_calls, len(dev.sweeps()), same), flush=True)
        dev.close()
        host.close()


if __name__ == "__main__":
    main()
