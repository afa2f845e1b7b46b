"""One run with a device integrand that returns NaN (everywhere / on part of the domain), in a process of its own with its own
time limit (tests/test_gpu_devfun.py), as tests/nan_worker.py does for the built-in integrands.  Input robustness with ordinary
arithmetic: the run must end, every pivot in range.

    python tests/devfun_nan_worker.py NAME PIV NPROC        NAME = rational_nan | rational_partnan
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import devfun_util as U
    from ttcross_amd import engine as E
    name, piv, nproc = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    d, n, r = 5, 5, 4
    s = U.user_setup(d, n)
    tt = E.TTCross(s["n"], E.TTX_FUN_DEVICE, [], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], nproc=nproc)
    tt.set_integrand_device(os.path.join(U.BUILD, "rational.hsaco"), name, s["par"]).run()
    tp = tt.tapes()
    act = tp[:, 1:tt.d, :]
    ok = tp.shape[0] >= 1 and bool(((act == -1) | ((act >= 1) & (act <= max(n, r + 1)))).all()) and all(1 <= rk <= r for rk in tt.ranks())
    # the host-callback engine with the C twin takes the same decisions
    hh = E.TTCross(s["n"], E.TTX_FUN_HOST, [], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], nproc=nproc)
    hh.set_integrand_host(U.twin_addr("ttx_devfun_" + name), s["par"]).run()
    same = np.array_equal(tp, hh.tapes()) and np.array_equal(tt.ranks(), hh.ranks())
    print(f"{name} piv={piv} nproc={nproc} sweeps={tp.shape[0]} ranks_max={int(max(tt.ranks()))} same_as_host={same} {'OK' if ok and same else 'BAD'}", flush=True)
    tt.close()
    hh.close()
    sys.exit(0 if ok and same else 1)


if __name__ == "__main__":
    main()
