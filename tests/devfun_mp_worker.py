"""One rank of a multi-process job with a LOADED device integrand (TTX_FUN_DEVICE) over the shared-memory transport; several
ranks share one GPU.  Every rank loads the code object itself, runs its bond groups, and compares the job with the same problem
run as ONE process in this worker (tapes, sweep records, the cores it holds, integral); then dtt_accchk on the multi-process
engine (collective; works on a replica that shares the module) against the one-process engine.

    RANK=r WORLD_SIZE=W TTX_SHM_NAME=x python tests/devfun_mp_worker.py D N R PIV NGROUPS
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
    d, n, r, piv, ng = (int(a) for a in sys.argv[1:6])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    s = U.user_setup(d, n)
    co = os.path.join(U.BUILD, "rational.hsaco")           # built by the test before the ranks start
    tt = E.TTCross(s["n"], E.TTX_FUN_DEVICE, [], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], nproc=ng, world_rank=rank, world_size=world)
    tt.set_integrand_device(co, "rational", s["par"])
    tt.comm_init_shm(os.environ.get("TTX_SHM_NAME", "ttx_devfun"))
    tt.run()
    val = tt.quad(s["quad"])
    one = E.TTCross(s["n"], E.TTX_FUN_DEVICE, [], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], nproc=ng)
    one.set_integrand_device(co, "rational", s["par"]).run()
    bad = []
    if not np.array_equal(tt.tapes()[:, 1:tt.d], one.tapes()[:, 1:tt.d]):
        bad.append("tapes")
    for a, b in zip(tt.sweeps(), one.sweeps()):
        for f in ("neval", "erank", "val", "amax", "pivotmax"):
            if a[f] != b[f]:
                bad.append(f"sweep{a['it']}.{f}")
    if len(tt.sweeps()) != len(one.sweeps()) or tt.neval != one.neval or not np.array_equal(tt.ranks(), one.ranks()):
        bad.append("neval/ranks/nsweeps")
    if val != one.quad(s["quad"]):
        bad.append("value")
    L = E.load_library()
    for k in range(1, tt.d + 1):
        if L.ttx_core_size(tt._h, k) > 0 and not np.array_equal(tt.core(k), one.core(k)):
            bad.append(f"core{k}")
    a1, a2 = tt.accchk(500), one.accchk(500)
    if any(a1[k] != a2[k] for k in ("einf", "efro", "ainf", "afro")) or not np.array_equal(a1["pivot"], a2["pivot"]):
        bad.append(f"accchk {a1} vs {a2}")
    if tt.host_calls != 0:
        bad.append("host_calls")
    print(f"[rank {rank}/{world}] groups={ng} value={val:.16e} neval={tt.neval} {'OK' if not bad else 'MISMATCH ' + '; '.join(bad[:6])}", flush=True)
    one.close()
    tt.close()
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
