"""One rank of a COS-coefficient job split over several engine processes on one GPU (the built-in shared-memory transport, no
torch): the job is checked against the oracle with the same number of bond groups running the C restatement.  Exit code != 0 on
any mismatch.

    RANK=r WORLD_SIZE=W TTX_SHM_NAME=x python tests/coscoeff_mp_worker.py D N R PIV NGROUPS
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    d, n, r, piv, ng = (int(x) for x in sys.argv[1:6])
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import coscoeff_util as CU
    import oracle_lib as O
    from ttcross_amd import drivers as D
    from ttcross_amd import engine as E
    s = D.coscoeff_setup(d, n)
    tt = E.TTCross(s["n"], E.TTX_FUN_COSCOEFF, [], r, pivoting=piv, accuracy=s["acc"], aux=s["aux"], nproc=ng,
                   world_rank=rank, world_size=world)
    tt.comm_init_shm(os.environ.get("TTX_SHM_NAME", "ttx_cc_test"))
    tt.run()
    oo = O.dmrgg(s["n"], E.TTX_FUN_HOST, s["aux"], r, piv=piv, accuracy=s["acc"], nproc=ng, user=CU.fun_addr())
    bad = []
    if not np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d]):
        bad.append("tapes")
    if [(a["neval"], a["erank"], a["amax"], a["pivotmax"]) for a in tt.sweeps()] != \
            [(b["neval"], b["erank"], b["amax"], b["pivotmax"]) for b in oo["sweeps"]]:
        bad.append("sweeps")
    if tt.neval != oo["neval"] or not np.array_equal(tt.ranks(), oo["r"]) or tt.host_calls != 0:
        bad.append("neval / ranks / host_calls")
    L = E.load_library()
    held = 0
    for k in range(1, tt.d + 1):
        if L.ttx_core_size(tt._h, k) > 0:
            held += 1
            if not np.array_equal(tt.core(k), oo["cores"][k - 1]):
                bad.append(f"core{k}")
    print(f"[rank {rank}/{world}] groups={ng} neval={tt.neval} cores_held={held} " + ("OK" if not bad else "BAD " + " ".join(bad)))
    tt.close()
    sys.exit(1 if bad or held == 0 else 0)


if __name__ == "__main__":
    main()
