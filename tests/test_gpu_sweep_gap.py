"""The stretch between the last bond step of one sweep and the first of the next in its new forms against the old ones: the tail
launch's event as the launch's own completion signal (TTX_TAIL_EVENT=kernel), boundary blocks that request their header words
together and evaluate the corner of Ising C over staged values (TTX_TAIL_LEAN), and the cluster kernel's exit with the left-going
message packed on workgroup 1 (TTX_CL_PACK2).  One fresh child process per problem (tests/sweep_gap_worker.py) runs it with all
three in the old form, with the defaults and with each switch alone; everything a run leaves -- all cores, ranks, the per-sweep records (val, erank, neval, amax, pivotmax, pivotmin), tapes, the
evaluation count and the integral -- is compared BYTE FOR BYTE between the forms, and the launches per kind are the same in all.

Shapes, the smallest at which these paths can go wrong: Ising C_6 (n = 33, r = 20, piv = 2: the first sweep has boundary rank 1,
20 x 20 LU entries are more than one per thread) in 1, 2 and 4 groups, whose end groups have one neighbour; groups of a single bond
(first == last: both messages and both boundary sides concern the same bond) -- C_5 in three groups, whose middle group has both
neighbours, and C_4 in two (Ising C_m has m - 1 dimensions and m - 2 bonds, and the engine, like the reference, wants fewer groups
than dimensions: three groups of one bond each need C_5); clusters of 1, 2 and 8 workgroups; the chain path (k_exch_boundary and
k_exch_pack); TTX_ARITH=fast; two runs on one engine; Ising D_6, whose corner evaluators stay as they are."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from ttcross_amd import drivers as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "sweep_gap_worker.py")
CLEARED = ("TTX_TAIL_EVENT", "TTX_TAIL_LEAN", "TTX_CL_PACK2", "TTX_TAIL", "TTX_TAIL_SIDE", "TTX_SWEEP", "TTX_ARITH", "TTX_PIPELINE",
           "TTX_CLUSTER_TEST_ABORT", "TTX_CLUSTER_COOP", "TTX_CLUSTER_NB", "TTX_CL_PAD", "TTX_CL_POWTAB", "TTX_CL_WORD", "TTX_CL_LISTS")
FORMS = ("old", "new", "only_tail_event", "only_tail_lean", "only_cl_pack2")
#                    tail event by kernel (either: a runtime may refuse the extended launch), lean, pack2
WANTED = {"old": (0, 0, 0), "new": (1, 1, 1), "only_tail_event": (1, 0, 0), "only_tail_lean": (0, 1, 0), "only_cl_pack2": (0, 0, 1)}


def _worker(tmp_path, tag, family, m, n, r, piv, groups, arith="exact", runs=1, env=None):
    out = str(tmp_path / f"{tag}.npz")
    e = {k: v for k, v in os.environ.items() if k not in CLEARED}
    e.update(env or {})
    argv = [sys.executable, WORKER, out, family] + [str(x) for x in (m, n, r, piv, groups, arith, runs)]
    p = subprocess.run(argv, capture_output=True, text=True, env=e, timeout=300)
    assert p.returncode == 0 and "WORKER OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    return dict(np.load(out))


def _same_bytes(x, ta, tb):
    """every array of run `ta` == the same array of run `tb`, as bytes (dtype and shape included)"""
    names = sorted(k[len(ta):] for k in x if k.startswith(ta))
    assert names == sorted(k[len(tb):] for k in x if k.startswith(tb)) and any(k.startswith("core") for k in names)
    for k in names:
        a, b = x[ta + k], x[tb + k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{k} differs between {ta} and {tb}"


def _forms_agree(x, path=None, runs=1):
    for form in FORMS:
        if path:
            assert x[form + "_path"][0] == path
        assert x[form + "_path"][0] == x["old_path"][0] and x[form + "_arith"][0] == x["old_arith"][0] and int(x[form + "_fallbacks"][0]) == 0
        for k in range(runs):
            _same_bytes(x, "old_run0_", f"{form}_run{k}_")
            assert x[f"{form}_entry{k}"].tobytes() == x["old_entry0"].tobytes()
        assert all(int(x[f"{form}_launches_{kind}"][0]) == int(x[f"old_launches_{kind}"][0]) for kind in ("other", "halfstep", "exchange", "quad"))
        # the engine says which form it used: the event by the kernel only where asked for, and where the runtime refused the extended
        # launch the engine says that too (marker, with the refusals counted)
        by_kernel, refused, *rest = (int(v) for v in x[form + "_gap"])
        assert tuple(rest) == WANTED[form][1:]
        if WANTED[form][0]:
            assert (by_kernel, refused) == (1, 0) or (by_kernel == 0 and refused >= 1)
        else:
            assert (by_kernel, refused) == (0, 0)
    return x


def _against_the_oracle(x, s, r, piv, groups):
    oo = O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=groups)
    d = len(s["n"])
    for form in ("old", "new"):
        t = form + "_run0_"
        assert np.array_equal(x[t + "tapes"][:, 1:d], oo["tapes"][:, 1:d])
        assert [int(v) for v in x[t + "sw_neval"]] == [b["neval"] for b in oo["sweeps"]]
        assert [float(v) for v in x[t + "sw_val"]] == [b["val"] for b in oo["sweeps"]]
        assert int(x[t + "neval"][0]) == oo["neval"] and np.array_equal(x[t + "ranks"], oo["r"])
        assert all(np.array_equal(x[f"{t}core{k}"], oo["cores"][k - 1]) for k in range(1, d + 1))
        assert float(x[t + "quad"][0]) == oo["value"]


@pytest.mark.parametrize("groups", [1, 2, 4])
def test_ising_c6_on_the_cluster_path(tmp_path, groups):
    """Ising C_6, n = 33, r = 20, piv = 2; two groups also against the oracle, bit for bit"""
    x = _forms_agree(_worker(tmp_path, f"c6_g{groups}", "c", 6, 33, 20, 2, groups, env={"TTX_SWEEP": "cluster"}), "cluster")
    assert len(x["new_run0_sw_it"]) > 2 and max(int(v) for v in x["new_run0_ranks"]) > 16
    if groups == 2:
        _against_the_oracle(x, D.ising_setup("c", 6, 33), 20, 2, groups)


@pytest.mark.parametrize("m,groups", [(5, 3), (4, 2)])
def test_groups_of_one_bond(tmp_path, m, groups):
    """first == last in every group: C_5 in three groups (the middle one has both neighbours), C_4 in two"""
    x = _forms_agree(_worker(tmp_path, f"c{m}_g{groups}", "c", m, 33, 20, 2, groups, env={"TTX_SWEEP": "cluster"}), "cluster")
    assert len(x["new_run0_ranks"]) == m and len(x["new_run0_sw_it"]) > 2


@pytest.mark.parametrize("nb", [1, 2, 8])
def test_cluster_sizes(tmp_path, nb):
    """C_6 in two groups with TTX_CLUSTER_NB = 1 (no workgroup 1: the engine leaves the cluster path), 2 (workgroup 1 is the last) and 8"""
    x = _forms_agree(_worker(tmp_path, f"c6_nb{nb}", "c", 6, 33, 20, 2, 2, env={"TTX_CLUSTER_NB": str(nb)}), "cluster" if nb > 1 else None)
    assert len(x["new_run0_sw_it"]) > 2


def test_chain_path(tmp_path):
    """TTX_SWEEP=chain: the boundary blocks of k_exch_boundary (flag, rank and index from upd, r and the tables) and k_exch_pack"""
    _forms_agree(_worker(tmp_path, "c6_chain", "c", 6, 33, 20, 2, 2, env={"TTX_SWEEP": "chain"}), "chain")


def test_fast_arithmetic(tmp_path):
    """TTX_ARITH=fast (the closed form inside the cluster kernel): the forms against each other"""
    x = _forms_agree(_worker(tmp_path, "c6_fast", "c", 6, 33, 20, 2, 2, arith="fast"), "cluster")
    assert x["new_arith"][0] == "fast"


def test_two_runs_on_one_engine(tmp_path):
    """the second run's first launch rebuilds its lists and its generator word; every later launch of either run takes the carried ones"""
    x = _forms_agree(_worker(tmp_path, "c6_twice", "c", 6, 33, 20, 2, 2, runs=2), "cluster", runs=2)
    sweeps = len(x["new_run0_sw_it"]) - 1
    assert sweeps > 2 and [int(v) for v in x["new_entry1"]] == [sweeps - 1, sweeps - 1]


def test_ising_d6(tmp_path):
    """Ising D_6, n = 17, r = 8 in two groups: corner evaluators the lean boundary blocks leave alone"""
    _forms_agree(_worker(tmp_path, "d6", "d", 6, 17, 8, 2, 2))
