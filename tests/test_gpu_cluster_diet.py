"""The glue of the cluster sweep kernel (ttx_cluster.h) at the smallest shapes at which each of its shortened parts can go
wrong, bit for bit against the oracle (Ising C, exact arithmetic, TTX_SWEEP=cluster, no fallback to the chain path):

* pivoting 0..3: the turn that ends a full rook search stores only its running-maximum record and takes no part in an
  arg-max exchange (H = 2, 4, 6 half-steps); pivoting 0 keeps both of its exchanges;
* fewer modes than workgroups: some workgroups own no mode index, their slices (cl_slice) are empty and one wave of
  them (cl_wact) still takes part in every exchange;
* TTX_CLUSTER_NB 2, 3, 8, 16: the slices and the record slots at every cluster width, both exact evaluators;
* a rank above 32: the one-solve-per-wave paths of the append (roles C and D);
* fast arithmetic: the closed-form instantiation shares the glue; against the chain path by the tolerances of test_gpu_fast.py.
"""
import numpy as np
import pytest

import oracle_lib as O
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

pytestmark = pytest.mark.gpu

_ORACLE = {}


def _oracle(m, n, r, piv, ng):
    """One oracle run per shape, shared by the cases that differ only in how the engine is configured."""
    key = (m, n, r, piv, ng)
    if key not in _ORACLE:
        s = D.ising_setup("c", m, n)
        _ORACLE[key] = O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=ng)
    return _ORACLE[key]


def _identical(tt, oo):
    gs, os_ = tt.sweeps(), oo["sweeps"]
    assert len(gs) == len(os_) and len(gs) >= 3, "two sweeps (one per direction) behind the initial one"
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d]), "pivot tapes differ"
    for a, b in zip(gs, os_):
        assert a["neval"] == b["neval"] and a["erank"] == b["erank"], f"sweep {a['it']}"
        assert a["val"] == b["val"], f"sweep {a['it']}: val {a['val']!r} vs {b['val']!r}"
        assert a["amax"] == b["amax"] and a["pivotmax"] == b["pivotmax"], f"sweep {a['it']}"
    assert tt.neval == oo["neval"] and np.array_equal(tt.ranks(), oo["r"])
    for k in range(1, tt.d + 1):
        assert np.array_equal(tt.core(k), oo["cores"][k - 1]), f"core {k} differs"


def _run(monkeypatch, m, n, r, piv, ng, nb=None, pad=None):
    monkeypatch.setenv("TTX_SWEEP", "cluster")
    for name, v in (("TTX_CLUSTER_NB", nb), ("TTX_CL_PAD", pad)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(v))
    s = D.ising_setup("c", m, n)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=ng)
    assert tt.sweep_path() == "cluster" and tt.arith == "exact"
    assert tt.cluster_eval() == ("predicated" if pad == 0 else "chunks")
    tt.run()
    assert tt.cluster_fallbacks == 0
    oo = _oracle(m, n, r, piv, ng)
    _identical(tt, oo)
    assert tt.quad(s["quad"]) == oo["value"]
    return tt


@pytest.mark.parametrize("ng", [1, 3])
@pytest.mark.parametrize("piv", [0, 1, 2, 3])
def test_every_pivoting_depth_bit_exact(monkeypatch, piv, ng):
    _run(monkeypatch, 10, 9, 8, piv, ng)


@pytest.mark.parametrize("n,r,nb,ng", [(5, 6, 8, 2), (3, 4, 4, 1)], ids=["n5_nb8", "n3_nb4"])
def test_fewer_modes_than_workgroups_bit_exact(monkeypatch, n, r, nb, ng):
    _run(monkeypatch, 10, n, r, 2, ng, nb=nb)


@pytest.mark.parametrize("nb,pad", [(2, None), (3, 1), (3, 0), (8, None), (16, None)], ids=["nb2", "nb3_pad1", "nb3_pad0", "nb8", "nb16"])
def test_every_cluster_width_bit_exact(monkeypatch, nb, pad):
    _run(monkeypatch, 17, 9, 8, 2, 2, nb=nb, pad=pad)


def test_rank_above_32_bit_exact(monkeypatch):
    tt = _run(monkeypatch, 10, 9, 40, 2, 1)
    assert tt.ranks().max() > 32, "roles C and D take the one-solve-per-wave path only above rank 32"


def test_fast_arithmetic_tracks_the_chain_path(monkeypatch):
    s = D.ising_setup("c", 17, 9)

    def engine(path):
        monkeypatch.setenv("TTX_SWEEP", path)
        return E.TTCross(s["n"], s["fun_id"], s["par"], 8, pivoting=2, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=2, arith="fast")

    a, b = engine("chain"), engine("cluster")
    assert a.sweep_path() == "chain" and b.sweep_path() == "cluster"
    assert b.arith == "fast" and b.cluster_eval() == "closed"
    a.run(), b.run()
    assert b.cluster_fallbacks == 0
    ra, rb = a.sweeps(), b.sweeps()
    assert len(ra) == len(rb) and len(rb) >= 3
    lead = min(4, len(ra) - 1)
    assert np.array_equal(a.tapes()[:lead, 1:a.d], b.tapes()[:lead, 1:a.d]), "pivots of the leading sweeps differ"
    for x, y in zip(ra[:lead + 1], rb[:lead + 1]):
        assert abs(x["val"] - y["val"]) <= 1e-11 * abs(x["val"]), f"sweep {x['it']}"
        assert abs(x["neval"] - y["neval"]) <= 0.02 * x["neval"]
    va, vb = a.quad(s["quad"]), b.quad(s["quad"])
    assert abs(va - vb) <= 1e-12 * abs(va)
