"""The two exact integrand evaluators of the cluster sweep kernel (ttx_cluster.h) against the oracle, bit for bit.

k_sweep_cluster<false, true> stages the value rows padded to whole chunks of 8 with neutral elements (0.0 behind the nodes in
processing order, 1.0 behind the weights) and walks them with f_ising_c4w, whose chains have no remainder and no test;
k_sweep_cluster<false, false> keeps the predicated remainders of f_ising_c4p (TTX_CL_PAD=0, or any node outside [0,1], where
the pad would not be neutral).  Ising C_m has d = m - 1 dimensions; at bond p the left row holds p - 1 and the right row
d - p - 1 entries, so C_10, C_17, C_18 and C_33 together meet every residue modulo 8 on either side, the lengths 0, 1, 7, 8, 9
among them (checked below without a GPU)."""
import numpy as np
import pytest

import oracle_lib as O
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

# (m, n, r, piv, bond groups): small modes and ranks; one and several groups; every case runs >= 2 sweeps (both directions)
CASES = [(10, 9, 8, 2, 1), (10, 5, 6, 1, 3), (17, 9, 8, 2, 1), (17, 7, 8, 3, 4), (18, 9, 8, 2, 2), (18, 5, 6, 2, 1), (33, 9, 8, 2, 1), (33, 7, 6, 2, 4)]
IDS = [f"C{c[0]}_n{c[1]}_r{c[2]}_p{c[3]}_g{c[4]}" for c in CASES]
EVAL = {"0": "predicated", "1": "chunks"}


def _lengths(m):
    d = m - 1
    return [(p - 1, d - p - 1) for p in range(1, d)]


def test_cases_cover_every_chain_length_residue():
    left = {a for c in CASES for a, _ in _lengths(c[0])}
    right = {b for c in CASES for _, b in _lengths(c[0])}
    for side in (left, right):
        assert {x % 8 for x in side} == set(range(8))
        assert {0, 1, 7, 8, 9} <= side


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


def _run(s, r, piv, ng, want_eval):
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=ng)
    assert tt.sweep_path() == "cluster" and tt.arith == "exact"
    assert tt.cluster_eval() == want_eval
    tt.run()
    assert tt.cluster_fallbacks == 0 and tt.cluster_eval() == want_eval
    oo = O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=ng)
    _identical(tt, oo)
    assert tt.quad(s["quad"]) == oo["value"]


@pytest.mark.gpu
@pytest.mark.parametrize("pad", ["0", "1"])
@pytest.mark.parametrize("m,n,r,piv,ng", CASES, ids=IDS)
def test_cluster_chunk_evaluators_bit_exact(monkeypatch, m, n, r, piv, ng, pad):
    monkeypatch.setenv("TTX_SWEEP", "cluster")
    monkeypatch.setenv("TTX_CL_PAD", pad)
    _run(D.ising_setup("c", m, n), r, piv, ng, EVAL[pad])


@pytest.mark.gpu
def test_padded_evaluator_is_the_default(monkeypatch):
    monkeypatch.setenv("TTX_SWEEP", "cluster")
    monkeypatch.delenv("TTX_CL_PAD", raising=False)
    _run(D.ising_setup("c", 17, 9), 8, 2, 2, "chunks")


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [None, "1"])
@pytest.mark.parametrize("node", [1.0625, -0.03125])
def test_node_outside_unit_interval_takes_the_predicated_evaluator(monkeypatch, pad, node):
    """0.0 is a neutral pad only while the running products are finite, which the host guarantees by nodes in [0,1]: with one
    node outside, the engine keeps the predicated evaluator whatever TTX_CL_PAD asks for, and stays bit-exact."""
    monkeypatch.setenv("TTX_SWEEP", "cluster")
    if pad is None:
        monkeypatch.delenv("TTX_CL_PAD", raising=False)
    else:
        monkeypatch.setenv("TTX_CL_PAD", pad)
    s = D.ising_setup("c", 18, 9)
    s["par"] = s["par"].copy()
    s["par"][8 if node > 1 else 0] = node
    s["tru"] = None
    _run(s, 8, 2, 2, "predicated")


@pytest.mark.gpu
def test_bad_pad_switch_is_refused(monkeypatch):
    monkeypatch.setenv("TTX_CL_PAD", "yes")
    s = D.ising_setup("c", 10, 9)
    with pytest.raises(E.TTXError, match="TTX_CL_PAD"):
        E.TTCross(s["n"], s["fun_id"], s["par"], 8, pivoting=2, accuracy=s["acc"], quad=s["quad"])
