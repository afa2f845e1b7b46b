"""What a launch of the cluster sweep kernel (ttx_cluster.h) carries to the next one instead of recomputing it at its entry -- the
generator's jump powers from a compile-time table (TTX_CL_POWTAB), the generator word (TTX_CL_WORD) and the sorted pivot lists of
every own bond (TTX_CL_LISTS) -- bit for bit against the oracle and against the form with all three switched off (the entry as it
was: three square-and-multiply loops, the word raised from rngpos, the lists rebuilt from vip), at the smallest shapes at which
carried state can go wrong: Ising C with d = 8 in two bond groups of 3 and 4 own bonds, exact arithmetic, TTX_SWEEP=cluster.

* seven sweeps: launch 1 rebuilds, launch 2 loads what a rebuilding launch extended, launches 3 .. 7 load what a loading launch
  extended, in both directions (the image is indexed by bond, not by step);
* n = 3: the outer bonds reach their rank limit 3 in sweep 2 and accept nothing in the five launches behind it, while the lists
  of the inner bonds go on growing;
* two run() calls on one engine: the tag of the first run's last launch must not reach the second run's first launch;
* TTX_PIPELINE=0: the plain loop, with the sweep's other kernels and a host wait between two launches;
* each of the three switches off alone.
ttx_cluster_entry counts the launches of a run that took the carried lists and the carried word: all but the first where the form is
on, none where it is off -- so a form that silently fell back to the rebuild would not pass.

A pivot row or column that repeats within a bond (fewer distinct entries than the rank) does not occur in a run: the new pivot's
residual vanishes on every pivot row and column the bond already has, and a search over the oracle's runs of d = 8, n = 3, 5, 9,
pivoting 0 .. 3, maxrank 6, 12, 20 found none; that arm of the lists has no case here.  That the oracle's runs have the shape
claimed above is checked without a GPU."""
import numpy as np
import pytest

import oracle_lib as O
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

SWITCHES = ("TTX_CL_POWTAB", "TTX_CL_WORD", "TTX_CL_LISTS")
BASE = (9, 9, 8, 2)        # Ising C_m (d = m - 1 = 8 dimensions), n, maxrank, pivoting
LIMIT = (9, 3, 8, 2)
NG, SWEEPS = 2, 7
ALL_ON = {"powtab": True, "word": True, "lists": True}

_ORACLE, _OFF = {}, {}


def _oracle(case):
    """One oracle run per shape, shared and left unchanged."""
    if case not in _ORACLE:
        m, n, r, piv = case
        s = D.ising_setup("c", m, n)
        _ORACLE[case] = (s, O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=0.0, quad=s["quad"], tru=s["tru"], nproc=NG))
    return _ORACLE[case]


def _engine(monkeypatch, case, off=(), pipeline=True):
    monkeypatch.setenv("TTX_SWEEP", "cluster")
    for name in SWITCHES:
        if name in off:
            monkeypatch.setenv(name, "0")
        else:
            monkeypatch.delenv(name, raising=False)
    if pipeline:
        monkeypatch.delenv("TTX_PIPELINE", raising=False)
    else:
        monkeypatch.setenv("TTX_PIPELINE", "0")
    for name in ("TTX_CLUSTER_NB", "TTX_CL_PAD", "TTX_ARITH"):
        monkeypatch.delenv(name, raising=False)
    m, n, r, piv = case
    s, _ = _oracle(case)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=0.0, quad=s["quad"], tru=s["tru"], nproc=NG)
    assert tt.sweep_path() == "cluster" and tt.arith == "exact"
    form = tt.cluster_entry()
    assert {k: form[k] for k in ALL_ON} == {"powtab": "TTX_CL_POWTAB" not in off, "word": "TTX_CL_WORD" not in off, "lists": "TTX_CL_LISTS" not in off}
    return tt


def _snapshot(tt):
    recs = [(a["it"], a["neval"], a["erank"], a["val"], a["amax"], a["pivotmax"]) for a in tt.sweeps()]
    return {"tapes": tt.tapes().copy(), "recs": recs, "neval": tt.neval, "ranks": tt.ranks().copy(), "cores": [tt.core(k).copy() for k in range(1, tt.d + 1)]}


def _same(a, b, what):
    assert np.array_equal(a["tapes"], b["tapes"]), f"{what}: pivot tapes differ"
    assert a["recs"] == b["recs"], f"{what}: per-sweep records differ"
    assert a["neval"] == b["neval"] and np.array_equal(a["ranks"], b["ranks"]), what
    for k, (x, y) in enumerate(zip(a["cores"], b["cores"])):
        assert np.array_equal(x, y), f"{what}: core {k + 1} differs"


def _against_oracle(tt, case):
    s, oo = _oracle(case)
    gs, os_ = tt.sweeps(), oo["sweeps"]
    assert len(gs) == len(os_) == SWEEPS + 1
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d]), "pivot tapes differ from the oracle"
    for a, b in zip(gs, os_):
        assert a["neval"] == b["neval"] and a["erank"] == b["erank"], f"sweep {a['it']}"
        assert a["val"] == b["val"], f"sweep {a['it']}: val {a['val']!r} vs {b['val']!r}"
        assert a["amax"] == b["amax"] and a["pivotmax"] == b["pivotmax"], f"sweep {a['it']}"
    assert tt.neval == oo["neval"] and np.array_equal(tt.ranks(), oo["r"])
    for k in range(1, tt.d + 1):
        assert np.array_equal(tt.core(k), oo["cores"][k - 1]), f"core {k} differs from the oracle"
    assert tt.quad(s["quad"]) == oo["value"]


def _taken(tt, off):
    """launches of the last run that took the carried lists / word: all but the first, or none"""
    form = tt.cluster_entry()
    assert tt.cluster_fallbacks == 0
    assert form["lists_taken"] == (0 if "TTX_CL_LISTS" in off else SWEEPS - 1)
    assert form["word_taken"] == (0 if "TTX_CL_WORD" in off else SWEEPS - 1)


def _off_form(monkeypatch, case):
    """The entry as it was before anything was carried: one run per shape, shared."""
    if case not in _OFF:
        tt = _engine(monkeypatch, case, off=SWITCHES)
        tt.run()
        _taken(tt, SWITCHES)
        _against_oracle(tt, case)
        _OFF[case] = _snapshot(tt)
    return _OFF[case]


@pytest.mark.parametrize("case", [BASE, LIMIT], ids=["n9", "n3_rank_limit"])
def test_oracle_runs_have_the_shape_the_cases_rely_on(case):
    _, oo = _oracle(case)
    assert len(oo["sweeps"]) - 1 == SWEEPS >= 4
    t = oo["tapes"]          # [sweep - 1][bond][i, j, k, q]; bonds 1 .. d - 1
    assert len(oo["r"]) == 9, "d = 8: two groups of 3 and 4 own bonds"
    grown = [[int(t[k, p, 0]) > 0 for k in range(t.shape[0])] for p in range(1, case[0] - 1)]
    assert all(g[0] and g[1] for g in grown[1:-1]), "every inner bond accepts a pivot in sweeps 1 and 2: lists extended by a rebuilding and by a loading launch"
    if case is LIMIT:
        assert oo["r"][1] == 3 and oo["r"][case[0] - 2] == 3, "the outer bonds stop at the mode size"
        assert not any(grown[0][2:]) and not any(grown[-1][2:]), "... and accept nothing from sweep 3 on"
    for p in range(1, case[0] - 1):      # no run repeats a pivot row or column within a bond (module docstring)
        pv = [tuple(t[k, p]) for k in range(t.shape[0]) if t[k, p, 0] > 0]
        assert len({(a, b) for a, b, _, _ in pv}) == len(pv) == len({(c, d) for _, _, c, d in pv})


@pytest.mark.gpu
@pytest.mark.parametrize("case", [BASE, LIMIT], ids=["n9", "n3_rank_limit"])
def test_carried_state_bit_exact(monkeypatch, case):
    off = _off_form(monkeypatch, case)
    tt = _engine(monkeypatch, case)
    tt.run()
    _taken(tt, ())
    _against_oracle(tt, case)
    _same(_snapshot(tt), off, "against the switches-off form")


@pytest.mark.gpu
def test_two_runs_on_one_engine(monkeypatch):
    off = _off_form(monkeypatch, BASE)
    tt = _engine(monkeypatch, BASE)
    for run in (1, 2):
        tt.run()
        _taken(tt, ())           # SWEEPS - 1 in the second run too: its first launch rebuilt
        _against_oracle(tt, BASE)
        _same(_snapshot(tt), off, f"run {run} against the switches-off form")


@pytest.mark.gpu
def test_plain_loop_bit_exact(monkeypatch):
    off = _off_form(monkeypatch, BASE)
    tt = _engine(monkeypatch, BASE, pipeline=False)
    tt.run()
    _taken(tt, ())
    _against_oracle(tt, BASE)
    _same(_snapshot(tt), off, "TTX_PIPELINE=0 against the switches-off form")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SWITCHES)
def test_each_switch_off_alone(monkeypatch, name):
    off = _off_form(monkeypatch, BASE)
    tt = _engine(monkeypatch, BASE, off=(name,))
    tt.run()
    _taken(tt, (name,))
    _against_oracle(tt, BASE)
    _same(_snapshot(tt), off, f"{name}=0 against the switches-off form")
