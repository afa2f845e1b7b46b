"""What the four samplers share on the device and on the host (sm_wave_search of ttcross_amd/csrc/ttx_sample.h, sq_frame and the
last-call records of ttx_engine.hip, the one call path of ttcross_amd/engine.py): they must not disturb each other on one engine,
and the search, shared by the cell samplers and written out in the index samplers, must keep the edge rules of all four at the
ends of the lanes.

The train: d = 4, modes of 66, 1, 31 and 2 nodes, ranks 1, 3, 4, 2, 1, standard normal cores (signed).  One mode has more than 64
entries and more than 64 cells (two rounds of the search), one has a single node (the real samplers hold it), 31 nodes fill two
index tiles of 16 and three cell tiles of 15 whose last one holds a single cell, and one mode has a single cell.  65 samples: one
more than a 64-sample block of the rows kernels and than sixteen workgroups of four waves.

The checkers are the verify functions of tests/sample_ref.py, sample_real_ref.py, sample_sq_ref.py and sample_sq_real_ref.py at
their own derived allowances; every sample goes through them."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sample_real_ref as SR
import sample_ref as S
import sample_sq_real_ref as QR
import sample_sq_ref as SQ
from ttcross_amd import engine as E

N_MODES, RANKS, NPTS, LONG = [66, 1, 31, 2], [1, 3, 4, 2, 1], 65, 0
IND, REAL = ("ind", "logq", "val"), ("x", "cell", "logq", "val")


@functools.lru_cache(maxsize=None)
def _train():
    rng = np.random.default_rng(66131)
    cores = [rng.standard_normal((RANKS[k], N_MODES[k], RANKS[k + 1])) for k in range(len(N_MODES))]
    nodes = [np.cumsum(rng.uniform(0.2, 1.0, nk)) - rng.uniform(0.0, 3.0) for nk in N_MODES]
    u = rng.random((NPTS, len(N_MODES)))
    u.setflags(write=False)
    return cores, nodes, u


def _calls(u_real=None):
    """name -> (the call on an engine, its output names, its *_last), in the order of the first round"""
    cores, nodes, u = _train()
    ur = u if u_real is None else u_real
    return {"sample": (lambda tt: tt.sample(u), IND, lambda tt: tt.sample_last()),
            "sample_sq": (lambda tt: tt.sample_sq(u, mode="exact"), IND, lambda tt: tt.sample_sq_last()),
            "sample_real": (lambda tt: tt.sample_real(ur, nodes), REAL, lambda tt: tt.sample_real_last()),
            "sample_sq_real": (lambda tt: tt.sample_sq_real(u, nodes, mode="mfma"), REAL, lambda tt: tt.sample_sq_real_last())}


def _same(a, b, names, rows=slice(None)):
    return all(np.ascontiguousarray(a[k][rows]).tobytes() == np.ascontiguousarray(b[k][rows]).tobytes() for k in names)


def test_the_samplers_do_not_disturb_each_other():
    cores, nodes, u = _train()
    tt = E.TTCross.from_cores(cores)
    bad_row = 7
    un = u.copy()
    un[bad_row, 2] = np.nan                                             # mode 3 (31 nodes) is drawn
    keep = np.arange(NPTS) != bad_row
    first = {name: c[0](tt) for name, c in _calls().items()}
    second = {name: c[0](tt) for name, c in reversed(list(_calls(un).items()))}
    last = {name: c[2](tt) for name, c in _calls().items()}
    for name, (call, names, _) in _calls().items():
        rows = keep if name == "sample_real" else slice(None)
        assert _same(first[name], second[name], names, rows), name
        fresh = call(E.TTCross.from_cores(cores))
        assert _same(first[name], fresh, names), name
        assert _same(second[name], fresh, names, rows), name
    sr = second["sample_real"]
    assert np.all(np.isnan(sr["x"][bad_row])) and np.all(sr["cell"][bad_row] == 0) and np.isnan(sr["logq"][bad_row]) and sr["val"][bad_row] == 0.0
    assert last["sample_real"]["failed"] == 1
    assert last["sample"]["failed"] == 0 and last["sample_sq"]["failed"] == 0 and last["sample_sq_real"]["failed"] == 0
    assert last["sample_sq"]["mode"] == "exact" and last["sample_sq_real"]["mode"] == "mfma"


@functools.lru_cache(maxsize=None)
def _edge_u():
    """the long mode's column is 0, the largest double below 1, 1 and 1.5 in the first four rows"""
    u = _train()[2].copy()
    u[:4, LONG] = [0.0, 1.0 - 2.0 ** -53, 1.0, 1.5]
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=None)
def _edge_engine():
    return E.TTCross.from_cores(_train()[0])


def test_index_search_at_the_lane_edges():
    cores, _, _ = _train()
    u, tt, n = _edge_u(), _edge_engine(), N_MODES[LONG]
    res = tt.sample(u)
    chk = S.verify(cores, u, None, None, res["ind"])
    assert tt.sample_last()["failed"] == 0 and chk["undecided"] <= NPTS // 1000
    assert np.all(S.draw(cores, u)[0][2:4, LONG] == n)                 # the last entry has positive mass: u >= 1 lands there
    assert np.all(res["ind"][2:4, LONG] == n)
    assert np.array_equal(res["val"], tt.tijk_batch(res["ind"], "exact"))
    for mode in ("exact", "mfma"):
        res = tt.sample_sq(u, mode=mode)
        chk = SQ.verify(cores, u, None, None, 0.0, res["ind"])
        assert tt.sample_sq_last()["failed"] == 0 and chk["undecided"] <= NPTS // 1000, mode
        assert np.all(SQ.draw(cores, u)[0][2:4, LONG] == n)
        assert np.all(res["ind"][2:4, LONG] == n), mode
        assert np.array_equal(res["val"], tt.tijk_batch(res["ind"], "exact")), mode


def test_cell_search_at_the_lane_edges():
    cores, nodes, _ = _train()
    u, tt, t = _edge_u(), _edge_engine(), nodes[LONG]
    res = tt.sample_real(u, nodes)
    chk = SR.verify(cores, nodes, u, None, res["x"], res["cell"])
    print("sample_real worst |CDF - T| / tol", chk["worst"])
    assert tt.sample_real_last()["failed"] == 0
    assert np.all(SR.draw(cores, nodes, u)[1][2:4, LONG] == t.size - 1)     # the last cell has positive mass: u >= 1 ends at its right node
    assert np.all(res["cell"][2:4, LONG] == t.size - 1) and np.all(res["x"][2:4, LONG] == t[-1])
    assert res["x"][0, LONG] == t[res["cell"][0, LONG] - 1]            # u = 0: the left node of the first cell with mass
    for mode in ("exact", "mfma"):
        res = tt.sample_sq_real(u, nodes, mode=mode)
        chk = QR.verify(cores, nodes, u, None, 0.0, res["x"], res["cell"])
        print("sample_sq_real", mode, "worst |CDF - T| / tol", chk["worst"])
        assert tt.sample_sq_real_last()["failed"] == 0, mode
        assert np.all(QR.draw(cores, nodes, u)[1][2:4, LONG] == t.size - 1)
        assert np.all(res["cell"][2:4, LONG] == t.size - 1) and np.all(res["x"][2:4, LONG] == t[-1]), mode
        assert res["x"][0, LONG] == t[res["cell"][0, LONG] - 1], mode
