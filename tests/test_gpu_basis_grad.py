"""Value and gradient of the resident train in a function basis on the device: ttx_basis_grad_batch / ttx_basis_grad_tab and their
_dev forms (ttcross_amd/csrc/ttx_basis_grad.h).

The checker is tests/basis_grad_ref.py: grad_chain restates the definition of include/ttx.h in numpy, and exact mode must equal it
bit for bit, val and grad.  val must equal basis_tab's bit for bit in both modes.  MFMA mode sums grad in another order; its bound
is the one derived in basis_grad_ref's docstring, |mfma - grad_chain| <= 2 N_g u B_m with N_g = sum_i (n_i max(r_(i-1), r_i) + 2) +
rmax + 1 and B_m the same chain on absolute values -- 2 N_g u relative for cores and tables without negative entries, where a dropped
tile or term shows.  Each shape's reference is computed once."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import basis_grad_ref as G
import basis_ref as B
import tt_ref as R
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {
    "mixed": ([7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]),
    "two_rows_mr5": ([4, 5, 3, 2], [1, 16, 33, 65, 1]),           # rank 65: two rows per lane in exact mode, MR = 5 in MFMA mode
    "bond128": ([2, 2, 2], [1, 128, 128, 1]),
    "mr6_mr8": ([3, 2, 3], [1, 96, 113, 1]),                      # MR = 6 and, below 128, MR = 8
    "ragged": ([3, 4, 2, 5], [1, 2, 70, 3, 1]),                   # rank 70 on one side only: the transposed step's row tails differ from the backward step's
    "d2": ([5, 7], [1, 3, 1]),
}
D1 = ([5], [1, 1])      # a train of one core: the engine holds none (ttx_from_tt), so this shape is checked where it can exist -- see the last test
NPTS = (1, 15, 17, 255, 257, 300)
PMAX = max(NPTS)
MODES = ("exact", "mfma")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _eq(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _case(name, nonneg):
    """cores, the engine, the tables of PMAX points, grad_chain and the bound at them: computed once, never changed"""
    n, r = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 1000 * nonneg)
    if nonneg:
        cores = [rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1])) / (0.5 * r[k + 1]) for k in range(len(n))]
        phis = [rng.uniform(0.0, 1.0, (PMAX, nk)) for nk in n]
        dphis = [rng.uniform(0.0, 1.0, (PMAX, nk)) for nk in n]
    else:
        cores = R.rand_train(sum(map(ord, name)), n, r)
        phis = [rng.standard_normal((PMAX, nk)) for nk in n]
        dphis = [rng.standard_normal((PMAX, nk)) for nk in n]
    tab, dtab = B.hstack(phis), B.hstack(dphis)
    val, grad = G.grad_chain(cores, phis, dphis)
    bnd = G.bound(cores, phis, dphis)
    for a in (tab, dtab, val, grad, bnd):
        a.setflags(write=False)
    return dict(n=n, r=r, cores=cores, phis=phis, dphis=dphis, tt=E.TTCross.from_cores(cores), tab=tab, dtab=dtab, val=val, grad=grad, bnd=bnd,
                N=G.count(cores))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_exact_tab_is_the_numpy_restatement_bit_for_bit(name, monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    monkeypatch.delenv("TTX_BASIS_GRAD_STORE", raising=False)
    for nonneg in (False, True):
        c = _case(name, nonneg)
        for p in NPTS:
            val, grad = c["tt"].basis_grad_tab(c["tab"][:p], c["dtab"][:p], "exact")
            assert _eq(val, c["val"][:p]) and _eq(grad, c["grad"][:p]), (nonneg, p)
    c = _case(name, False)
    monkeypatch.setenv("TTX_BASIS_CHUNK", "64")                                  # 300 points cross four chunk borders, the last chunk is short
    val, grad = c["tt"].basis_grad_tab(c["tab"], c["dtab"], "exact")
    assert _eq(val, c["val"]) and _eq(grad, c["grad"])
    last = c["tt"].basis_grad_last()
    assert last["mode"] == "exact" and last["chunk"] == 64


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_exact_tab_under_a_store_budget_that_forces_the_floor_of_256_points(name, monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    c = _case(name, False)
    S = sum(c["r"][:-1])
    monkeypatch.setenv("TTX_BASIS_GRAD_STORE", str(8 * S * 100))                # room for 100 points: below one tile, so 256 points per chunk and 300 make two
    val, grad = c["tt"].basis_grad_tab(c["tab"], c["dtab"], "exact")
    assert c["tt"].basis_grad_last()["chunk"] == 256
    assert _eq(val, c["val"]) and _eq(grad, c["grad"])
    monkeypatch.setenv("TTX_BASIS_GRAD_STORE", str(8 * S * 300))                # room for 300: the largest multiple of 256 below is 256 again
    c["tt"].basis_grad_tab(c["tab"], c["dtab"], "exact")
    assert c["tt"].basis_grad_last()["chunk"] == 256
    monkeypatch.delenv("TTX_BASIS_GRAD_STORE")
    c["tt"].basis_grad_tab(c["tab"], c["dtab"], "exact")
    assert c["tt"].basis_grad_last()["chunk"] == 300                            # the default budget does not bind here: one chunk of npts


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_val_is_basis_tab_bit_for_bit_in_both_modes_and_may_be_null(name, monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    monkeypatch.delenv("TTX_BASIS_GRAD_STORE", raising=False)
    L = E.load_library()
    for nonneg in (False, True):
        c = _case(name, nonneg)
        tt = c["tt"]
        for mode in MODES:
            for p in (17, 300):
                val, grad = tt.basis_grad_tab(c["tab"][:p], c["dtab"][:p], mode)
                assert _eq(val, tt.basis_tab(c["tab"][:p], mode)), (nonneg, mode, p)
            g2 = np.zeros_like(grad)
            tab, dtab = np.ascontiguousarray(c["tab"]), np.ascontiguousarray(c["dtab"])
            assert L.ttx_basis_grad_tab(tt._h, PMAX, E._dp(tab), E._dp(dtab), None, E._dp(g2), E.EVAL_MODES[mode]) == 0
            assert _eq(g2, grad), (nonneg, mode)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mfma_grad_is_within_the_derived_bound(name, monkeypatch):
    monkeypatch.delenv("TTX_BASIS_GRAD_STORE", raising=False)
    for nonneg in (False, True):
        c = _case(name, nonneg)
        monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
        for p in NPTS + (-64,):
            if p < 0:
                monkeypatch.setenv("TTX_BASIS_CHUNK", str(-p))
                p = PMAX
            _, grad = c["tt"].basis_grad_tab(c["tab"][:p], c["dtab"][:p], "mfma")
            err = np.abs(grad - c["grad"][:p])
            with np.errstate(invalid="ignore", divide="ignore"):
                print(name, "nonneg" if nonneg else "signed", p, "max err / bound", float(np.nanmax(np.where(c["bnd"][:p] > 0, err / c["bnd"][:p], 0.0))))
            assert np.all(err <= c["bnd"][:p]), (nonneg, p)
            if nonneg:
                assert np.all(c["grad"][:p] > 0.0) and np.all(err <= 2 * c["N"] * B.U * c["grad"][:p]), p
    assert c["tt"].basis_grad_last()["mode"] == "mfma"


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mfma_results_of_a_point_do_not_depend_on_the_batch_the_chunk_or_the_call(name, monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    monkeypatch.delenv("TTX_BASIS_GRAD_STORE", raising=False)
    c = _case(name, False)
    tt = c["tt"]
    v300, g300 = tt.basis_grad_tab(c["tab"], c["dtab"], "mfma")
    v17, g17 = tt.basis_grad_tab(c["tab"][:17], c["dtab"][:17], "mfma")
    assert _eq(v300[:17], v17) and _eq(g300[:17], g17)
    again = tt.basis_grad_tab(c["tab"], c["dtab"], "mfma")
    assert _eq(again[0], v300) and _eq(again[1], g300)
    monkeypatch.setenv("TTX_BASIS_CHUNK", "64")
    v64, g64 = tt.basis_grad_tab(c["tab"], c["dtab"], "mfma")
    assert tt.basis_grad_last()["chunk"] == 64
    assert _eq(v64, v300) and _eq(g64, g300)
    monkeypatch.delenv("TTX_BASIS_CHUNK")
    monkeypatch.setenv("TTX_BASIS_GRAD_STORE", "1")
    v256, g256 = tt.basis_grad_tab(c["tab"], c["dtab"], "mfma")
    assert tt.basis_grad_last()["chunk"] == 256
    assert _eq(v256, v300) and _eq(g256, g300)


def _bases(n, rng):
    """per mode a COS or a LINEAR entry, alternating, and points that lie inside, on the ends, on the nodes and (LINEAR) outside"""
    basis, cols = [], []
    for k, nk in enumerate(n):
        if k % 2 == 0:
            a, b = -1.0 - k, 2.5 + k
            basis.append(("cos", a, b, True) if k % 4 == 0 else ("cos", a, b))
            x = rng.uniform(a, b, PMAX)
            x[:2] = a, b
        else:
            t = np.sort(rng.uniform(-2.0, 3.0, nk))
            basis.append(("linear", t))
            x = rng.uniform(t[0] - 0.5, t[-1] + 0.5, PMAX)
            x[:nk] = t[:PMAX]
        cols.append(x)
    return basis, np.ascontiguousarray(np.stack(cols, axis=1))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_basis_grad_batch_is_basis_grad_tab_of_the_host_tables_bit_for_bit(name, monkeypatch):
    monkeypatch.delenv("TTX_BASIS_GRAD_STORE", raising=False)
    c = _case(name, False)
    tt, n = c["tt"], c["n"]
    basis, x = _bases(n, np.random.default_rng(37))
    tab = B.hstack([E.basis_table(e, nk, x[:, k]) for k, (e, nk) in enumerate(zip(basis, n))])
    dtab = B.hstack([E.basis_dtable(e, nk, x[:, k]) for k, (e, nk) in enumerate(zip(basis, n))])
    assert np.isfinite(tab).all() and np.isfinite(dtab).all() and np.any(dtab != 0.0)
    for mode in MODES:
        monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
        wv, wg = tt.basis_grad_tab(tab, dtab, mode)
        for p in (1, 17, 300):
            val, grad = tt.basis_grad_batch(x[:p], basis, mode)
            assert _eq(val, wv[:p]) and _eq(grad, wg[:p]), (mode, p)
        assert _eq(val, tt.basis_batch(x, basis, mode)), mode
        monkeypatch.setenv("TTX_BASIS_CHUNK", "64")
        val, grad = tt.basis_grad_batch(x, basis, mode)
        assert _eq(val, wv) and _eq(grad, wg), mode
        assert tt.basis_grad_last()["ms_table"] > 0.0


def test_gradient_agrees_with_basis_tab_of_the_substituted_tables_for_every_mode(monkeypatch):
    """the substitution route on the device: grad[:, m] against basis_tab with mode m's table replaced by dphi"""
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    monkeypatch.delenv("TTX_BASIS_GRAD_STORE", raising=False)
    for nonneg in (False, True):
        c = _case("mixed", nonneg)
        tt = c["tt"]
        for mode in MODES:
            _, grad = tt.basis_grad_tab(c["tab"], c["dtab"], mode)
            for m in range(len(c["n"])):
                sub = tt.basis_tab(B.hstack(G.substituted(c["phis"], c["dphis"], m)), mode)
                assert np.all(np.abs(grad[:, m] - sub) <= c["bnd"][:, m]), (nonneg, mode, m)
                if nonneg:
                    assert np.all(sub > 0.0)


def test_a_nan_coordinate_stays_with_its_point():
    c = _case("mixed", False)
    tt = c["tt"]
    rng = np.random.default_rng(45)
    basis = [("cos", 0.0, 1.0), ("linear", [0.0, 1.0]), ("cos", 0.0, 1.0, True), ("cos", 0.0, 1.0), ("linear", np.linspace(0.0, 1.0, 9))]
    x = rng.uniform(0.0, 1.0, (300, 5))
    bad = x.copy()
    bad[7, 1] = np.nan                                                          # LINEAR: a NaN row
    bad[100, 2] = np.nan                                                        # COS: NaN
    bad[130, 0] = 2.0 ** 18                                                     # COS, n = 7: j pi 2^18 > 2^19 from j = 1 on
    bad[299, 4] = np.nan
    hit = np.zeros(300, bool)
    hit[[7, 100, 130, 299]] = True
    for mode in MODES:
        (cv, cg), (gv, gg) = tt.basis_grad_batch(x, basis, mode), tt.basis_grad_batch(bad, basis, mode)
        assert np.isfinite(cv).all() and np.isfinite(cg).all()
        assert np.isnan(gv[hit]).all() and np.isnan(gg[hit]).all(), mode
        assert _eq(gv[~hit], cv[~hit]) and _eq(gg[~hit], cg[~hit]), mode


def test_device_pointer_entries_equal_the_host_entries():
    """torch tensors by data_ptr() through the _dev entries, in a child process (basis_grad_dev_worker.py says why)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "basis_grad_dev_worker.py")], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert res[mode] == dict(batch_is_cuda=True, batch_equal=True, tab_is_cuda=True, tab_equal=True, chunked_equal=True, empty=[[0], [0, 4]]), (mode, res[mode])
    assert res["float32_refused"] and res["shape_refused"] and res["host_dphi_refused"]


def test_conditions_refusals_and_figures(monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    monkeypatch.delenv("TTX_BASIS_GRAD_STORE", raising=False)
    L = E.load_library()
    c = _case("mixed", False)
    tt, n, r = c["tt"], c["n"], c["r"]
    EINVAL, ESTATE, nul = 1, 4, ctypes.POINTER(ctypes.c_double)()
    val, grad, x = np.zeros(4), np.zeros((4, 5)), np.full((4, 5), 0.5)
    arr = (E._Basis * 5)(*[E._Basis(E.TTX_BASIS_COS, 0, 0.0, 1.0, None) for _ in range(5)])
    t4, d4 = np.ascontiguousarray(c["tab"][:4]), np.ascontiguousarray(c["dtab"][:4])

    def refused(rc, entry):
        return rc == EINVAL and entry in L.ttx_last_error().decode()

    # npts = 0 succeeds and launches nothing
    assert L.ttx_basis_grad_tab(tt._h, 0, nul, nul, nul, nul, 0) == 0 and L.ttx_basis_grad_batch(tt._h, 0, nul, None, nul, nul, 1) == 0
    assert L.ttx_basis_grad_tab_dev(tt._h, 0, None, None, None, None, 2) == 0 and L.ttx_basis_grad_batch_dev(tt._h, 0, None, None, None, None, 0) == 0
    v0, g0 = tt.basis_grad_tab(np.zeros((0, sum(n))), np.zeros((0, sum(n))), "mfma")
    assert v0.shape == (0,) and g0.shape == (0, 5) and tt.basis_grad_last()["flops"] == 0.0
    # a null grad, null tables, an unknown mode, negative npts
    assert refused(L.ttx_basis_grad_tab(tt._h, 4, E._dp(t4), E._dp(d4), E._dp(val), nul, 0), "ttx_basis_grad_tab:")
    assert refused(L.ttx_basis_grad_tab(tt._h, 4, E._dp(t4), nul, E._dp(val), E._dp(grad), 0), "ttx_basis_grad_tab:")
    assert refused(L.ttx_basis_grad_tab(tt._h, 4, nul, E._dp(d4), E._dp(val), E._dp(grad), 0), "ttx_basis_grad_tab:")
    assert refused(L.ttx_basis_grad_tab(tt._h, 4, E._dp(t4), E._dp(d4), E._dp(val), E._dp(grad), 3), "ttx_basis_grad_tab:")
    assert refused(L.ttx_basis_grad_tab(tt._h, -1, E._dp(t4), E._dp(d4), E._dp(val), E._dp(grad), 0), "ttx_basis_grad_tab:")
    assert refused(L.ttx_basis_grad_tab_dev(tt._h, 4, None, None, None, None, 0), "ttx_basis_grad_tab_dev:")
    assert refused(L.ttx_basis_grad_batch(tt._h, 4, E._dp(x), arr, E._dp(val), nul, 0), "ttx_basis_grad_batch:")
    assert refused(L.ttx_basis_grad_batch(tt._h, 4, E._dp(x), None, E._dp(val), E._dp(grad), 0), "ttx_basis_grad_batch:")
    assert refused(L.ttx_basis_grad_batch(tt._h, 4, E._dp(x), arr, E._dp(val), E._dp(grad), 7), "ttx_basis_grad_batch:")
    assert refused(L.ttx_basis_grad_batch_dev(tt._h, 4, None, arr, None, None, 0), "ttx_basis_grad_batch_dev:")
    # an unknown kind, before any launch
    arr2 = (E._Basis * 5)(*([arr[0]] * 3 + [E._Basis(9, 0, 0.0, 1.0, None)] + [arr[0]]))
    assert refused(L.ttx_basis_grad_batch(tt._h, 4, E._dp(x), arr2, E._dp(val), E._dp(grad), 0), "ttx_basis_grad_batch: mode 4")
    assert "unknown basis kind 9" in L.ttx_last_error().decode()
    with pytest.raises(ValueError):
        tt.basis_grad_batch(x, [("cos", 0.0, 1.0)] * 4)
    with pytest.raises(ValueError):
        tt.basis_grad_tab(c["tab"], c["dtab"][:, :-1])
    # an engine without a train (five modes, as the tables here): TTX_ESTATE
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    assert L.ttx_basis_grad_tab(fresh._h, 4, E._dp(t4), E._dp(d4), E._dp(val), E._dp(grad), 0) == ESTATE
    assert L.ttx_basis_grad_batch(fresh._h, 4, E._dp(x), arr, E._dp(val), E._dp(grad), 0) == ESTATE
    # the figures of the last call; auto is one of the two modes
    w = sum(r[k] * n[k] * r[k + 1] for k in range(5))
    res = {m: tt.basis_grad_tab(c["tab"], c["dtab"], m) for m in MODES}
    for m in MODES:
        tt.basis_grad_tab(c["tab"][:257], c["dtab"][:257], m)
        last = tt.basis_grad_last()
        assert last["mode"] == m and last["flops"] == 6.0 * 257 * w and last["chunk"] == 257
        assert last["ms_back"] > 0.0 and last["ms_fwd"] > 0.0 and last["ms_table"] == 0.0
    av, ag = tt.basis_grad_tab(c["tab"], c["dtab"], "auto")
    ran = tt.basis_grad_last()["mode"]
    assert ran in MODES and _eq(av, res[ran][0]) and _eq(ag, res[ran][1])
    assert _eq(tt.basis_tab(c["tab"], "exact"), c["val"])                       # the train and basis_tab's results are untouched
    for k, core in enumerate(c["cores"]):
        assert np.array_equal(tt.core(k + 1), core)


def test_a_train_of_one_core_cannot_be_resident_and_its_gradient_is_checked_on_the_host():
    """d = 1 of the definition: the engine refuses to hold a train of one core (include/ttx.h: "at least two cores"), whatever the
    operation, so no device call can see this shape.  What exists of it is checked: the numpy restatement gives val = sum_j phi_j
    U(1, j, 1) and grad_1 = sum_j dphi_j U(1, j, 1) (summed from 0.0 over ascending j), and the same core padded with a second mode
    of one index and the table (1), which multiplies by 1.0 and adds 0.0 only, gives the same numbers on the device in exact mode."""
    n, r = D1
    rng = np.random.default_rng(77)
    core = rng.standard_normal((r[0], n[0], r[1]))
    with pytest.raises(E.TTXError, match="at least two cores"):
        E.TTCross.from_cores([core])
    phi, dphi = rng.standard_normal((PMAX, n[0])), rng.standard_normal((PMAX, n[0]))
    val, grad = G.grad_chain([core], [phi], [dphi])
    v = g = np.zeros(PMAX)
    for j in range(n[0]):
        v, g = v + phi[:, j] * core[0, j, 0], g + dphi[:, j] * core[0, j, 0]
    assert _eq(val, v) and _eq(grad[:, 0], g)
    tt = E.TTCross.from_cores([core, np.ones((1, 1, 1))])
    one, zero = np.ones((PMAX, 1)), np.zeros((PMAX, 1))
    for p in NPTS:
        dv, dg = tt.basis_grad_tab(B.hstack([phi, one])[:p], B.hstack([dphi, zero])[:p], "exact")
        assert np.array_equal(dv, val[:p]) and np.array_equal(dg[:, 0], grad[:p, 0]) and not dg[:, 1].any()      # == : the sign of a zero is not compared
        mv, mg = tt.basis_grad_tab(B.hstack([phi, one])[:p], B.hstack([dphi, zero])[:p], "mfma")
        bnd = G.bound([core], [phi], [dphi])[:p, 0]
        assert np.all(np.abs(mg[:, 0] - grad[:p, 0]) <= bnd) and not mg[:, 1].any()
