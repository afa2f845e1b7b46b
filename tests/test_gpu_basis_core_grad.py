"""Gradient with respect to the cores of the resident train in a function basis on the device: ttx_basis_core_grad_batch /
ttx_basis_core_grad_tab, their _dev forms and ttx_cores_axpy (ttcross_amd/csrc/ttx_basis_core_grad.h).

The checker is tests/basis_core_grad_ref.py: core_grad_chain restates the definition of include/ttx.h in numpy, and exact mode must
equal it bit for bit, val and every G_i.  val must equal basis_tab's bit for bit in both modes.  MFMA mode sums G in another order;
its bound is the one derived in basis_core_grad_ref's docstring, |mfma - core_grad_chain| <= 2 N_i u B_i with N_i = sum_(m < i)
(n_m r_(m-1) + 2) + sum_(m > i) (n_m r_m + 2) + P + 4 and B_i the same sums on absolute values -- 2 N_i u relative for cores, tables
and weights without negative entries, where a dropped tile, point group or partial block shows.  Each shape's references are
computed once."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import basis_core_grad_ref as C
import basis_ref as B
import tt_ref as R
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {                                                          # the shapes of test_gpu_basis_grad.py
    "mixed": ([7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]),
    "two_rows_mr5": ([4, 5, 3, 2], [1, 16, 33, 65, 1]),
    "bond128": ([2, 2, 2], [1, 128, 128, 1]),
    "mr6_mr8": ([3, 2, 3], [1, 96, 113, 1]),
    "ragged": ([3, 4, 2, 5], [1, 2, 70, 3, 1]),
    "d2": ([5, 7], [1, 3, 1]),
}
NPTS = (1, 3, 4, 5, 15, 17, 63, 65, 255, 257, 300)                  # the four-point grouping of the contraction, the tile edges, two segments
PMAX = max(NPTS)
MODES = ("exact", "mfma")
CHUNK_VARS = ("TTX_BASIS_CHUNK", "TTX_BASIS_GRAD_STORE")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _eqs(ga, gb):
    return len(ga) == len(gb) and all(_eq(a, b) for a, b in zip(ga, gb))


def _within(g, ref, bnd):
    return all(np.all(np.abs(a - b) <= t) for a, b, t in zip(g, ref, bnd))


def _clear(monkeypatch):
    for v in CHUNK_VARS:
        monkeypatch.delenv(v, raising=False)


@functools.lru_cache(maxsize=None)
def _case(name, nonneg):
    """cores, the engine, the tables and weights of PMAX points: computed once, never changed"""
    n, r = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 1000 * nonneg + 7)
    if nonneg:
        cores = [rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1])) / (0.5 * r[k + 1]) for k in range(len(n))]
        phis = [rng.uniform(0.0, 1.0, (PMAX, nk)) for nk in n]
        c = rng.uniform(0.0, 1.0, PMAX)
    else:
        cores = R.rand_train(sum(map(ord, name)), n, r)
        phis = [rng.standard_normal((PMAX, nk)) for nk in n]
        c = rng.standard_normal(PMAX)
    tab = B.hstack(phis)
    for a in (tab, c):
        a.setflags(write=False)
    return dict(n=n, r=r, d=len(n), cores=cores, phis=phis, c=c, tab=tab, tt=E.TTCross.from_cores(cores))


@functools.lru_cache(maxsize=None)
def _ref(name, nonneg, p):
    """(val, G, bound) of the restatement at the first p points"""
    cs = _case(name, nonneg)
    phis, c = [ph[:p] for ph in cs["phis"]], cs["c"][:p]
    val, G = C.core_grad_chain(cs["cores"], phis, c)
    return val, G, C.bound(cs["cores"], phis, c)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_exact_is_the_numpy_restatement_and_val_is_basis_tabs_bit_for_bit(name, monkeypatch):
    _clear(monkeypatch)
    for nonneg in (False, True):
        cs = _case(name, nonneg)
        tt = cs["tt"]
        for p in NPTS:
            rv, rG, _ = _ref(name, nonneg, p)
            val, G = tt.basis_core_grad_tab(cs["tab"][:p], cs["c"][:p], "exact")
            assert _eq(val, rv) and _eqs(G, rG), (nonneg, p)
            assert [g.shape for g in G] == [u.shape for u in cs["cores"]]
        for mode in MODES:
            for p in (17, 300):
                val, _ = tt.basis_core_grad_tab(cs["tab"][:p], cs["c"][:p], mode)
                assert _eq(val, tt.basis_tab(cs["tab"][:p], mode)), (nonneg, mode, p)
    assert tt.basis_core_grad_last()["mode"] == "mfma"


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mfma_is_within_the_derived_bound(name, monkeypatch):
    _clear(monkeypatch)
    for nonneg in (False, True):
        cs = _case(name, nonneg)
        for p in NPTS:
            _, rG, bnd = _ref(name, nonneg, p)
            _, G = cs["tt"].basis_core_grad_tab(cs["tab"][:p], cs["c"][:p], "mfma")
            for i in range(cs["d"]):
                err = np.abs(G[i] - rG[i])
                with np.errstate(invalid="ignore", divide="ignore"):
                    print(name, "nonneg" if nonneg else "signed", p, "core", i + 1, "max err / bound", float(np.nanmax(np.where(bnd[i] > 0, err / bnd[i], 0.0))))
                assert np.all(err <= bnd[i]), (nonneg, p, i)
                if nonneg:                                                      # relative: a dropped tile, point group or partial block shows
                    assert np.all(rG[i] > 0.0) and np.all(err <= 2 * C.count(cs["cores"], i, p) * B.U * rG[i]), (p, i)
    last = cs["tt"].basis_core_grad_last()
    assert last["mode"] == "mfma" and last["chunk"] == PMAX and last["ms_acc"] > 0.0 and last["ms_back"] > 0.0 and last["ms_fwd"] > 0.0


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_chunks_accumulation_and_masked_points(name, monkeypatch):
    cs = _case(name, False)
    tt, tab, c = cs["tt"], cs["tab"], cs["c"]
    for var, value in (("TTX_BASIS_CHUNK", "256"), ("TTX_BASIS_GRAD_STORE", "1")):     # a chunk of 256 asked for; a store below one tile, which forces 256
        _clear(monkeypatch)
        monkeypatch.setenv(var, value)
        for p in (257, 300):
            rv, rG, bnd = _ref(name, False, p)
            val, G = tt.basis_core_grad_tab(tab[:p], c[:p], "exact")
            assert tt.basis_core_grad_last()["chunk"] == 256
            assert _eq(val, rv) and _eqs(G, rG), (var, p)                       # each chunk continues from the buffer: the unchunked bits
            val, G = tt.basis_core_grad_tab(tab[:p], c[:p], "mfma")
            assert tt.basis_core_grad_last()["chunk"] == 256
            assert _eq(val, tt.basis_tab(tab[:p], "mfma")) and _within(G, rG, bnd), (var, p)
    _clear(monkeypatch)
    rv, rG, bnd = _ref(name, False, PMAX)
    for h in (150, 257):                                                        # two calls on the two parts, the second accumulates
        for mode in MODES:
            _, G1 = tt.basis_core_grad_tab(tab[:h], c[:h], mode)
            v2, G2 = tt.basis_core_grad_tab(tab[h:], c[h:], mode, out=G1, accumulate=True)
            assert _eq(v2, tt.basis_tab(tab[h:], mode))
            assert _eqs(G2, rG) if mode == "exact" else _within(G2, rG, bnd), (h, mode)
    # appended points with c = 0 and finite tables: every term is a zero, exact mode's bits stay
    rng = np.random.default_rng(3)
    tab0 = np.vstack([tab, rng.standard_normal((5, tab.shape[1]))])
    _, G0 = tt.basis_core_grad_tab(tab0, np.concatenate([c, np.zeros(5)]), "exact")
    assert _eqs(G0, rG)
    _, G0 = tt.basis_core_grad_tab(tab0, np.concatenate([c, np.zeros(5)]), "mfma")
    assert _within(G0, rG, bnd)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mfma_repeats_bit_for_bit(name, monkeypatch):
    _clear(monkeypatch)
    cs = _case(name, False)
    a = cs["tt"].basis_core_grad_tab(cs["tab"], cs["c"], "mfma")
    b = cs["tt"].basis_core_grad_tab(cs["tab"], cs["c"], "mfma")
    assert _eq(a[0], b[0]) and _eqs(a[1], b[1])
    monkeypatch.setenv("TTX_BASIS_CHUNK", "256")                                # and so does a chunked call
    a = cs["tt"].basis_core_grad_tab(cs["tab"], cs["c"], "mfma")
    b = cs["tt"].basis_core_grad_tab(cs["tab"], cs["c"], "mfma")
    assert _eq(a[0], b[0]) and _eqs(a[1], b[1])


def _bases(n, rng):
    """per mode a COS or a LINEAR entry, alternating, and points inside, on the ends and (LINEAR) outside"""
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
        cols.append(x)
    return basis, np.ascontiguousarray(np.stack(cols, axis=1))


@pytest.mark.parametrize("name", ["mixed", "two_rows_mr5"])
def test_coordinates_give_what_the_host_tables_give_bit_for_bit(name, monkeypatch):
    cs = _case(name, False)
    tt, n, c = cs["tt"], cs["n"], cs["c"]
    basis, x = _bases(n, np.random.default_rng(41))
    tab = B.hstack([E.basis_table(e, nk, x[:, k]) for k, (e, nk) in enumerate(zip(basis, n))])
    for mode in MODES:
        _clear(monkeypatch)
        wv, wG = tt.basis_core_grad_tab(tab, c, mode)
        val, G = tt.basis_core_grad(x, basis, c, mode)
        assert _eq(val, wv) and _eqs(G, wG), mode
        assert tt.basis_core_grad_last()["ms_table"] > 0.0
        monkeypatch.setenv("TTX_BASIS_CHUNK", "256")
        cv, cG = tt.basis_core_grad_tab(tab, c, mode)
        val, G = tt.basis_core_grad(x, basis, c, mode)
        assert _eq(val, cv) and _eqs(G, cG), mode


def test_device_pointer_entries_equal_the_host_entries():
    """torch tensors by data_ptr() through the _dev entries, in a child process (basis_core_grad_dev_worker.py says why)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "basis_core_grad_dev_worker.py")], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert res[mode] == dict(batch_is_cuda=True, batch_equal=True, tab_is_cuda=True, tab_equal=True, chunked_equal=True, accumulated_equal=True,
                                 empty_zeroes=True, empty_keeps=True), (mode, res[mode])
    assert res["axpy_equal"] and res["float32_refused"] and res["host_c_refused"] and res["short_out_refused"]


@pytest.mark.parametrize("name", ["mixed", "ragged"])
def test_linearity_identity_against_basis_tab_of_the_replaced_train(name, monkeypatch):
    """sum_p c_p f_(U_i <- E)(x_p) = <G_i, E>: the left side by existing code (from_cores of the train with core i replaced, basis_tab),
    within the sum of both allowances (basis_core_grad_ref.identity_allowance)"""
    _clear(monkeypatch)
    rng = np.random.default_rng(61)
    for nonneg in (False, True):
        cs = _case(name, nonneg)
        Bi = C.abs_core_grad(cs["cores"], cs["phis"], cs["c"])
        for mode in MODES:
            _, G = cs["tt"].basis_core_grad_tab(cs["tab"], cs["c"], mode)
            for i in range(cs["d"]):
                E_ = rng.uniform(0.0, 1.0, cs["cores"][i].shape) if nonneg else rng.standard_normal(cs["cores"][i].shape)
                on_device = lambda cores, phis: E.TTCross.from_cores(cores).basis_tab(B.hstack(phis), mode)     # noqa: E731
                left, right = C.identity_sides(cs["cores"], cs["phis"], cs["c"], i, E_, G[i], chain=on_device)
                allow = C.identity_allowance(cs["cores"], cs["phis"], cs["c"], i, E_, Bi[i])
                assert abs(left - right) <= allow, (nonneg, mode, i, abs(left - right) / allow)
                if nonneg:
                    assert left > 0.0 and allow < 1e-9 * left                   # relative: a missing point would be 1 / 300 of the sum


def test_cores_axpy_updates_every_core_and_nothing_stale_survives(monkeypatch):
    _clear(monkeypatch)
    cs = _case("mixed", False)
    cores, tab, n = cs["cores"], cs["tab"], cs["n"]
    tt = E.TTCross.from_cores(cores)                                            # an engine of its own: this test changes the cores
    _, G = tt.basis_core_grad_tab(tab, cs["c"], "exact")
    w = [np.cos(np.arange(nk) + 1.0) for nk in n]
    before = (tt.basis_tab(tab, "exact"), tt.norm(), tt.quad(w))               # whatever these calls leave behind is now on the engine
    alpha = np.array([0.5, -1.25, 0.0, 3.0, 1e-3])
    G[2][0, 1, 2] = np.nan                                                      # core 3 has alpha = 0: its NaN must not be read
    tt.cores_axpy(alpha, G)
    want = [u + a * g for u, a, g in zip(cores, alpha, G)]
    want[2] = cores[2]
    for k in range(5):
        assert _eq(tt.core(k + 1), want[k]), k
    fresh = E.TTCross.from_cores(want)
    after = (tt.basis_tab(tab, "exact"), tt.norm(), tt.quad(w))
    assert _eq(after[0], fresh.basis_tab(tab, "exact")) and _eq(after[0], B.chain(want, cs["phis"]))
    assert _bits(after[1]) == _bits(fresh.norm()) and _bits(after[2]) == _bits(fresh.quad(w))
    assert not _eq(after[0], before[0]) and after[1] != before[1] and after[2] != before[2]
    for k in range(5):                                                          # norm and quad did not change the cores either
        assert _eq(tt.core(k + 1), want[k]), k
    # a scalar alpha, a flat array, and the gradient of the updated train
    flat = np.concatenate([g.ravel(order="F") for g in want])
    assert np.array_equal(tt.core_offsets(), np.concatenate([[0], np.cumsum([u.size for u in cores])]))
    tt.cores_axpy(-1.0, flat)
    for k in range(5):
        assert _eq(tt.core(k + 1), want[k] + (-1.0) * want[k]), k


def test_block_coordinate_least_squares_fit_follows_the_numpy_loop_bit_for_bit(monkeypatch):
    """n = [5, 6, 4], r = [1, 3, 2, 1], 200 points, hat-function tables, targets from a second seeded train, 3 sweeps, each core in
    turn, the exact step alpha = <G_i, G_i> / sum_p f_(U_i <- G_i)(x_p)^2 computed on the host from basis_tab"""
    _clear(monkeypatch)
    start, phis, y = C.fit_problem()
    tab = B.hstack(phis)
    want, fitted = C.fit_numpy()
    tt = E.TTCross.from_cores(start)
    losses = []
    for _ in range(C.FIT_SWEEPS):
        for i in range(3):
            val, G = tt.basis_core_grad_tab(tab, tt.basis_tab(tab, "exact") - y, "exact")
            losses.append(C.fit_loss(val, y))
            cores = [tt.core(k + 1) for k in range(3)]
            f_dir = E.TTCross.from_cores(C.replaced(cores, i, G[i])).basis_tab(tab, "exact")
            alpha = np.zeros(3)
            alpha[i] = C.fit_step(G[i], f_dir)
            tt.cores_axpy(alpha, G)
    losses.append(C.fit_loss(tt.basis_tab(tab, "exact"), y))
    assert losses == want, (losses, want)
    assert all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] < losses[0]
    for k in range(3):
        assert _eq(tt.core(k + 1), fitted[k])
    # MFMA mode: the same loop, the same property -- the loss falls at every step and ends below its start
    tt = E.TTCross.from_cores(start)
    losses = []
    for _ in range(C.FIT_SWEEPS):
        for i in range(3):
            val, G = tt.basis_core_grad_tab(tab, tt.basis_tab(tab, "mfma") - y, "mfma")
            losses.append(C.fit_loss(val, y))
            cores = [tt.core(k + 1) for k in range(3)]
            alpha = np.zeros(3)
            alpha[i] = C.fit_step(G[i], E.TTCross.from_cores(C.replaced(cores, i, G[i])).basis_tab(tab, "mfma"))
            tt.cores_axpy(alpha, G)
    losses.append(C.fit_loss(tt.basis_tab(tab, "mfma"), y))
    assert all(b < a for a, b in zip(losses, losses[1:])) and losses[-1] < losses[0], losses


@pytest.mark.parametrize("what", ["coord", "weight"])
def test_a_nan_coordinate_or_weight_gives_nan_where_documented(what):
    """in a child process: whatever a NaN does to a kernel, it does not take this process with it"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "basis_core_grad_nan_worker.py"), what], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert res[mode] == dict(clean_finite=True, val_as_documented=True, g_all_nan=True, clean_again_equal=True), (what, mode, res[mode])


def test_empty_calls_refusals_and_figures(monkeypatch):
    _clear(monkeypatch)
    L = E.load_library()
    cs = _case("mixed", False)
    tt, n, r = cs["tt"], cs["n"], cs["r"]
    EINVAL, ESTATE, nul = 1, 4, ctypes.POINTER(ctypes.c_double)()
    total = int(tt.core_offsets()[-1])
    assert total == sum(u.size for u in cs["cores"])
    x, c4, val = np.full((4, 5), 0.5), np.ones(4), np.zeros(4)
    arr = (E._Basis * 5)(*[E._Basis(E.TTX_BASIS_COS, 0, 0.0, 1.0, None) for _ in range(5)])
    t4 = np.ascontiguousarray(cs["tab"][:4])
    g = np.full(total, 7.0)

    def refused(rc, entry):
        return rc == EINVAL and entry in L.ttx_last_error().decode() and np.all(g == 7.0)

    # npts = 0: accumulate = 0 writes 0.0 to all of g, accumulate = 1 touches nothing; no chain is launched
    assert L.ttx_basis_core_grad_tab(tt._h, 0, nul, nul, nul, E._dp(g), 1, 0) == 0 and np.all(g == 7.0)
    assert L.ttx_basis_core_grad_batch(tt._h, 0, nul, None, nul, nul, E._dp(g), 1, 1) == 0 and np.all(g == 7.0)
    assert L.ttx_basis_core_grad_tab(tt._h, 0, nul, nul, nul, nul, 0, 0) == 0
    z = np.full(total, 7.0)
    assert L.ttx_basis_core_grad_tab(tt._h, 0, nul, nul, nul, E._dp(z), 0, 2) == 0 and not z.any() and not np.signbit(z).any()
    last = tt.basis_core_grad_last()
    assert last["flops"] == 0.0 and last["chunk"] == 0 and last["ms_back"] == 0.0 and last["ms_acc"] == 0.0
    v0, g0 = tt.basis_core_grad_tab(np.zeros((0, sum(n))), np.zeros(0), "mfma")
    assert v0.shape == (0,) and all(not b.any() for b in g0)
    # a null c, g or table, an unknown mode, negative npts, an accumulate that is neither 0 nor 1
    tab_ = "ttx_basis_core_grad_tab:"
    assert refused(L.ttx_basis_core_grad_tab(tt._h, 4, E._dp(t4), nul, E._dp(val), E._dp(g), 0, 0), tab_)
    assert L.ttx_basis_core_grad_tab(tt._h, 4, E._dp(t4), E._dp(c4), E._dp(val), nul, 0, 0) == EINVAL
    assert refused(L.ttx_basis_core_grad_tab(tt._h, 4, nul, E._dp(c4), E._dp(val), E._dp(g), 0, 0), tab_)
    assert refused(L.ttx_basis_core_grad_tab(tt._h, 4, E._dp(t4), E._dp(c4), E._dp(val), E._dp(g), 0, 3), tab_)
    assert refused(L.ttx_basis_core_grad_tab(tt._h, -1, E._dp(t4), E._dp(c4), E._dp(val), E._dp(g), 0, 0), tab_)
    for acc in (2, -1):
        assert refused(L.ttx_basis_core_grad_tab(tt._h, 4, E._dp(t4), E._dp(c4), E._dp(val), E._dp(g), acc, 0), tab_)
        assert "accumulate" in L.ttx_last_error().decode()
    assert refused(L.ttx_basis_core_grad_tab_dev(tt._h, 4, None, None, None, None, 0, 0), "ttx_basis_core_grad_tab_dev:")
    bat = "ttx_basis_core_grad_batch:"
    assert refused(L.ttx_basis_core_grad_batch(tt._h, 4, E._dp(x), None, E._dp(c4), E._dp(val), E._dp(g), 0, 0), bat)
    assert refused(L.ttx_basis_core_grad_batch(tt._h, 4, E._dp(x), arr, nul, E._dp(val), E._dp(g), 0, 0), bat)
    assert refused(L.ttx_basis_core_grad_batch(tt._h, 4, E._dp(x), arr, E._dp(c4), E._dp(val), E._dp(g), 0, 7), bat)
    assert refused(L.ttx_basis_core_grad_batch_dev(tt._h, 4, None, arr, None, None, None, 0, 0), "ttx_basis_core_grad_batch_dev:")
    arr2 = (E._Basis * 5)(*([arr[0]] * 3 + [E._Basis(9, 0, 0.0, 1.0, None)] + [arr[0]]))       # an unknown kind, before any launch
    assert refused(L.ttx_basis_core_grad_batch(tt._h, 4, E._dp(x), arr2, E._dp(c4), E._dp(val), E._dp(g), 0, 0), bat + " mode 4")
    al = np.ones(5)
    assert L.ttx_cores_axpy(tt._h, nul, E._dp(g)) == EINVAL and L.ttx_cores_axpy(tt._h, E._dp(al), nul) == EINVAL
    assert L.ttx_cores_axpy_dev(tt._h, E._dp(al), None) == EINVAL and "ttx_cores_axpy_dev:" in L.ttx_last_error().decode()
    with pytest.raises(ValueError):
        tt.basis_core_grad(x, [("cos", 0.0, 1.0)] * 4, c4)
    with pytest.raises(ValueError):
        tt.basis_core_grad_tab(cs["tab"][:4], np.ones(5))
    with pytest.raises(ValueError):
        tt.basis_core_grad_tab(cs["tab"][:4], c4, accumulate=True)                # accumulate needs something to add onto
    with pytest.raises(ValueError):
        tt.cores_axpy(1.0, np.zeros(total - 1))
    # ranks above 128 and boundary ranks other than 1: no engine can hold such a train, so these two refusals are the plan's
    # (tests/basis_core_grad_plan_main.cpp walks them); what exists is checked -- the engine refuses the train itself
    with pytest.raises(E.TTXError, match="1..128"):
        E.TTCross.from_cores([np.ones((1, 2, 129)), np.ones((129, 2, 1))])
    # an engine without a train (five modes, as the tables here): TTX_ESTATE
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    assert L.ttx_basis_core_grad_tab(fresh._h, 4, E._dp(t4), E._dp(c4), E._dp(val), E._dp(g), 0, 0) == ESTATE and np.all(g == 7.0)
    assert L.ttx_basis_core_grad_batch(fresh._h, 4, E._dp(x), arr, E._dp(c4), E._dp(val), E._dp(g), 0, 0) == ESTATE
    assert L.ttx_cores_axpy(fresh._h, E._dp(al), E._dp(g)) == ESTATE
    # val may be null; the figures of the last call; auto is one of the two modes
    w = sum(r[k] * n[k] * r[k + 1] for k in range(5))
    tab, c = np.ascontiguousarray(cs["tab"]), np.ascontiguousarray(cs["c"])
    res = {m: tt.basis_core_grad_tab(tab, c, m) for m in MODES}
    for m in MODES:
        g2 = np.full(total, 7.0)
        assert L.ttx_basis_core_grad_tab(tt._h, PMAX, E._dp(tab), E._dp(c), nul, E._dp(g2), 0, E.EVAL_MODES[m]) == 0
        assert _eq(g2, np.concatenate([b.ravel(order="F") for b in res[m][1]])), m
        tt.basis_core_grad_tab(tab[:257], c[:257], m)
        last = tt.basis_core_grad_last()
        assert last["mode"] == m and last["flops"] == 6.0 * 257 * w and last["chunk"] == 257
        assert last["ms_back"] > 0.0 and last["ms_fwd"] > 0.0 and last["ms_acc"] > 0.0 and last["ms_table"] == 0.0
    av, ag = tt.basis_core_grad_tab(tab, c, "auto")
    ran = tt.basis_core_grad_last()["mode"]
    assert ran in MODES and _eq(av, res[ran][0]) and _eqs(ag, res[ran][1])
    for k, core in enumerate(cs["cores"]):                                      # the train is untouched
        assert np.array_equal(tt.core(k + 1), core)
