"""Ranks grown from data on the device: ttx_basis_enrich_batch / ttx_basis_enrich_tab (ttcross_amd/csrc/ttx_basis_enrich.h).

The checker is tests/enrich_ref.py: sketch restates steps 1 - 5 of include/ttx.h in numpy, and exact mode must equal it bit for bit (Y,
ynorm2, added).  MFMA mode sums in another order; its bound is the one derived in enrich_ref's docstring, 2 N_b u B_b.  The new
directions are compared by what a Householder QR pins down: the projector Q_b Q_b^T and |R_qq|, never Q_b's bits.

Allowances of the structure and span tests, for a bond with rows = r(b-1) n(b), cols = r(b) + k_b.  A Householder QR is column-wise
backward stable: the computed Q is within gamma = c rows cols u of an exactly orthonormal matrix that factors a matrix whose columns are
within gamma of the given ones, relative to each column's own norm (Higham, Accuracy and Stability, Thm 19.4 and 19.13), c a small
integer.  That worst case grows with cols; the structure test holds Q_b^T Q_b - I, and U^L^T Q_b relative to ||U^L||_2, to the form the
feature was specified with, STRUCT = 8 rows u, without the factor cols.  The span of Q_b is the range of
M = (I - P_U) Y_b; a perturbation of Y_b's columns by gamma ||Y_b|| turns it by at most gamma ||Y_b||_2 / sigma_min(M), and one of U^L's
columns turns P_U by gamma cond(U^L), which reaches M with the same factor.  The device's and numpy's QR each deviate by that much, so
the projectors differ by at most SPAN = 2 (8 rows cols u) (||Y_b||_2 / sigma_min(M)) cond(U^L).  The test first asserts on the CPU, from the
restatement alone, that cond(M) < 1e6 (c and the seed are chosen so); ||Y_b||_2 / sigma_min(M) >= cond(M) is what the bound needs.
One bond of test_gpu_basis_core_grad.SHAPES cannot satisfy that for any c and seed: at bond 2 of two_rows_mr5 the right factor
phi_3 (x) X_3 spans 3 * 2 = 6 directions, so Y_2 has rank 6 under its k = 20 columns (enrich_ref.sketch_rank).  There sigma_min is the
sixth singular value, the condition is asserted over those six, and the new columns must contain the six-dimensional range of M within
the same allowance; the other fourteen are an orthonormal completion, which the structure test checks.  Each shape's references are
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
import enrich_ref as N
import tt_ref as R
from test_gpu_basis_core_grad import SHAPES as CG_SHAPES
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = dict(CG_SHAPES)
SHAPES["tiles"] = ([4, 6, 5, 6, 4], [1, 4, 15, 17, 4, 1])                      # new ranks 24 and 37; k and r + k cross the 16-tile
SHAPES["wide"] = ([30, 30, 30], [1, 2, 2, 1])                                  # k = 20 against ranks of 2: the k_i, not the ranks, set the stride of every state row (20 instead of 4)
EXPECT_K = {"mixed": [4, 0, 4, 1], "ragged": [1, 0, 5], "d2": [2], "bond128": [0, 0], "tiles": [0, 9, 20, 4], "wide": [20, 20]}
NPTS = (1, 5, 17, 65, 257, 300)
CHUNKED = (65, 257, 300)                                                    # with TTX_BASIS_CHUNK=64: the counts that make more than one chunk (a new engine per call costs a quarter of a second)
PMAX, ADD, SEED = max(NPTS), 20, 11
MODES = ("exact", "mfma")
CHUNK_VARS = ("TTX_BASIS_CHUNK", "TTX_BASIS_GRAD_STORE", "TTX_ENRICH_AUTO_FLOPS")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _eqs(ga, gb):
    return len(ga) == len(gb) and all(_eq(a, b) for a, b in zip(ga, gb))


def _clear(monkeypatch):
    for v in CHUNK_VARS:
        monkeypatch.delenv(v, raising=False)


@functools.lru_cache(maxsize=None)
def _case(name):
    """cores, the engine, the tables and weights of PMAX points: computed once, never changed"""
    n, r = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 7)
    cores = R.rand_train(sum(map(ord, name)), n, r)
    phis = [rng.standard_normal((PMAX, nk)) for nk in n]
    c = rng.standard_normal(PMAX)
    tab = B.hstack(phis)
    for a in (tab, c):
        a.setflags(write=False)
    return dict(n=n, r=r, d=len(n), cores=cores, phis=phis, c=c, tab=tab, tt=E.TTCross.from_cores(cores), k=N.plan_k(n, r, ADD))


@functools.lru_cache(maxsize=None)
def _ref(name, p):
    """the restatement's sketch at the first p points"""
    cs = _case(name)
    return N.sketch(cs["cores"], [ph[:p] for ph in cs["phis"]], cs["c"][:p], ADD, SEED)


@functools.lru_cache(maxsize=None)
def _bound(name, p):
    cs = _case(name)
    return N.bound(cs["cores"], [ph[:p] for ph in cs["phis"]], cs["c"][:p], ADD, SEED)


def _want_added(sk):
    return [k if m > 0.0 and np.isfinite(m) else 0 for k, m in zip(sk["k"], sk["maxabs"])]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_exact_is_the_numpy_restatement_bit_for_bit(name, monkeypatch):
    cs = _case(name)
    tt = cs["tt"]
    if name in EXPECT_K:
        assert cs["k"] == EXPECT_K[name]
    for chunk in (None, "64"):
        _clear(monkeypatch)
        if chunk:
            monkeypatch.setenv("TTX_BASIS_CHUNK", chunk)
        for p in (NPTS if not chunk else CHUNKED):
            sk = _ref(name, p)
            new, info = tt.enrich_tab(cs["tab"][:p], cs["c"][:p], ADD, SEED, "exact", want_sketch=True)
            assert info["k"] == cs["k"] and info["added"] == _want_added(sk), (chunk, p)
            assert _eqs(info["y"], sk["y"]) and _eq(info["ynorm2"], np.array(sk["ynorm2"])), (chunk, p)
            assert [int(v) for v in new.ranks()] == [1] + [cs["r"][b] + info["added"][b - 1] for b in range(1, cs["d"])] + [1]
            last = tt.enrich_last()
            assert last["mode"] == "exact" and last["chunk"] == (min(p, 64) if chunk else p) * (max(cs["k"]) > 0)
            new.close()


def _bases(n, rng):
    basis, cols = [], []
    for k, nk in enumerate(n):
        if k % 2 == 0:
            a, b = -1.0 - k, 2.5 + k
            basis.append(("cos", a, b, True) if k % 4 == 0 else ("cos", a, b))
            x = rng.uniform(a, b, PMAX)
        else:
            t = np.sort(rng.uniform(-2.0, 3.0, nk))
            basis.append(("linear", t))
            x = rng.uniform(t[0] - 0.5, t[-1] + 0.5, PMAX)
        cols.append(x)
    return basis, np.ascontiguousarray(np.stack(cols, axis=1))


@pytest.mark.parametrize("name", ["mixed", "tiles"])
def test_coordinates_give_what_the_host_tables_give_bit_for_bit(name, monkeypatch):
    cs = _case(name)
    tt, n, c = cs["tt"], cs["n"], cs["c"]
    basis, x = _bases(n, np.random.default_rng(41))
    phis = [E.basis_table(e, nk, x[:, k]) for k, (e, nk) in enumerate(zip(basis, n))]
    want = N.sketch(cs["cores"], phis, c, ADD, SEED)
    for chunk in (None, "64"):
        _clear(monkeypatch)
        if chunk:
            monkeypatch.setenv("TTX_BASIS_CHUNK", chunk)
        new, info = tt.enrich(x, basis, c, ADD, SEED, "exact", want_sketch=True)
        assert _eqs(info["y"], want["y"]) and _eq(info["ynorm2"], np.array(want["ynorm2"])) and info["added"] == want["k"], chunk
        assert tt.enrich_last()["ms_table"] > 0.0
        new.close()
        wn, wi = tt.enrich_tab(B.hstack(phis), c, ADD, SEED, "mfma", want_sketch=True)
        new, info = tt.enrich(x, basis, c, ADD, SEED, "mfma", want_sketch=True)
        assert _eqs(info["y"], wi["y"]) and all(_eq(new.core(i + 1), wn.core(i + 1)) for i in range(cs["d"])), chunk
        new.close()
        wn.close()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_structure_of_every_new_core_and_the_function_is_kept(name, monkeypatch):
    _clear(monkeypatch)
    cs = _case(name)
    n, r, d, k = cs["n"], cs["r"], cs["d"], cs["k"]
    rng = np.random.default_rng(5)
    fresh = rng.standard_normal((40, sum(n)))
    ind = np.stack([rng.integers(1, nk + 1, 40) for nk in n], axis=1).astype(np.int32)
    for mode in MODES:
        for p in (1, PMAX):
            new, info = cs["tt"].enrich_tab(cs["tab"][:p], cs["c"][:p], ADD, SEED, mode)
            assert info["added"] == k
            ka = [0] + k + [0]
            for i in range(d):
                U, G = cs["cores"][i], new.core(i + 1)
                assert G.shape == (r[i] + ka[i], n[i], r[i + 1] + ka[i + 1])
                assert _eq(G[:r[i], :, :r[i + 1]], U), (mode, p, i)             # the source's block, bit for bit
                assert not G[r[i]:].any() and not np.signbit(G[r[i]:]).any(), (mode, p, i)      # padded rows exactly +0.0
                if ka[i + 1]:
                    rows = r[i] * n[i]
                    Q, UL = G[:r[i], :, r[i + 1]:].reshape((rows, ka[i + 1]), order="F"), U.reshape((rows, r[i + 1]), order="F")
                    allow = 8 * rows * B.U
                    eo, eu = np.max(np.abs(Q.T @ Q - np.eye(ka[i + 1]))), np.max(np.abs(UL.T @ Q)) / np.linalg.norm(UL, 2)
                    print(name, mode, p, "bond", i + 1, "Q^T Q - I / allowance", eo / allow, "U^T Q / allowance", eu / allow)
                    assert eo <= allow and eu <= allow, (mode, p, i)
            # the same function: in exact mode the value chains are equal, at fresh points and at fresh indices
            assert _eq(new.basis_tab(fresh, "exact"), cs["tt"].basis_tab(fresh, "exact")), (mode, p)
            assert _eq(new.tijk_batch(ind, "exact"), cs["tt"].tijk_batch(ind, "exact")), (mode, p)
            new.close()
    for i in range(d):                                                          # the source is untouched
        assert _eq(cs["tt"].core(i + 1), cs["cores"][i])


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_new_directions_span_what_numpys_qr_spans_and_gain_is_its_r(name, monkeypatch):
    _clear(monkeypatch)
    cs = _case(name)
    n, r, d, k = cs["n"], cs["r"], cs["d"], cs["k"]
    sk = _ref(name, PMAX)
    rho = {b: N.sketch_rank(n, b, k[b - 1]) for b in range(1, d) if k[b - 1]}
    conds = {b: N.projected_cond(cs["cores"][b - 1], sk["y"][b - 1], rho[b]) for b in rho}
    assert all(v < 1e6 for v in conds.values()), conds                          # on the CPU, from the restatement alone
    if name == "two_rows_mr5":
        assert rho == {2: 6, 3: 2}                                              # bond 2: phi_3 (x) X_3 spans 3 * 2 directions, fewer than k = 20
    else:
        assert all(rho[b] == k[b - 1] for b in rho)
    new, info = cs["tt"].enrich_tab(cs["tab"], cs["c"], ADD, SEED, "exact")
    for b in range(1, d):
        kb = k[b - 1]
        if not kb:
            assert info["gain"][b - 1].size == 0
            continue
        U, y = cs["cores"][b - 1], sk["y"][b - 1]
        rows, cols = r[b - 1] * n[b - 1], r[b] + kb
        Qn, gn, _ = N.new_directions(U, y)
        Q = new.core(b)[:r[b - 1], :, r[b]:].reshape((rows, kb), order="F")
        UL, Ym = U.reshape((rows, r[b]), order="F"), y.reshape((rows, kb), order="F")
        M, s = N.projected(U, y)
        ynorm = np.linalg.norm(Ym, 2)
        allow = 2 * 8 * rows * cols * B.U * (ynorm / s[rho[b] - 1]) * np.linalg.cond(UL)
        if rho[b] == kb:
            err = np.max(np.abs(N.projector(Q) - N.projector(Qn)))
        else:
            # the shapes leave the sketch rank-deficient: the QR pins down the span of its rho directions, which the new columns must
            # contain; the other k - rho columns are any orthonormal completion (the structure test holds them to that)
            W = np.linalg.svd(M, full_matrices=False)[0][:, :rho[b]]
            err = max(np.max(np.abs(W - Q @ (Q.T @ W))), np.max(np.abs(W - Qn @ (Qn.T @ W))))
        gerr = np.max(np.abs(info["gain"][b - 1] - gn))
        print(name, "bond", b, "cond", conds[b], "projector err / allowance", err / allow, "gain err / (allowance ||Y||)", gerr / (allow * ynorm))
        assert err <= allow and allow < 1e-6, b
        assert gerr <= allow * ynorm, b
        assert float(np.sum(info["gain"][b - 1] ** 2)) <= info["ynorm2"][b - 1] * (1.0 + 1e-9)
    new.close()


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mfma_is_within_the_derived_bound_and_repeats_bit_for_bit(name, monkeypatch):
    cs = _case(name)
    tt = cs["tt"]
    for chunk in (None, "64"):
        _clear(monkeypatch)
        if chunk:
            monkeypatch.setenv("TTX_BASIS_CHUNK", chunk)
        for p in (NPTS if not chunk else CHUNKED):
            sk, bnd = _ref(name, p), _bound(name, p)
            new, info = tt.enrich_tab(cs["tab"][:p], cs["c"][:p], ADD, SEED, "mfma", want_sketch=True)
            assert tt.enrich_last()["mode"] == "mfma" and info["added"] == _want_added(sk)
            for b in range(1, cs["d"]):
                err = np.abs(info["y"][b - 1] - sk["y"][b - 1])
                if err.size:
                    with np.errstate(invalid="ignore", divide="ignore"):
                        print(name, chunk, p, "bond", b, "max err / bound", float(np.nanmax(np.where(bnd[b - 1] > 0, err / bnd[b - 1], 0.0))))
                assert np.all(err <= bnd[b - 1]), (chunk, p, b)
            if (p, chunk) in ((17, None), (PMAX, "64")):
                again, ai = tt.enrich_tab(cs["tab"][:p], cs["c"][:p], ADD, SEED, "mfma", want_sketch=True)
                assert _eqs(ai["y"], info["y"]) and _eq(ai["ynorm2"], info["ynorm2"]) and _eqs(ai["gain"], info["gain"])
                assert all(_eq(again.core(i + 1), new.core(i + 1)) for i in range(cs["d"]))
                again.close()
            new.close()


def _loss(tt, tab, y, mode):
    res = tt.basis_tab(tab, mode) - y
    return 0.5 * float(np.sum(res * res))


@pytest.mark.parametrize("mode", MODES)
def test_one_enrichment_recovers_a_fit_that_stalled_below_the_true_ranks(mode, monkeypatch):
    """fit_problem(): the truth truncated to [1, 2, 1, 1], fit_tab, enrich_tab with add = [1, 1] and c = the residual, fit_tab again; the
    enriched-then-fitted loss is at most 1e-20 of the stalled one (the numpy route reaches about 4e-31 of it: test_enrich_cpu.py).
    The same by fit_adaptive in one call, ending at ranks [1, 3, 2, 1]."""
    _clear(monkeypatch)
    start, phis, y = N.recovery_start()
    tab = B.hstack(phis)
    tt = E.TTCross.from_cores(start)
    h1 = tt.fit_tab(tab, y, max_iter=24, mode=mode)
    stalled = float(h1["loss"][h1["iters"]])
    assert 6.8 < stalled < 6.9 and stalled == pytest.approx(_loss(tt, tab, y, mode), rel=1e-9)
    res = tt.basis_tab(tab, mode) - y
    new, info = tt.enrich_tab(tab, res, [1, 1], 0, mode)
    assert info["added"] == [1, 1] and [int(v) for v in new.ranks()] == [1, 3, 2, 1]
    assert _loss(new, tab, y, "exact") == _loss(tt, tab, y, "exact")           # the same function before the second fit
    h2 = new.fit_tab(tab, y, mode=mode)
    after = float(h2["loss"][h2["iters"]])
    print(mode, "stalled", stalled, "after", after, "ratio", after / stalled)
    assert after <= 1e-20 * stalled
    # fit_adaptive: coordinates and hat functions, the tables of fit_problem()
    rng = np.random.default_rng(20240521)
    for k in range(6):
        rng.standard_normal((C.FIT_R[k % 3], C.FIT_N[k % 3], C.FIT_R[k % 3 + 1]))
    x = rng.uniform(0.0, 1.0, (C.FIT_NPTS, 3))
    basis = [("linear", np.linspace(0.0, 1.0, nk)) for nk in C.FIT_N]
    t2 = E.TTCross.from_cores(start)
    assert np.allclose(t2.basis_batch(x, basis, "exact"), t2.basis_tab(tab, "exact"), rtol=1e-12, atol=1e-12)     # the same points as the tables
    grown, hist = t2.fit_adaptive(x, basis, y, add=1, rmax=[3, 2], rounds=4, mode=mode, max_iter=24)
    print(mode, [(h["ranks"], h["loss"], h["added"]) for h in hist])
    assert [int(v) for v in grown.ranks()] == [1, 3, 2, 1] and len(hist) == 2 and hist[0]["added"] == [1, 1] and hist[1]["added"] == [0, 0]
    assert 6.8 < hist[0]["loss"] < 6.9 and hist[1]["loss"] <= 1e-20 * hist[0]["loss"]
    for t in (new, grown):
        t.close()


def test_a_nan_weight_takes_no_direction_and_leaves_the_rest_intact():
    """in a child process: whatever a NaN does to a kernel, it does not take this process with it"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "enrich_nan_worker.py")], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert res[mode] == dict(clean_added=True, clean_finite=True, nan_added_none=True, nan_gain=True, nan_sketch=True, nan_train_is_a_copy=True,
                                 source_untouched=True, clean_again_equal=True), (mode, res[mode])


def test_zero_weights_empty_calls_refusals_and_figures(monkeypatch):
    _clear(monkeypatch)
    L = E.load_library()
    cs = _case("mixed")
    tt, n, r, d = cs["tt"], cs["n"], cs["r"], cs["d"]
    EINVAL, ESTATE, nul = 1, 4, ctypes.POINTER(ctypes.c_double)()

    def is_copy(t):
        return [int(v) for v in t.ranks()] == r and all(_eq(t.core(i + 1), cs["cores"][i]) for i in range(d))

    for mode in MODES:
        # c = 0: every term is a zero, no bond takes a direction, the new train is a plain copy
        new, info = tt.enrich_tab(cs["tab"], np.zeros(PMAX), ADD, SEED, mode, want_sketch=True)
        assert info["added"] == [0] * 4 and is_copy(new) and not any(y.any() for y in info["y"]) and not info["ynorm2"].any()
        assert all(not g.any() for g in info["gain"])
        new.close()
        # npts = 0: a zero sketch on every bond, no chain is launched
        new, info = tt.enrich_tab(np.zeros((0, sum(n))), np.zeros(0), ADD, SEED, mode, want_sketch=True)
        assert info["added"] == [0] * 4 and is_copy(new) and not info["ynorm2"].any() and [y.shape for y in info["y"]] == [(1, 7, 4), (3, 2, 0), (17, 51, 4), (5, 1, 1)]
        last = tt.enrich_last()
        assert last["flops"] == 0.0 and last["chunk"] == 0 and last["ms_back"] == 0.0 and last["ms_sketch"] == 0.0
        new.close()
        # add = 0 everywhere: a copy as well
        new, info = tt.enrich_tab(cs["tab"], cs["c"], 0, SEED, mode)
        assert info["added"] == [0] * 4 and info["k"] == [0] * 4 and is_copy(new)
        new.close()
    # refusals: *out is NULL afterwards
    t4, c4 = np.ascontiguousarray(cs["tab"][:4]), np.ones(4)
    add = np.full(4, 2, dtype=np.int32)
    x = np.full((4, 5), 0.5)
    arr = (E._Basis * 5)(*[E._Basis(E.TTX_BASIS_COS, 0, 0.0, 1.0, None) for _ in range(5)])
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))            # noqa: E731

    def refused(call, entry, code=EINVAL):
        out = ctypes.c_void_p(12345)
        rc = call(out)
        return rc == code and out.value is None and (code != EINVAL or entry in L.ttx_last_error().decode())

    tab_ = "ttx_basis_enrich_tab:"
    tail = (None, None, None, None)
    assert refused(lambda o: L.ttx_basis_enrich_tab(tt._h, 4, E._dp(t4), nul, ip(add), 1, 0, ctypes.byref(o), *tail), tab_)                  # a null c
    assert refused(lambda o: L.ttx_basis_enrich_tab(tt._h, 4, nul, E._dp(c4), ip(add), 1, 0, ctypes.byref(o), *tail), tab_)                  # a null table
    assert refused(lambda o: L.ttx_basis_enrich_tab(tt._h, 4, E._dp(t4), E._dp(c4), None, 1, 0, ctypes.byref(o), *tail), tab_)               # a null add
    assert L.ttx_basis_enrich_tab(tt._h, 4, E._dp(t4), E._dp(c4), ip(add), 1, 0, None, *tail) == EINVAL                                      # a null out
    assert refused(lambda o: L.ttx_basis_enrich_tab(tt._h, 4, E._dp(t4), E._dp(c4), ip(add), 1, 3, ctypes.byref(o), *tail), tab_)            # an unknown mode
    assert refused(lambda o: L.ttx_basis_enrich_tab(tt._h, -1, E._dp(t4), E._dp(c4), ip(add), 1, 0, ctypes.byref(o), *tail), tab_)
    neg = np.array([2, 2, -1, 2], dtype=np.int32)
    assert refused(lambda o: L.ttx_basis_enrich_tab(tt._h, 4, E._dp(t4), E._dp(c4), ip(neg), 1, 0, ctypes.byref(o), *tail), tab_ + " add(3)=-1")
    assert refused(lambda o: L.ttx_basis_enrich_tab_dev(tt._h, 4, None, None, ip(add), 1, 0, ctypes.byref(o), *tail), "ttx_basis_enrich_tab_dev:")
    bat = "ttx_basis_enrich_batch:"
    assert refused(lambda o: L.ttx_basis_enrich_batch(tt._h, 4, E._dp(x), None, E._dp(c4), ip(add), 1, 0, ctypes.byref(o), *tail), bat)      # a null basis
    arr2 = (E._Basis * 5)(*([arr[0]] * 3 + [E._Basis(9, 0, 0.0, 1.0, None)] + [arr[0]]))
    assert refused(lambda o: L.ttx_basis_enrich_batch(tt._h, 4, E._dp(x), arr2, E._dp(c4), ip(add), 1, 0, ctypes.byref(o), *tail), bat + " mode 4")
    assert refused(lambda o: L.ttx_basis_enrich_batch_dev(tt._h, 4, None, arr, None, ip(add), 1, 0, ctypes.byref(o), *tail), "ttx_basis_enrich_batch_dev:")
    # the storage check of step 1: 60 x 2000 is stored, 66 x 2000 is not -- refused before any device work, with the bond and the rank
    big = E.TTCross.from_cores([np.ones((1, 70, 60)), np.ones((60, 2000, 1))])
    tb, a6 = np.ones((2, 2070)), np.array([6], dtype=np.int32)
    assert refused(lambda o: L.ttx_basis_enrich_tab(big._h, 2, E._dp(tb), E._dp(np.ones(2)), ip(a6), 1, 0, ctypes.byref(o), *tail), tab_ + " the rank at bond 1 grows to 66")
    assert "maxrank*n too large" in L.ttx_last_error().decode()
    big.close()
    with pytest.raises(ValueError):
        tt.enrich_tab(cs["tab"][:4], np.ones(5), 1)
    with pytest.raises(ValueError):
        tt.enrich_tab(cs["tab"][:4], c4, -1)
    with pytest.raises(ValueError):
        tt.enrich(x, [("cos", 0.0, 1.0)] * 4, c4, 1)
    # an engine without a train: TTX_ESTATE
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    assert refused(lambda o: L.ttx_basis_enrich_tab(fresh._h, 4, E._dp(t4), E._dp(c4), ip(add), 1, 0, ctypes.byref(o), *tail), tab_, ESTATE)
    # every output but out may be null; the figures of the last call; auto is one of the two modes
    k = cs["k"]
    w = sum(r[i] * n[i] * r[i + 1] for i in range(d))
    ws = sum(k[b - 1] * (n[b] * r[b + 1] + r[b - 1] * n[b - 1]) for b in range(1, d))
    tab, c = np.ascontiguousarray(cs["tab"]), np.ascontiguousarray(cs["c"])
    a20 = np.full(4, ADD, dtype=np.int32)
    for m in MODES:
        out = ctypes.c_void_p()
        assert L.ttx_basis_enrich_tab(tt._h, 257, E._dp(tab), E._dp(c), ip(a20), SEED, E.EVAL_MODES[m], ctypes.byref(out), *tail) == 0 and out.value
        got = E.TTCross._adopt(out, tt.device)
        assert [int(v) for v in got.ranks()] == [1, 7, 17, 9, 5, 1]
        got.close()
        last = tt.enrich_last()
        assert last["mode"] == m and last["flops"] == 257 * (4.0 * w + 2.0 * ws) and last["chunk"] == 257
        assert last["ms_back"] > 0.0 and last["ms_sketch"] > 0.0 and last["ms_qr"] > 0.0 and last["ms_asm"] > 0.0 and last["ms_table"] == 0.0
    new, info = tt.enrich_tab(tab, c, ADD, SEED, "auto", want_sketch=True)
    ran = tt.enrich_last()["mode"]
    assert ran in MODES
    ref, ri = tt.enrich_tab(tab, c, ADD, SEED, ran, want_sketch=True)
    assert _eqs(info["y"], ri["y"])
    monkeypatch.setenv("TTX_ENRICH_AUTO_FLOPS", "1")                            # the break-even from the environment: everything is above 1 flop
    tt.enrich_tab(tab, c, ADD, SEED, "auto")[0].close()
    assert tt.enrich_last()["mode"] == "mfma"
    monkeypatch.setenv("TTX_ENRICH_AUTO_FLOPS", "1e30")
    tt.enrich_tab(tab, c, ADD, SEED, "auto")[0].close()
    assert tt.enrich_last()["mode"] == "exact"
    for t in (new, ref):
        t.close()
