"""The Gauss-Newton / Levenberg-Marquardt solver on the device: ttx_basis_fit_tab, ttx_basis_fit_batch (controller
ttcross_amd/csrc/ttx_fit_plan.h, kernels ttx_basis_jvp.h and ttx_basis_core_grad.h).

The checker of exact mode is basis_jvp_ref.fit_numpy, the controller restated in numpy operation by operation on jvp_chain,
core_grad_chain and the fixed-order dot: the history and the final cores must equal it bit for bit.  The problem is
basis_core_grad_ref.fit_problem(): n = [5, 6, 4], r = [1, 3, 2, 1], 200 points, hat-function tables, targets from a second train.
From the truth perturbed by 10 % per entry the numpy solver goes from a loss of 0.6 - 0.9 to 3e-30 in 12 iterations, so the bound
of 1e-20 of the initial loss asked of both device modes leaves ten orders of margin."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import basis_core_grad_ref as C
import basis_jvp_ref as J
import basis_ref as B
import tt_ref as R
from test_gpu_basis_core_grad import SHAPES
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

MODES = ("exact", "mfma")
PINNED = dict(max_iter=6, lambda0=1.0, cg_max=40, cg_tol=1e-2)                  # the random start of fit_problem()
NEAR = dict(max_iter=12, lambda0=1e-2, cg_max=60, cg_tol=1e-3)                  # the truth perturbed by 10 % per entry


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same(h1, h2):
    return (_eq(h1["loss"], h2["loss"]) and _eq(h1["lambda_"], h2["lambda_"]) and np.array_equal(h1["cg_iters"], h2["cg_iters"])
            and np.array_equal(h1["accepted"], h2["accepted"]) and h1["iters"] == h2["iters"])


def test_exact_mode_follows_the_numpy_solver_bit_for_bit(monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    monkeypatch.delenv("TTX_BASIS_GRAD_STORE", raising=False)
    start, phis, y = C.fit_problem()
    tab = B.hstack(phis)
    want = J.fit_numpy(start, phis, y, **PINNED)
    assert want["accepted"].sum() >= 1 and (want["accepted"] == 0).sum() >= 1   # both branches of the schedule are walked
    tt = E.TTCross.from_cores(start)
    got = tt.fit_tab(tab, y, mode="exact", **PINNED)
    print("loss", got["loss"], "lambda", got["lambda_"], "cg", got["cg_iters"], "accepted", got["accepted"])
    assert _same(got, want), (got, want)
    assert got["stop"] == "max_iter" and want["stop"] == 1
    for k in range(3):
        assert _eq(tt.core(k + 1), want["cores"][k]), k
    # the engine's train gives the last reported loss bit for bit: a rejected step was restored, not subtracted
    res = tt.basis_tab(tab, "exact") - y
    assert _bits(0.5 * J.dot(res, res)) == _bits(got["loss"][-1])
    last = tt.fit_last()
    assert last["mode"] == "exact" and last["n_jvp"] == want["n_jvp"] == int(got["cg_iters"].sum()) and last["n_core_grad"] == want["n_core_grad"]
    # chunks change no bit of the exact solver
    monkeypatch.setenv("TTX_BASIS_CHUNK", "64")
    monkeypatch.setenv("TTX_BASIS_GRAD_STORE", "1")
    tt2 = E.TTCross.from_cores(start)
    again = tt2.fit_tab(tab, y, mode="exact", max_iter=2, lambda0=1.0, cg_max=40, cg_tol=1e-2)
    assert _eq(again["loss"], want["loss"][:3]) and np.array_equal(again["cg_iters"], want["cg_iters"][:2])


@pytest.mark.parametrize("mode", MODES)
def test_from_near_the_truth_the_loss_never_rises_and_falls_twenty_orders(mode, monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    monkeypatch.delenv("TTX_BASIS_GRAD_STORE", raising=False)
    _, phis, y = C.fit_problem()
    tab = B.hstack(phis)
    start = J.perturbed_truth(1)
    tt = E.TTCross.from_cores(start)
    h = tt.fit_tab(tab, y, mode=mode, **NEAR)
    print(mode, "loss", h["loss"], "accepted", h["accepted"], "cg", h["cg_iters"])
    assert np.all(h["loss"][1:] <= h["loss"][:-1])
    assert np.all(np.isfinite(h["loss"])) and h["loss"][-1] <= 1e-20 * h["loss"][0]
    assert tt.fit_last()["mode"] == mode
    # w = 0 on half the points gives the fit of the other half: the masked points' targets change no bit of the result
    w = (np.arange(y.size) % 2 == 0).astype(np.float64)
    y2 = y.copy()
    y2[w == 0.0] = y2[w == 0.0] * -3.0 + 17.0
    runs = []
    for yy in (y, y2):
        e = E.TTCross.from_cores(start)
        runs.append((e.fit_tab(tab, yy, w, mode=mode, **NEAR), e.cores_get()))
    assert _same(runs[0][0], runs[1][0]) and _eq(runs[0][1], runs[1][1])
    hw = runs[0][0]
    print(mode, "half: loss", hw["loss"], "accepted", hw["accepted"], "cg", hw["cg_iters"])
    assert np.all(hw["loss"][1:] <= hw["loss"][:-1]) and hw["loss"][-1] < hw["loss"][0]
    # it is the other half's problem: the loss at entry is the sum over the kept points alone -- 100 non-negative terms, so within
    # (100 + 1) u relative of their sum in any order, and the value chain adds its own bound twice over (the residual is squared)
    res = B.chain(start, phis) - y
    kept = 0.5 * float(np.sum(res[w == 1.0] ** 2))
    slack = 101 * B.U * kept + float(np.sum(np.abs(res[w == 1.0]) * 2.0 * B.bound(start, phis)[w == 1.0]))
    assert abs(hw["loss"][0] - kept) <= slack and hw["loss"][0] < h["loss"][0]
    if mode == "exact":                                                         # and the weighted solver is the weighted restatement, bit for bit
        short = dict(NEAR, max_iter=3)                                          # three iterations of the restatement; the solver does not look ahead
        want = J.fit_numpy(start, phis, y, w, **short)
        e = E.TTCross.from_cores(start)
        got = e.fit_tab(tab, y, w, mode="exact", **short)
        assert _same(got, want) and _eq(e.cores_get(), J.pack(want["cores"]))
        assert _eq(hw["loss"][:4], want["loss"]) and np.array_equal(hw["cg_iters"][:3], want["cg_iters"])


def test_mixed_shape_300_points_on_the_matrix_cores(monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    monkeypatch.delenv("TTX_BASIS_GRAD_STORE", raising=False)
    n, r = SHAPES["mixed"]
    rng = np.random.default_rng(300)
    truth = R.rand_train(300, n, r)
    phis = [rng.standard_normal((300, nk)) for nk in n]
    tab = B.hstack(phis)
    y = B.chain(truth, phis)
    tt = E.TTCross.from_cores([u * (1.0 + 0.01 * rng.uniform(-1.0, 1.0, u.shape)) for u in truth])
    h = tt.fit_tab(tab, y, mode="mfma", max_iter=4, cg_max=10, lambda0=1e-2, cg_tol=1e-3)
    print("loss", h["loss"], "accepted", h["accepted"], "cg", h["cg_iters"])
    assert np.all(h["loss"][1:] <= h["loss"][:-1]) and h["loss"][-1] < h["loss"][0]
    assert h["stop"] == "max_iter" and h["iters"] == 4
    last = tt.fit_last()
    assert last["mode"] == "mfma" and last["n_jvp"] == int(h["cg_iters"].sum())
    assert last["n_core_grad"] == int(h["cg_iters"].sum()) + 1 + int(h["accepted"][:-1].sum())     # one gradient at entry and one after every accepted step that another iteration follows
    assert last["ms_jvp"] > 0.0 and last["ms_core_grad"] > 0.0 and last["ms_value"] > 0.0 and last["ms_vector"] > 0.0
    res = tt.basis_tab(tab, "mfma") - y
    assert _bits(0.5 * J.dot(res, res)) == _bits(h["loss"][-1])


def test_stop_reasons_refusals_and_an_untouched_train(monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    L = E.load_library()
    start, phis, y = C.fit_problem()
    tab = B.hstack(phis)
    tt = E.TTCross.from_cores(start)
    # loss_tol met at entry, and after the first accepted step; every array is filled past the iterations that ran
    h = tt.fit_tab(tab, y, mode="exact", max_iter=3, loss_tol=1e9)
    assert h["stop"] == "loss_tol" and h["iters"] == 0 and np.all(h["loss"] == h["loss"][0]) and np.all(h["lambda_"] == 1.0) and not h["cg_iters"].any()
    h = tt.fit_tab(tab, y, mode="exact", max_iter=3, loss_tol=100.0)
    assert h["stop"] == "loss_tol" and h["iters"] == 1 and h["accepted"].tolist() == [1, 0, 0] and h["loss"][1] <= 100.0 < h["loss"][0]
    assert np.all(h["loss"][1:] == h["loss"][1]) and h["lambda_"].tolist() == [1.0, 0.3, 0.3]
    # a non-finite loss at entry; a zero gradient with a loss that is not zero (two zero cores)
    tt = E.TTCross.from_cores(start)
    yn = y.copy()
    yn[7] = np.nan
    h = tt.fit_tab(tab, yn, mode="exact", max_iter=2)
    assert h["stop"] == "non_finite" and h["iters"] == 0 and np.isnan(h["loss"]).all()
    for k in range(3):
        assert _eq(tt.core(k + 1), start[k])
    zero = E.TTCross.from_cores([np.zeros(start[0].shape), start[1], np.zeros(start[2].shape)])
    h = zero.fit_tab(tab, y, mode="mfma", max_iter=2)
    assert h["stop"] == "zero_gradient" and h["iters"] == 0 and h["loss"][0] > 0.0 and zero.fit_last()["n_core_grad"] == 1
    # refusals leave the train alone
    EINVAL, ESTATE, nul = 1, 4, ctypes.POINTER(ctypes.c_double)()
    res = E._FitResult()

    def call(npts=200, t=tab, yy=y, w=None, null_opts=False, **o):
        f = dict(E.FIT_DEFAULTS, mode=0)
        f.update(o)
        fo = E._FitOpts(f["max_iter"], f["cg_max"], f["max_reject"], f["mode"], f["lambda0"], f["lambda_down"], f["lambda_up"], f["cg_tol"], f["loss_tol"])
        return L.ttx_basis_fit_tab(tt._h, npts, E._dp(t) if t is not None else nul, E._dp(yy) if yy is not None else nul, E._dp(w) if w is not None else nul,
                                   None if null_opts else ctypes.byref(fo), nul, nul, None, None, ctypes.byref(res))

    wneg, wnan = np.ones(200), np.ones(200)
    wneg[3], wnan[5] = -1.0, np.nan
    for kw in (dict(npts=0), dict(npts=-1), dict(t=None), dict(yy=None), dict(null_opts=True), dict(w=wneg), dict(w=wnan), dict(max_iter=-1), dict(cg_max=0),
               dict(max_reject=0), dict(mode=3), dict(lambda0=0.0), dict(lambda0=np.inf), dict(lambda_down=0.0), dict(lambda_down=1.5), dict(lambda_up=0.5),
               dict(cg_tol=-1.0), dict(loss_tol=np.nan)):
        assert call(**kw) == EINVAL and "ttx_basis_fit_tab:" in L.ttx_last_error().decode(), kw
    assert call(max_iter=0) == 0 and res.iters == 0 and res.stop == 1            # nothing to do is no error; all history pointers may be null
    for k in range(3):
        assert _eq(tt.core(k + 1), start[k])
    with pytest.raises(ValueError):
        tt.fit_tab(tab, y, no_such_option=1)
    with pytest.raises(ValueError):
        tt.fit_tab(tab, y[:-1])
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    fo = E._FitOpts(1, 1, 1, 0, 1.0, 0.3, 4.0, 1e-2, 0.0)
    assert L.ttx_basis_fit_tab(fresh._h, 200, E._dp(tab), E._dp(y), nul, ctypes.byref(fo), nul, nul, None, None, None) == ESTATE
