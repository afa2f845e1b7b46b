"""The normaliser of the squared density, its gradient with respect to the cores and the negative log-likelihood on the device:
ttx_sq_lognorm_grad, ttx_sq_nll_batch, their _dev forms and TTCross.fit_density (ttcross_amd/csrc/ttx_sq_norm.h).

The checker is tests/sq_norm_ref.py: lognorm_grad restates the definition of include/ttx.h in numpy, and exact mode must equal it bit
for bit -- z_mant, z_exp and every G_k, with and without a G0.  MFMA mode runs the same chains and another order in the assembly; its
allowance is mfma_bound, derived there.  logz and nll go through log and are held to logz_allowance and nll_allowance.  The identities
(Euler, the block identity with the right side by mode_apply and dot, the sampler's logq, the scale invariance of the likelihood) are
checked on the device's own numbers.  Each case's references are computed once."""
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
import sample_sq_real_ref as QR
import sample_sq_ref as SQ
import sq_norm_ref as S
import tt_ref as R
from test_gpu_basis_core_grad import SHAPES as CG_SHAPES
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
U = S.U
SHAPES = dict(CG_SHAPES)
SHAPES["ragged17"] = ([17, 17, 17, 17], [1, 5, 33, 2, 1])                 # every mode diagonal: mo = NULL
MODES = ("exact", "mfma")
KINDS = ("mass", "diag")
NAMES = sorted(SHAPES) + ["long255"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _eqs(ga, gb):
    return len(ga) == len(gb) and all(_eq(a, b) for a, b in zip(ga, gb))


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """cores, the engine, md and mo, a G0: computed once, never changed"""
    if name == "long255":
        cores, _, w = SQ.long_case()
        n = [c.shape[1] for c in cores]
        rng = np.random.default_rng(2550)
        if kind == "mass":
            md, mo = [q.copy() for q in w], [0.1 * np.minimum(q[:-1], q[1:]) for q in w]
        else:
            md, mo = [q.copy() for q in w], None
    else:
        n, r = SHAPES[name]
        rng = np.random.default_rng(sum(map(ord, name)) + 31)
        cores = R.rand_train(sum(map(ord, name)), n, r)
        if kind == "mass" and name != "ragged17":
            md, mo = E.mass_tridiag([np.cumsum(rng.uniform(0.2, 1.0, nk)) for nk in n])
            if len(n) > 2:
                mo[2] = None                                                    # one diagonal mode among the tridiagonal ones
        else:
            md, mo = [rng.uniform(0.5, 1.5, nk) for nk in n], None
    g0 = [rng.standard_normal(c.shape) for c in cores]
    return dict(n=n, d=len(n), cores=cores, md=md, mo=mo, g0=g0, tt=E.TTCross.from_cores(cores))


@functools.lru_cache(maxsize=None)
def _chains(name, kind):
    cs = _case(name, kind)
    return S.chains(cs["cores"], cs["md"], cs["mo"])


ARGS = ((0.0, 1.0), (0.37, -1.7))                                              # (gvol, coef)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_exact_is_the_numpy_restatement_bit_for_bit(name, kind):
    cs, ch = _case(name, kind), _chains(name, kind)
    tt = cs["tt"]
    for gvol, coef in ARGS:
        zm, ze, lz, G = S.lognorm_grad(cs["cores"], cs["md"], cs["mo"], gvol, coef, ch=ch)
        res = tt.sq_lognorm_grad(cs["md"], cs["mo"], gvol, coef, mode="exact")
        assert _bits(res["z_mant"]) == _bits(zm) and res["z_exp"] == ze, (res["z_mant"], zm, res["z_exp"], ze)
        assert abs(res["logz"] - lz) <= S.logz_allowance(zm, ze, gvol)
        assert _eqs(res["g"], G) and [g.shape for g in res["g"]] == [u.shape for u in cs["cores"]]
        assert tt.sq_lognorm_grad_last()["mode"] == "exact"
        # onto a G0: the same sum continued
        _, _, _, G1 = S.lognorm_grad(cs["cores"], cs["md"], cs["mo"], gvol, coef, cs["g0"], ch=ch)
        acc = tt.sq_lognorm_grad(cs["md"], cs["mo"], gvol, coef, out=[g.copy() for g in cs["g0"]], accumulate=True, mode="exact")
        assert _eqs(acc["g"], G1)
    if name == "long255":
        assert abs(ze) > 1100 and np.isfinite(res["logz"]) and all(np.isfinite(g).all() for g in res["g"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_mfma_is_within_the_derived_allowance_and_repeats(name, kind):
    cs, ch = _case(name, kind), _chains(name, kind)
    tt = cs["tt"]
    for gvol, coef in ARGS:
        for g0 in (None, cs["g0"]):
            zm, ze, lz, G = S.lognorm_grad(cs["cores"], cs["md"], cs["mo"], gvol, coef, g0, ch=ch)
            bnd = S.mfma_bound(cs["cores"], cs["md"], cs["mo"], gvol, coef, g0, ch=ch)
            kw = {} if g0 is None else dict(out=[g.copy() for g in g0], accumulate=True)
            res = tt.sq_lognorm_grad(cs["md"], cs["mo"], gvol, coef, mode="mfma", **kw)
            assert _bits(res["z_mant"]) == _bits(zm) and res["z_exp"] == ze       # the chains are the same kernels
            for k in range(cs["d"]):
                err = np.abs(res["g"][k] - G[k])
                with np.errstate(invalid="ignore", divide="ignore"):
                    print(name, kind, "core", k + 1, "max err / allowance", float(np.nanmax(np.where(bnd[k] > 0, err / bnd[k], 0.0))))
                assert np.all(err <= bnd[k]), (gvol, g0 is None, k)
            kw = {} if g0 is None else dict(out=[g.copy() for g in g0], accumulate=True)
            again = tt.sq_lognorm_grad(cs["md"], cs["mo"], gvol, coef, mode="mfma", **kw)
            assert _eqs(again["g"], res["g"]) and _bits(again["logz"]) == _bits(res["logz"])
    last = tt.sq_lognorm_grad_last()
    assert last["mode"] == "mfma" and last["ms_asm"] > 0.0 and last["ms_left"] > 0.0 and last["flops"] > 0.0


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_eulers_identity_on_the_devices_own_numbers(name):
    """<G_k, U_k> = 2 for coef = 1, gvol = 0: the allowance of test_sq_norm_cpu.py (the dot product and half of bound())"""
    cs = _case(name, "mass")
    bnd = S.bound(cs["cores"], cs["md"], cs["mo"])
    for mode in MODES:
        G = cs["tt"].sq_lognorm_grad(cs["md"], cs["mo"], mode=mode)["g"]
        for k, (g, u) in enumerate(zip(G, cs["cores"])):
            allow = 2.0 * (g.size + 1) * U * float(np.sum(np.abs(g) * np.abs(u))) + float(np.sum(bnd[k] * np.abs(u)))
            assert abs(float(np.sum(g * u)) - 2.0) <= allow, (mode, k)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["mixed", "ragged", "d2", "two_rows_mr5"])
def test_block_identity_against_mode_apply_and_dot(name, kind):
    """<dZ/dU_k, E> = 2 <T, T_(U_k <- E)>_M with the right side by existing operations: mode_apply with M then dot, or wdot for
    diagonal weights.  Their own error: a term passes, per mode, the matrix (a sum of n_m terms, n_m + 1) and a contraction over
    (a, a', i) in some order (at most r_(m-1)^2 n_m + 2): N_dot u times the contraction on absolute values, twice."""
    cs = _case(name, kind)
    tt, cores, md, mo = cs["tt"], cs["cores"], cs["md"], cs["mo"]
    rng = np.random.default_rng(71)
    res = tt.sq_lognorm_grad(md, mo, mode="exact")
    Z = float(np.ldexp(res["z_mant"], res["z_exp"]))
    bnd = S.bound(cores, md, mo)
    ndot = sum(c.shape[0] ** 2 * c.shape[1] + c.shape[1] + 3 for c in cores)
    absm = ([np.abs(c) for c in cores], [np.abs(m) for m in md], None if mo is None else [None if m is None else np.abs(m) for m in mo])
    small = max(c.shape[2] for c in cores) ** 2 <= 128                          # wdot goes through a Hadamard product: its ranks multiply
    MT = None if kind == "diag" and small else tt.mode_apply([S.tridiag_dense(md[k], None if mo is None else mo[k]) for k in range(cs["d"])], "exact")
    try:
        for k in range(cs["d"]):
            E_ = rng.standard_normal(cores[k].shape)
            te = E.TTCross.from_cores(cores[:k] + [E_] + cores[k + 1:])
            try:
                right = 2.0 * (te.wdot(tt, md) if MT is None else te.dot(MT)) / Z
            finally:
                te.close()
            left = float(np.sum(res["g"][k] * E_))
            rabs = float(2 * S.dense_longdouble(absm[0], absm[1], absm[2], sub=(k, np.abs(E_)))) / abs(Z)
            allow = 2.0 * (E_.size + 1) * U * float(np.sum(np.abs(res["g"][k]) * np.abs(E_))) + float(np.sum(bnd[k] * np.abs(E_))) + 2.0 * (ndot + 4) * U * rabs
            assert abs(left - right) <= allow, (k, abs(left - right) / allow)
            assert abs(left - right) <= 1e-9 * max(abs(left), rabs)
    finally:
        if MT is not None:
            MT.close()


def test_logq_of_the_sampler_plus_logz_is_the_log_of_the_density():
    """for x, logq, val of sample_sq_real on the same nodes and gamma: logq + logz = log(val^2 + gamma), within the sampler's own
    logq_bound (sample_sq_real_ref.verify) plus what Z carries (rel_s u against the true Z, logz_allowance for the log)"""
    cores, u, _ = SQ.edge_case()
    n = SQ.EDGE_RANKS[0]
    rng = np.random.default_rng(4517)
    nodes = [np.cumsum(rng.uniform(0.2, 1.0, nk)) - rng.uniform(0.0, 3.0) for nk in n]
    tt = E.TTCross.from_cores(cores)
    md, mo = E.mass_tridiag(nodes)
    vol = float(np.prod([t[-1] - t[0] for t in nodes if t.size > 1]))       # a mode of one node is held: it has no extent
    for gamma in (0.0, 0.25):
        smp = tt.sample_sq_real(u, nodes, gamma=gamma, mode="exact")
        chk = QR.verify(cores, nodes, u, None, gamma, smp["x"], smp["cell"])
        res = tt.sq_lognorm_grad(md, mo, gvol=gamma * vol, mode="exact")
        allow = chk["logq_bound"] + 8.0 * chk["N"] * U + S.logz_allowance(res["z_mant"], res["z_exp"], gamma * vol) + S.rel_s(cores, md, mo, gamma * vol) * U
        want = np.log(smp["val"] * smp["val"] + gamma)
        assert np.all(np.abs(smp["logq"] + res["logz"] - want) <= 2.0 * allow + 4.0 * U * np.abs(want))


@functools.lru_cache(maxsize=None)
def _nll_case(name):
    n, r = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 77)
    cores = R.rand_train(sum(map(ord, name)) + 1, n, r)
    nodes = [np.cumsum(rng.uniform(0.2, 1.0, nk)) for nk in n]
    x = np.stack([rng.uniform(t[0], t[-1], 33) if t.size > 1 else np.full(33, t[0]) for t in nodes], axis=1)
    md, mo = E.mass_tridiag(nodes)
    vol = float(np.prod([t[-1] - t[0] for t in nodes if t.size > 1]))
    return dict(cores=cores, nodes=nodes, x=np.ascontiguousarray(x), w=rng.uniform(0.5, 1.5, 33), md=md, mo=mo, vol=vol, tt=E.TTCross.from_cores(cores),
                basis=[("linear", t) for t in nodes])


@pytest.mark.parametrize("name", ["mixed", "ragged", "d2", "two_rows_mr5"])
def test_nll_val_c_and_gradient_follow_the_definition(name):
    cs = _nll_case(name)
    tt, x, w, basis = cs["tt"], cs["x"], cs["w"], cs["basis"]
    gamma, gvol = 0.05, 0.05 * cs["vol"]
    ref = S.nll_numpy(cs["cores"], x, cs["nodes"], w, gamma, cs["md"], cs["mo"], gvol)
    for ww, rr in ((w, ref), (None, S.nll_numpy(cs["cores"], x, cs["nodes"], None, gamma, cs["md"], cs["mo"], gvol))):
        res = tt.sq_nll(x, basis, gamma, cs["md"], cs["mo"], gvol, ww, "exact")
        assert _eq(res["val"], tt.basis_batch(x, basis, "exact")) and _eq(res["val"], rr["val"])
        # G through the public calls: basis_core_grad(c) followed by sq_lognorm_grad(coef = W, accumulate)
        _, G = tt.basis_core_grad(x, basis, rr["c"], "exact")
        G = tt.sq_lognorm_grad(cs["md"], cs["mo"], gvol, rr["wsum"], out=G, accumulate=True, mode="exact")["g"]
        assert _eqs(res["g"], G) and _eqs(res["g"], rr["g"])
        allow = S.nll_allowance(rr["lt"], rr["wv"], rr["z_mant"], rr["z_exp"], gvol)
        print(name, "nll", res["nll"], "ref", rr["nll"], "allowance", allow)
        assert abs(res["nll"] - rr["nll"]) <= allow and abs(res["logz"] - rr["logz"]) <= S.logz_allowance(rr["z_mant"], rr["z_exp"], gvol)
    for mode in MODES:                                                          # val is basis_batch's in the mode asked for
        assert _eq(tt.sq_nll(x, basis, gamma, cs["md"], cs["mo"], gvol, w, mode)["val"], tt.basis_batch(x, basis, mode))


@pytest.mark.parametrize("name", ["mixed", "ragged", "d2"])
def test_scale_invariance_of_the_likelihood_at_gamma_zero(name):
    """q does not change when a core is scaled, so <G_k, U_k> = 0 for every k at gamma = 0: the data term gives -2 W, the normaliser
    +2 W.  Allowance: the data term's G carries basis_core_grad_ref.bound (half: one evaluation), the normaliser's half of bound()
    with coef = W; the dot product (size_k + 1) u sum |G_k| |U_k| on the two terms' absolute sums; twice the first-order sum."""
    cs = _nll_case(name)
    tt, x, w, basis = cs["tt"], cs["x"], cs["w"], cs["basis"]
    ref = S.nll_numpy(cs["cores"], x, cs["nodes"], w, 0.0, cs["md"], cs["mo"], 0.0)
    phis = [B.linear_table(cs["nodes"][k], x[:, k]) for k in range(len(cs["cores"]))]
    bdata = C.bound(cs["cores"], phis, ref["c"])
    gdata = C.abs_core_grad(cs["cores"], phis, ref["c"])
    bnorm = S.bound(cs["cores"], cs["md"], cs["mo"], 0.0, ref["wsum"])
    _, _, _, gnorm = S.lognorm_grad(cs["cores"], cs["md"], cs["mo"], 0.0, ref["wsum"])
    for mode in MODES:
        res = tt.sq_nll(x, basis, 0.0, cs["md"], cs["mo"], 0.0, w, mode)
        for k, (g, u) in enumerate(zip(res["g"], cs["cores"])):
            au = np.abs(u)
            allow = float(np.sum((bdata[k] + bnorm[k]) * au)) + 2.0 * (g.size + 2) * U * float(np.sum((gdata[k] + np.abs(gnorm[k])) * au))
            val = float(np.sum(g * u))
            print(name, mode, "core", k + 1, "<G, U>", val, "allowance", allow, "2 W", 2.0 * ref["wsum"])
            assert abs(val) <= allow, (mode, k)
            assert allow < 1e-6 * ref["wsum"]


def test_a_nan_core_gives_nan_and_no_fault():
    """in a child process: whatever a NaN does to a kernel, it does not take this process with it"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "sq_norm_nan_worker.py")], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert res[mode] == dict(clean_finite=True, z_nan=True, g_all_nan=True, nll_nan=True, clean_again_equal=True), (mode, res[mode])


def test_empty_calls_refusals_and_figures():
    L = E.load_library()
    cs = _case("mixed", "mass")
    tt, n, md, mo = cs["tt"], cs["n"], cs["md"], cs["mo"]
    EINVAL, ESTATE = 1, 4
    total = int(tt.core_offsets()[-1])
    # refusals: g untouched
    dp, op, keep = tt._tridiag_rows("t", md, mo)
    g = np.full(total, 7.0)
    zm, ze, lz = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double()
    tail = (ctypes.byref(zm), ctypes.byref(ze), ctypes.byref(lz))

    def refused(rc, word):
        return rc == EINVAL and "ttx_sq_lognorm_grad" in L.ttx_last_error().decode() and word in L.ttx_last_error().decode() and np.all(g == 7.0)

    assert L.ttx_sq_lognorm_grad(tt._h, dp, op, 0.0, 1.0, E._dp(g), 0, 0, *tail) == 0 and not np.all(g == 7.0)
    g[:] = 7.0
    assert refused(L.ttx_sq_lognorm_grad(tt._h, None, op, 0.0, 1.0, E._dp(g), 0, 0, *tail), "md")
    assert L.ttx_sq_lognorm_grad(tt._h, dp, op, 0.0, 1.0, None, 0, 0, *tail) == EINVAL
    assert L.ttx_sq_lognorm_grad_dev(tt._h, dp, op, 0.0, 1.0, None, 0, 0, *tail) == EINVAL and "ttx_sq_lognorm_grad_dev:" in L.ttx_last_error().decode()
    for gv in (-1.0, float("inf"), float("nan")):
        assert refused(L.ttx_sq_lognorm_grad(tt._h, dp, op, gv, 1.0, E._dp(g), 0, 0, *tail), "gvol")
    for cf in (float("inf"), float("nan")):
        assert refused(L.ttx_sq_lognorm_grad(tt._h, dp, op, 0.0, cf, E._dp(g), 0, 0, *tail), "coef")
    for acc in (2, -1):
        assert refused(L.ttx_sq_lognorm_grad(tt._h, dp, op, 0.0, 1.0, E._dp(g), acc, 0, *tail), "accumulate")
    assert refused(L.ttx_sq_lognorm_grad(tt._h, dp, op, 0.0, 1.0, E._dp(g), 0, 3, *tail), "mode")
    dp2, _, keep2 = tt._tridiag_rows("t", md, mo)
    dp2[1] = ctypes.POINTER(ctypes.c_double)()
    assert refused(L.ttx_sq_lognorm_grad(tt._h, dp2, op, 0.0, 1.0, E._dp(g), 0, 0, *tail), "md[1]")
    for bad in (float("nan"), float("inf")):
        mdb = [m.copy() for m in md]
        mdb[2][50] = bad
        dpb, opb, keepb = tt._tridiag_rows("t", mdb, mo)
        assert refused(L.ttx_sq_lognorm_grad(tt._h, dpb, opb, 0.0, 1.0, E._dp(g), 0, 0, *tail), "md[2][50]")
        mob = [None if m is None else m.copy() for m in mo]
        mob[4][7] = bad
        dpb, opb, keepb = tt._tridiag_rows("t", md, mob)
        assert refused(L.ttx_sq_lognorm_grad(tt._h, dpb, opb, 0.0, 1.0, E._dp(g), 0, 0, *tail), "mo[4][7]")
    # z_mant, z_exp and logz may be null; a null mo is a diagonal matrix
    assert L.ttx_sq_lognorm_grad(tt._h, dp, None, 0.0, 1.0, E._dp(g), 0, 0, None, None, None) == 0
    assert _eq(g, S.pack(S.lognorm_grad(cs["cores"], md, None)[3]))
    g[:] = 7.0
    # an engine without a train: TTX_ESTATE.  (Ranks above 128 and boundary ranks other than 1: no engine can hold such a train, the
    # plan's refusals are walked by tests/sq_norm_plan_main.cpp; a multi-process engine is refused by the shared preflight)
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    assert L.ttx_sq_lognorm_grad(fresh._h, dp, op, 0.0, 1.0, E._dp(g), 0, 0, *tail) == ESTATE and np.all(g == 7.0)
    with pytest.raises(E.TTXError, match="1..128"):
        E.TTCross.from_cores([np.ones((1, 2, 129)), np.ones((129, 2, 1))])
    with pytest.raises(ValueError):
        tt.sq_lognorm_grad(md[:-1], None)
    with pytest.raises(ValueError):
        tt.sq_lognorm_grad(md, mo, accumulate=True)
    # ttx_sq_nll_batch: refusals, npts = 0
    nodes = [np.linspace(0.0, 1.0, nk) if nk > 1 else np.array([0.5]) for nk in n]
    basis = [("linear", t) for t in nodes]
    arr, keepa = tt._basis_arr("t", basis)
    x, w = np.full((4, 5), 0.5), np.ones(4)
    nll, val = ctypes.c_double(), np.zeros(4)

    def nll_call(xx=x, ww=w, gamma=0.1, gvol=0.1, mode=0, basis_=arr, npts=4, dd=dp):
        return L.ttx_sq_nll_batch(tt._h, npts, E._dp(xx), basis_, E._dp(ww), gamma, dd, op, gvol, mode, ctypes.byref(nll), ctypes.byref(lz), E._dp(val), E._dp(g))

    assert nll_call() == 0 and not np.all(g == 7.0) and np.isfinite(nll.value)
    g[:] = 7.0
    for kw in (dict(gamma=-1.0), dict(gamma=float("nan")), dict(gvol=-1.0), dict(mode=5), dict(ww=np.array([1.0, -1.0, 1.0, 1.0])), dict(ww=np.array([1.0, np.inf, 1.0, 1.0])),
               dict(basis_=None), dict(npts=-1), dict(dd=None), dict(xx=None)):
        assert nll_call(**kw) == EINVAL and "ttx_sq_nll_batch:" in L.ttx_last_error().decode() and np.all(g == 7.0), kw
    assert L.ttx_sq_nll_batch(tt._h, 4, E._dp(x), arr, E._dp(w), 0.1, dp, op, 0.1, 0, None, None, None, E._dp(g)) == EINVAL
    assert L.ttx_sq_nll_batch(fresh._h, 4, E._dp(x), arr, E._dp(w), 0.1, dp, op, 0.1, 0, ctypes.byref(nll), None, None, E._dp(g)) == ESTATE and np.all(g == 7.0)
    e0 = tt.sq_nll(np.zeros((0, 5)), basis, 0.1, md, mo, 0.1)
    assert e0["nll"] == 0.0 and e0["val"].shape == (0,) and all(not b.any() for b in e0["g"])
    assert abs(e0["logz"] - tt.sq_lognorm_grad(md, mo, 0.1)["logz"]) == 0.0
    # a point without mass at gamma = 0: nll = +inf and G NaN, by the arithmetic
    zero = E.TTCross.from_cores([np.zeros_like(cs["cores"][0])] + cs["cores"][1:])
    rz = zero.sq_nll(x, basis, 0.0, md, mo, 1.0)
    assert rz["nll"] == np.inf and all(np.isnan(b).all() for b in rz["g"])
    # the figures; auto is one of the two modes
    res = {m: tt.sq_lognorm_grad(md, mo, 0.3, mode=m) for m in MODES}
    for m in MODES:
        tt.sq_lognorm_grad(md, mo, 0.3, mode=m)
        last = tt.sq_lognorm_grad_last()
        r = tt.ranks()
        assert last["mode"] == m and last["flops"] == sum(4.0 * r[k] ** 2 * n[k] * r[k + 1] + 6.0 * r[k] * n[k] * r[k + 1] ** 2 for k in range(5))
        assert last["ms_right"] > 0.0 and last["ms_left"] > 0.0 and last["ms_asm"] > 0.0
    auto = tt.sq_lognorm_grad(md, mo, 0.3, mode="auto")
    ran = tt.sq_lognorm_grad_last()["mode"]
    assert ran in MODES and _eqs(auto["g"], res[ran]["g"])
    for k, core in enumerate(cs["cores"]):                                      # the train is untouched
        assert _eq(tt.core(k + 1), core), k


def _worker(what):
    p = subprocess.run([sys.executable, os.path.join(HERE, "sq_norm_dev_worker.py"), what], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_device_pointer_entries_equal_the_host_pointer_entries():
    """in a child process: torch has to initialise its device before the engine's library does"""
    res = _worker("dev")
    for mode in MODES:
        assert res[mode] == dict(lognorm_equal=True, accumulated_equal=True, nll_is_cuda=True, nll_into_out=True, nll_equal=True, nll_unweighted_equal=True), (mode, res[mode])
    assert res["float32_refused"] and res["host_w_refused"] and res["short_out_refused"]


def test_fit_density_follows_the_numpy_restatement():
    """EXACT mode: the same accept / reject sequence, every trial's nll within the derived allowance (the pinned problem keeps every
    Armijo margin above twice that: test_sq_norm_cpu.py asserts it on the reference alone), the held-out nll ends below the start's.
    MFMA mode: the nll falls at every accepted step.  In a child process, as fit_density works on torch tensors."""
    want = S.fit_density_numpy()
    res = _worker("fit")
    got = res["exact"]
    assert [h[1] for h in got["hist"]] == [h[1] for h in want["hist"]] and got["iters"] == want["iters"]
    for (fn, _, _), (rn, _, _), allow in zip(got["hist"], want["hist"], want["allow"]):
        print("trial nll", fn, "ref", rn, "allowance", allow)
        assert abs(fn - rn) <= allow
    for mode in MODES:
        g = res[mode]
        assert g["iters"] >= 1 and all(b < a for a, b in zip(g["nll"], g["nll"][1:])) and g["held_after"] < g["held_before"], (mode, g)
