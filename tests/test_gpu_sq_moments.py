"""Moments and reduced density matrices of the squared density on the device: ttx_sq_moments, TTCross.sq_moments, density_moments and
sq_marginal_pdf (ttcross_amd/csrc/ttx_sq_moments.h).

The checker is tests/sq_moments_ref.py: moments() restates the definition of include/ttx.h in numpy, and exact mode must equal it bit for
bit -- z_mant, z_exp, bd, bo, m1 and c2, with all modes selected and with a subset.  MFMA mode evaluates the carried steps in another
order; its allowance is bound(), derived there, and everything that does not pass a carried step is EXACT's bits.  The batch cuts change
no bit.  The identities are checked on the device's own numbers, the moments of q against a seeded sample of sample_sq_real.  The shapes
and matrices are those of test_gpu_sq_norm.py; each case's references are computed once."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sq_moments_ref as M
import sq_norm_ref as S
from test_gpu_sq_norm import KINDS, NAMES, _case
from test_sq_moments_cpu import SAMPLER_SEED, exact_density_moments
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
U = S.U
MODES = ("exact", "mfma")
LONG_SEL = [0, 7, 8, 127, 253, 254]                                             # the first, two adjacent, the middle, the last two
KEYS = ("m1", "c2")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _same(ra, rb, band=True):
    ok = _bits(ra["z_mant"]) == _bits(rb["z_mant"]) and ra["z_exp"] == rb["z_exp"] and _eq(ra["m1"], rb["m1"]) and _eq(ra["c2"], rb["c2"])
    if band:
        ok = ok and all(_eq(a, b) for a, b in zip(ra["bd"] + ra["bo"], rb["bd"] + rb["bo"])) and len(ra["bd"]) == len(rb["bd"])
    return bool(ok)


@functools.lru_cache(maxsize=None)
def _obs(name, kind):
    """the observables of a case: A_k and A2_k, signed, tridiagonal where M_k is; the selection (all modes, six of long255)"""
    cs = _case(name, kind)
    d, n = cs["d"], cs["n"]
    rng = np.random.default_rng(sum(map(ord, name)) + 97)
    tri = [cs["mo"] is not None and cs["mo"][k] is not None for k in range(d)]
    ad, a2d = [rng.uniform(-1.0, 1.0, n[k]) for k in range(d)], [rng.uniform(0.0, 1.0, n[k]) for k in range(d)]
    ao = [rng.uniform(-0.3, 0.3, max(n[k] - 1, 0)) if tri[k] else None for k in range(d)]
    a2o = [rng.uniform(0.0, 0.3, max(n[k] - 1, 0)) if tri[k] else None for k in range(d)]
    sel = LONG_SEL if name == "long255" else list(range(d))
    if name == "long255":
        ad = [a if k in sel else None for k, a in enumerate(ad)]
    sub = list(ad)
    for k in (sel[1::2] if len(sel) > 2 else sel[:1]):                          # the subset: every other selected mode left out
        sub[k] = None
    return dict(ad=ad, ao=ao, a2d=a2d, a2o=a2o, sub=sub, sel=sel)


@functools.lru_cache(maxsize=None)
def _ref(name, kind, which):
    cs, ob = _case(name, kind), _obs(name, kind)
    return M.moments(cs["cores"], cs["md"], cs["mo"], ob[which], ob["ao"], ob["a2d"], ob["a2o"])


@functools.lru_cache(maxsize=None)
def _bound(name, kind):
    cs, ob = _case(name, kind), _obs(name, kind)
    return M.bound(cs["cores"], cs["md"], cs["mo"], ob["ad"], ob["ao"], ob["a2d"], ob["a2o"], got=_ref(name, kind, "ad"))


def _call(name, kind, which, mode, **kw):
    cs, ob = _case(name, kind), _obs(name, kind)
    return cs["tt"].sq_moments(cs["md"], cs["mo"], ob[which], ob["ao"], ob["a2d"], ob["a2o"], mode=mode, **kw)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_exact_is_the_numpy_restatement_bit_for_bit(name, kind):
    cs = _case(name, kind)
    tt = cs["tt"]
    zn = tt.sq_lognorm_grad(cs["md"], cs["mo"], mode="exact")
    for which in ("ad", "sub"):
        want, got = _ref(name, kind, which), _call(name, kind, which, "exact")
        assert _bits(got["z_mant"]) == _bits(zn["z_mant"]) and got["z_exp"] == zn["z_exp"]
        for key in KEYS:
            assert _eq(got[key], want[key]), (which, key, got[key], want[key])
        assert _same(got, want)
        last = tt.sq_moments_last()
        sel = [k for k, a in enumerate(_obs(name, kind)[which]) if a is not None]
        assert last["mode"] == "exact" and last["steps"] == M.steps_of(sel) and last["ms_chains"] > 0.0 and last["ms_band"] > 0.0
    if name == "long255":
        assert abs(got["z_exp"]) > 1100 and np.isfinite(got["c2"]).all() and np.isfinite(got["m1"]).all() and all(np.isfinite(v).all() for v in got["bd"])
        assert np.count_nonzero(_call(name, kind, "ad", "exact")["c2"]) == 36
    # without the band, without moments: the rest is the same bits
    nb = _call(name, kind, "ad", "exact", band=False)
    assert nb["bd"] is None and _same(nb, _ref(name, kind, "ad"), band=False)
    zb = tt.sq_moments(cs["md"], cs["mo"], mode="exact")
    assert zb["m1"] is None and all(_eq(a, b) for a, b in zip(zb["bd"] + zb["bo"], _ref(name, kind, "ad")["bd"] + _ref(name, kind, "ad")["bo"]))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", NAMES)
def test_mfma_is_within_the_derived_allowance_and_repeats(name, kind):
    want, bnd = _ref(name, kind, "ad"), _bound(name, kind)
    got = _call(name, kind, "ad", "mfma")
    assert _case(name, kind)["tt"].sq_moments_last()["mode"] == "mfma"
    assert _bits(got["z_mant"]) == _bits(want["z_mant"]) and got["z_exp"] == want["z_exp"]         # the chains are the same kernels
    err = np.abs(got["c2"] - want["c2"])
    with np.errstate(invalid="ignore", divide="ignore"):
        print(name, kind, "c2 max err / allowance", float(np.nanmax(np.where(bnd["c2"] > 0, err / bnd["c2"], 0.0))), "C", bnd["C"], "rho", bnd["rho"])
    assert np.all(err <= bnd["c2"])
    assert np.array_equal(got["c2"], got["c2"].T)
    # what passes no carried step is EXACT's bits: m1, the diagonal of c2, the band
    assert _eq(got["m1"], want["m1"]) and _eq(np.diag(got["c2"]), np.diag(want["c2"]))
    assert all(_eq(a, b) for a, b in zip(got["bd"] + got["bo"], want["bd"] + want["bo"]))
    assert _same(_call(name, kind, "ad", "mfma"), got)
    if name == "long255":
        assert np.isfinite(got["c2"]).all()


@pytest.mark.parametrize("name", ["mixed", "two_rows_mr5", "long255"])
def test_batch_cuts_change_no_bit(name, monkeypatch):
    for mode in MODES:
        monkeypatch.delenv("TTX_SQM_BATCH", raising=False)
        base = _call(name, "mass", "ad", mode)
        for b in ("1", "3"):
            monkeypatch.setenv("TTX_SQM_BATCH", b)
            assert _same(_call(name, "mass", "ad", mode), base), (mode, b)
    monkeypatch.delenv("TTX_SQM_BATCH", raising=False)
    assert _same(base, _call(name, "mass", "ad", "mfma"))


@pytest.mark.parametrize("name", ["mixed", "ragged", "d2", "two_rows_mr5"])
def test_identities_on_the_devices_own_numbers(name):
    cs, ob, bnd = _case(name, "mass"), _obs(name, "mass"), _bound(name, "mass")
    tt, md, mo, d = cs["tt"], cs["md"], cs["mo"], cs["d"]
    off = ~np.eye(d, dtype=bool)
    for mode in MODES:
        got = _call(name, "mass", "ad", mode)
        for k in range(d):
            one, a1 = M.band_trace(got["bd"][k], got["bo"][k], bnd["bd"][k], bnd["bo"][k], md[k], None if mo is None else mo[k])
            assert abs(one - 1.0) <= a1, (mode, k, one)
            m, a2 = M.band_trace(got["bd"][k], got["bo"][k], bnd["bd"][k], bnd["bo"][k], ob["ad"][k], ob["ao"][k])
            assert abs(m - got["m1"][k]) <= a2 + bnd["m1"][k], (mode, k)
        # A_l = M_l for l > 1: c2[1][l] = m1[1]; A_k = M_k everywhere: every c2[k][l] = 1 and every m1 = 1
        mix = ([ob["ad"][0]] + list(md[1:]), [ob["ao"][0]] + [None if mo is None else mo[k] for k in range(1, d)])
        g2 = tt.sq_moments(md, mo, mix[0], mix[1], mode=mode, band=False)
        b2 = M.bound(cs["cores"], md, mo, mix[0], mix[1], band=False)
        for l in range(1, d):
            assert abs(g2["c2"][0, l] - got["m1"][0]) <= b2["c2"][0, l] + bnd["m1"][0], (mode, l)
        g3 = tt.sq_moments(md, mo, md, mo, mode=mode, band=False)
        b3 = M.bound(cs["cores"], md, mo, md, mo, band=False)
        assert np.all(np.abs(g3["c2"] - 1.0)[off] <= b3["c2"][off]) and np.all(np.abs(g3["m1"] - 1.0) <= b3["m1"]), mode
        assert np.array_equal(g3["c2"], g3["c2"].T) and not np.diag(g3["c2"]).any()


def test_density_moments_against_the_sampler_and_the_marginal_integrates_to_one():
    prob = S.fit_problem()
    tt = E.TTCross.from_cores(prob["cores"])
    nodes, gamma = prob["nodes"], prob["gamma"]
    assert gamma > 0.0
    mean, cov, alpha = exact_density_moments(prob)
    u = np.random.default_rng(SAMPLER_SEED).random((100000, 3))
    x = tt.sample_sq_real(u, nodes, gamma=gamma, mode="exact", want=("x",))["x"]
    assert not np.isnan(x).any()
    for mode in MODES:
        dm = tt.density_moments(nodes, gamma=gamma, mode=mode)
        zn = tt.sq_lognorm_grad(prob["md"], prob["mo"], gvol=prob["gvol"], mode="exact")
        assert dm["modes"] == [0, 1, 2] and abs(dm["alpha"] - alpha) <= 8 * U
        assert abs(dm["logz"] - zn["logz"]) <= 2.0 * S.logz_allowance(zn["z_mant"], zn["z_exp"], prob["gvol"])
        okm, okc, rm, rc = M.sample_check(x, dm["mean"], dm["cov"])
        print(mode, "worst mean ratio", rm, "worst cov ratio", rc)
        assert okm and okc, (mode, rm, rc)
    sub = tt.density_moments(nodes, gamma=gamma, select=[2, 0], mode="exact")
    full = tt.density_moments(nodes, gamma=gamma, mode="exact")
    assert sub["modes"] == [0, 2] and np.array_equal(sub["mean"], full["mean"][[0, 2]]) and np.array_equal(sub["cov"], full["cov"][np.ix_([0, 2], [0, 2])])
    # the marginal: a quadratic on every cell.  With m equal parts per cell the trapezoid rule's error on a cell of width h is
    # h^3 / (12 m^2) |p''|, p'' = 2 alpha (bd_c - 2 bo_c + bd_(c+1)) / h^2; the exact integral is the mass identity, within its allowance
    res = tt.sq_moments(prob["md"], prob["mo"], mode="exact")
    bnd = M.bound(prob["cores"], prob["md"], prob["mo"])
    m = 64
    for k in range(3):
        t, bd, bo = nodes[k], res["bd"][k], res["bo"][k]
        grid = np.concatenate([t[c] + (t[c + 1] - t[c]) * np.arange(m) / m for c in range(t.size - 1)] + [t[-1:]])
        p = tt.sq_marginal_pdf(k, grid, nodes, gamma=gamma)
        trap = float(np.sum(0.5 * (p[1:] + p[:-1]) * np.diff(grid)))
        h = np.diff(t)
        rule = float(np.sum(h * np.abs(bd[:-1] - 2.0 * bo[:-1] + bd[1:]))) * dm["alpha"] / (6.0 * m * m)
        _, ident = M.band_trace(bd, bo, bnd["bd"][k], bnd["bo"][k], prob["md"][k], prob["mo"][k])
        rounding = 8.0 * (grid.size + 8) * U * float(np.sum(0.5 * (np.abs(p[1:]) + np.abs(p[:-1])) * np.diff(grid)))
        print("mode", k, "trapezoid", trap, "rule bound", rule, "identity allowance", ident)
        assert abs(trap - 1.0) <= rule + ident + rounding and rule < 1e-3
        assert np.all(p > 0.0) and tt.sq_marginal_pdf(k, np.array([t[0] - 1.0, t[-1] + 1.0]), nodes, gamma=gamma).tolist() == [0.0, 0.0]
    tt.close()


def test_a_nan_core_gives_nan_and_no_fault():
    """in a child process: whatever a NaN does to a kernel, it does not take this process with it"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "sq_moments_nan_worker.py")], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert res[mode] == dict(clean_finite=True, z_nan=True, moments_all_nan=True, band_all_nan=True, clean_again_equal=True), (mode, res[mode])


def test_refusals_leave_the_outputs_untouched_and_figures():
    L = E.load_library()
    cs, ob = _case("mixed", "mass"), _obs("mixed", "mass")
    tt, n, md, mo, d = cs["tt"], cs["n"], cs["md"], cs["mo"], cs["d"]
    EINVAL, ESTATE = 1, 4
    dp, op, keep = tt._tridiag_rows("t", md, mo)
    ap, aop, keepa = tt._opt_rows("t", "ad", ob["ad"], ob["ao"])
    a2p, a2op, keepb = tt._opt_rows("t", "a2d", ob["a2d"], ob["a2o"])
    nsum = sum(n)
    bd, bo, m1, c2 = np.full(nsum, 7.0), np.full(nsum, 7.0), np.full(d, 7.0), np.full((d, d), 7.0)
    zm, ze = ctypes.c_double(7.0), ctypes.c_int64(7)

    def call(h=tt._h, dp_=dp, op_=op, ap_=ap, aop_=aop, a2p_=a2p, a2op_=a2op, mode=0, outs=True):
        o = (ctypes.byref(zm), ctypes.byref(ze), E._dp(bd), E._dp(bo), E._dp(m1), E._dp(c2)) if outs else (None,) * 6
        return L.ttx_sq_moments(h, dp_, op_, ap_, aop_, a2p_, a2op_, mode, *o)

    def untouched():
        return zm.value == 7.0 and ze.value == 7 and all(np.all(a == 7.0) for a in (bd, bo, m1, c2))

    def refused(rc, word):
        msg = L.ttx_last_error().decode()
        return rc == EINVAL and "ttx_sq_moments" in msg and word in msg and untouched()

    assert refused(call(dp_=None), "md")
    assert refused(call(mode=3), "mode")
    assert refused(call(outs=False), "output")
    dp2, _, keep2 = tt._tridiag_rows("t", md, mo)
    dp2[1] = ctypes.POINTER(ctypes.c_double)()
    assert refused(call(dp_=dp2), "md[1]")
    for bad in (float("nan"), float("inf")):
        mdb = [m.copy() for m in md]
        mdb[2][50] = bad
        dpb, opb, kb = tt._tridiag_rows("t", mdb, mo)
        assert refused(call(dp_=dpb, op_=opb), "md[2][50]")
        for nd, no, rows, offs, slots in (("ad", "ao", ob["ad"], ob["ao"], ("ap_", "aop_")), ("a2d", "a2o", ob["a2d"], ob["a2o"], ("a2p_", "a2op_"))):
            rb = [a.copy() for a in rows]
            rb[0][3] = bad
            pb, pob, kb2 = tt._opt_rows("t", nd, rb, offs)
            assert refused(call(**{slots[0]: pb, slots[1]: pob}), nd + "[0][3]")
            ofb = [None if a is None else a.copy() for a in offs]
            ofb[4][7] = bad
            pb, pob, kb3 = tt._opt_rows("t", nd, rows, ofb)
            assert refused(call(**{slots[0]: pb, slots[1]: pob}), no + "[4][7]")
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    assert call(h=fresh._h) == ESTATE and untouched()
    # a call that is not refused writes everything; ad NULL fills m1 and c2 with 0.0
    assert call() == 0 and not untouched() and _eq(m1, _ref("mixed", "mass", "ad")["m1"]) and _eq(c2, _ref("mixed", "mass", "ad")["c2"])
    assert call(ap_=None, aop_=None) == 0 and not m1.any() and not c2.any()
    with pytest.raises(ValueError):
        tt.sq_moments(md[:-1])
    with pytest.raises(ValueError):
        tt.sq_moments(md, mo, ob["ad"][:-1])
    # auto is one of the two modes; the environment moves the break-even
    auto = _call("mixed", "mass", "ad", "auto")
    ran = tt.sq_moments_last()
    assert ran["mode"] in MODES and ran["flops"] > 0.0 and _same(auto, _call("mixed", "mass", "ad", ran["mode"]))
    for k, core in enumerate(cs["cores"]):                                      # the train is untouched
        assert _eq(tt.core(k + 1), core), k


def test_auto_follows_the_break_even_of_the_environment(monkeypatch):
    tt = _case("mixed", "mass")["tt"]
    monkeypatch.setenv("TTX_SQM_AUTO_FLOPS", "1")
    _call("mixed", "mass", "ad", "auto")
    assert tt.sq_moments_last()["mode"] == "mfma"
    monkeypatch.setenv("TTX_SQM_AUTO_FLOPS", "1e30")
    _call("mixed", "mass", "ad", "auto")
    assert tt.sq_moments_last()["mode"] == "exact"
