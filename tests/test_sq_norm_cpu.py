"""The normaliser of the squared density and its gradient (ttx_sq_lognorm_grad, ttx_sq_nll_batch, TTCross.fit_density): what can be
checked without a GPU -- the numpy restatement (tests/sq_norm_ref.py) against a dense long-double einsum, Euler's identity and the block
identity on the restatement, accumulation, mass_tridiag against mass_cholesky, the d = 255 train whose unscaled chains overflow, the
L-BFGS restatement on the pinned problem, the plan of a call (tests/sq_norm_plan_main.cpp, plain and under the sanitizers) and the C ABI
as declared and exported."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sample_sq_ref as Q
import sq_norm_ref as S
import tt_ref as R
from ttcross_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ttx_sq_lognorm_grad", "ttx_sq_lognorm_grad_dev", "ttx_sq_lognorm_grad_last", "ttx_sq_nll_batch", "ttx_sq_nll_batch_dev")
SHAPES = [([7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]), ([3, 4, 2, 5], [1, 2, 70, 3, 1]), ([5, 7], [1, 3, 1]), ([5], [1, 1]), ([1, 4, 1], [1, 2, 3, 1])]
U = S.U


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _data(n, r, seed, nonneg):
    """cores, md, mo: signed cores with a mass-like matrix (mode 2 diagonal), or everything without negative entries"""
    rng = np.random.default_rng(seed)
    if nonneg:
        cores = [rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1])) for k in range(len(n))]
    else:
        cores = R.rand_train(seed, n, r)
    md = [rng.uniform(0.5, 1.5, nk) for nk in n]
    mo = [rng.uniform(0.05, 0.25, max(nk - 1, 0)) for nk in n]
    if len(n) > 1:
        mo[1] = None
    return cores, md, mo


@pytest.mark.parametrize("n,r", SHAPES)
def test_restatement_agrees_with_a_dense_long_double_einsum(n, r):
    """The restatement lies within half of bound() of the true values (sq_norm_ref's derivation).  The long-double einsum stands for
    the true value: its own error is the same count at u = 2^-64, below 2^-10 of that half, which the factor 1 + 2^-10 takes in."""
    for nonneg in (False, True):
        for gvol, coef, with_g0 in ((0.0, 1.0, False), (0.37, -1.7, True)):
            cores, md, mo = _data(n, r, 5 + len(n), nonneg)
            rng = np.random.default_rng(3)
            g0 = [rng.standard_normal(c.shape) for c in cores] if with_g0 else None
            zm, ze, lz, G = S.lognorm_grad(cores, md, mo, gvol, coef, g0)
            Z, dZ = S.dense_longdouble(cores, md, mo)
            assert 0.5 <= abs(zm) < 1.0
            nz = sum(S.left_count(c) for c in cores)
            zabs = S.dense_longdouble([np.abs(c) for c in cores], [np.abs(m) for m in md], [None if m is None else np.abs(m) for m in mo])[0]
            assert abs(np.ldexp(np.longdouble(zm), ze) - Z) <= 0.5 * (1.0 + 2.0 ** -10) * 2.0 * nz * U * float(zabs)
            assert abs(lz - float(np.log(Z + np.longdouble(gvol)))) <= S.logz_allowance(zm, ze, gvol) + S.rel_s(cores, md, mo, gvol) * U
            bnd = S.bound(cores, md, mo, gvol, coef, g0)
            for k in range(len(n)):
                true = (np.longdouble(coef) / (Z + np.longdouble(gvol))) * dZ[k] + (0 if g0 is None else g0[k].astype(np.longdouble))
                err = np.abs(G[k].astype(np.longdouble) - true).astype(np.float64)
                assert G[k].shape == cores[k].shape and np.all(err <= 0.5 * (1.0 + 2.0 ** -10) * bnd[k]), (nonneg, k, float(np.max(err / bnd[k])))
            if nonneg and not with_g0:                                          # no cancellation: the bound is relative, a dropped term shows
                for k in range(len(n)):
                    assert np.all(bnd[k] <= 2.0 * U * (sum(S.left_count(c) + S.right_count(c) for c in cores) + 3 * nz + 20) * np.abs(G[k]) * 1.01)


@pytest.mark.parametrize("n,r", SHAPES)
def test_eulers_identity_holds_on_the_restatement(n, r):
    """<dZ/dU_k, U_k> = 2 Z for every k: with coef = 1 and gvol = 0, <G_k, U_k> = 2.  The allowance: the dot product of size_k terms
    carries (size_k + 1) u sum |G_k| |U_k|, G_k carries half of bound(); twice the first-order sum."""
    for nonneg in (False, True):
        cores, md, mo = _data(n, r, 9 + len(n), nonneg)
        _, _, _, G = S.lognorm_grad(cores, md, mo)
        bnd = S.bound(cores, md, mo)
        for k, (g, u) in enumerate(zip(G, cores)):
            allow = 2.0 * (g.size + 1) * U * float(np.sum(np.abs(g) * np.abs(u))) + float(np.sum(bnd[k] * np.abs(u)))
            assert abs(float(np.sum(g * u)) - 2.0) <= allow, (nonneg, k)
            if nonneg:
                assert allow < 1e-9


@pytest.mark.parametrize("n,r", SHAPES)
def test_block_identity_holds_on_the_restatement(n, r):
    """<dZ/dU_k, E> = 2 <T, T_(U_k <- E)>_M for a random block E; the right side by the unscaled long-double chain"""
    rng = np.random.default_rng(33)
    for nonneg in (False, True):
        cores, md, mo = _data(n, r, 17 + len(n), nonneg)
        zm, ze, _, G = S.lognorm_grad(cores, md, mo)
        bnd = S.bound(cores, md, mo)
        Z = np.ldexp(np.longdouble(zm), ze)
        for k in range(len(n)):
            E_ = rng.uniform(0.0, 1.0, cores[k].shape) if nonneg else rng.standard_normal(cores[k].shape)
            left = float(np.sum(G[k] * E_))                                     # <G_k, E> with G_k = dZ/dU_k / Z
            right = float(2 * S.dense_longdouble(cores, md, mo, sub=(k, E_)) / Z)
            allow = 2.0 * (E_.size + 1) * U * float(np.sum(np.abs(G[k]) * np.abs(E_))) + float(np.sum(bnd[k] * np.abs(E_))) + 4.0 * U * abs(right)
            assert abs(left - right) <= allow, (nonneg, k, abs(left - right) / allow)
            if nonneg:
                assert left > 0.0 and abs(left - right) <= 1e-10 * left
                worse = float(np.sum(G[k][:, 1:, :] * E_[:, 1:, :])) if cores[k].shape[1] > 1 else 0.0
                assert abs(worse - right) > allow                              # a dropped index shows


@pytest.mark.parametrize("n,r", SHAPES)
def test_accumulating_onto_g0_continues_the_same_sum(n, r):
    cores, md, mo = _data(n, r, 21, False)
    rng = np.random.default_rng(4)
    g0 = [rng.standard_normal(c.shape) for c in cores]
    ch = S.chains(cores, md, mo)
    _, _, _, G = S.lognorm_grad(cores, md, mo, 0.2, 3.0, g0)
    _, _, _, D = S.lognorm_grad(cores, md, mo, 0.2, 3.0, None, ch)
    for k in range(len(n)):                                                     # D = 0.0 + s D_k is s D_k itself, so G = G0 + D to the bit
        assert np.array_equal(_bits(G[k]), _bits(g0[k] + D[k]))


def test_mass_tridiag_is_the_cholesky_factors_product():
    rng = np.random.default_rng(8)
    for n in (1, 2, 3, 17, 51):
        t = np.cumsum(rng.uniform(0.1, 2.0, n))
        md, mo = E.mass_tridiag(t)
        rd, ro = S.mass_tridiag(t)
        assert np.array_equal(_bits(md), _bits(rd)) and np.array_equal(_bits(mo), _bits(ro)) and mo.shape == (n - 1,)
        dg, sp = E.mass_cholesky(t)
        if n == 1:
            assert md.tolist() == [1.0]
            continue
        # M = U^T U: M[i, i] = dg[i]^2 + sp[i-1]^2, M[i, i+1] = dg[i] sp[i]; three roundings each
        d2 = dg * dg
        d2[1:] += sp[:-1] * sp[:-1]
        assert np.all(np.abs(d2 - md) <= 4 * U * md) and np.all(np.abs(dg[:-1] * sp[:-1] - mo) <= 4 * U * mo)
    mds, mos = E.mass_tridiag([np.array([0.0, 1.0, 3.0]), np.array([2.0]), np.array([0.0, 2.0])], [0.5, None, float("nan")])
    assert mds[0].tolist() == [0.25, 0.25, 0.0] and mos[0].tolist() == [0.25, 0.0] and mds[1].tolist() == [1.0] and mos[1].size == 0
    assert mds[2].tolist() == [2.0 / 3.0, 2.0 / 3.0] and mos[2].tolist() == [2.0 / 6.0]
    with pytest.raises(ValueError):
        E.mass_tridiag([np.array([0.0, 1.0])], [2.0])


def test_long_train_stays_finite_where_unscaled_chains_overflow():
    cores, _, w = Q.long_case()
    ch = S.chains(cores, w, None)
    zm, ze, lz, G = S.lognorm_grad(cores, w, None, ch=ch)
    assert abs(ze) > 1100 and 0.5 <= abs(zm) < 1.0 and np.isfinite(lz) and all(np.isfinite(g).all() for g in G)
    for k, (g, u) in enumerate(zip(G, cores)):                                  # Euler, loosely: the scaling loses nothing
        assert abs(float(np.sum(g * u)) - 2.0) < 1e-9, k
    with np.errstate(over="ignore", invalid="ignore"):                          # the same chain without the powers of two
        p = np.ones((1, 1))
        for c, m in zip(cores, w):
            p = np.einsum("ac,aib,i,cid->bd", p, c, m, c)
    assert not np.isfinite(p).all()


def test_fit_density_numpy_lowers_the_nll_at_every_accepted_step():
    prob = S.fit_problem()
    assert [u.shape for u in prob["cores"]] == [(1, 5, 3), (3, 6, 2), (2, 4, 1)] and prob["x"].shape == (160, 3) and prob["w"].shape == (160,)
    res = S.fit_density_numpy(prob)
    assert res["iters"] >= 4 and np.isfinite(res["nll"]).all()
    assert all(b < a for a, b in zip(res["nll"], res["nll"][1:])), res["nll"]
    assert [h[0] for h in res["hist"] if h[1]] == res["nll"][1:]
    # every Armijo decision is safe: its margin exceeds twice the nll allowance of the trial
    assert len(res["allow"]) == len(res["hist"])
    for (fn, ok, bound), allow in zip(res["hist"], res["allow"]):
        assert abs(bound - fn) > 2.0 * allow, (fn, bound, allow)
    again = S.fit_density_numpy(prob)
    assert again["nll"] == res["nll"] and again["hist"] == res["hist"]           # a fixed list of doubles
    held = lambda cs: S.nll_numpy(cs, prob["xh"], prob["nodes"], None, prob["gamma"], prob["md"], prob["mo"], prob["gvol"])["nll"]     # noqa: E731
    assert held(res["cores"]) < held(prob["cores"])


def test_dot_rule_is_a_sum():
    rng = np.random.default_rng(2)
    for tot in (1, 255, 257, 70000):
        a, b = rng.uniform(0.0, 1.0, tot), rng.uniform(0.0, 1.0, tot)
        assert abs(S.dot_rule(a, b) - float(np.dot(a, b))) <= (tot + 1) * U * float(np.dot(a, b))


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no host C++ compiler")
    return c


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_plan_of_a_lognorm_grad_call(cxx, tmp_path, flags):
    exe = str(tmp_path / "sq_norm_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "ttcross_amd", "csrc"), os.path.join(ROOT, "tests", "sq_norm_plan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"sq norm plan: ok \((\d+) plans\)", r.stdout.strip()), r.stdout
    assert int(re.search(r"\((\d+) plans", r.stdout).group(1)) == 3 * 2 * (15 * 15 * 6 * 6 * 2 + 2)


def test_header_and_library_declare_the_entry_points():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        raw = f.read()
    h = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw, flags=re.S))
    for decl in ("int ttx_sq_lognorm_grad (ttx_engine *h, const double *const *md, const double *const *mo, double gvol, double coef, double *g, int32_t accumulate, int32_t mode, double *z_mant, int64_t *z_exp, double *logz);",
                 "int ttx_sq_lognorm_grad_dev (ttx_engine *h, const double *const *md, const double *const *mo, double gvol, double coef, double *g_dev, int32_t accumulate, int32_t mode, double *z_mant, int64_t *z_exp, double *logz);",
                 "int ttx_sq_lognorm_grad_last(const ttx_engine *h, double *ms_right, double *ms_left, double *ms_asm, double *flops, int32_t *mode_ran);",
                 "int ttx_sq_nll_batch (ttx_engine *h, int64_t npts, const double *x , const ttx_basis *basis , const double *w, double gamma, const double *const *md, const double *const *mo, double gvol, int32_t mode, double *nll, double *logz, double *val, double *g);",
                 "int ttx_sq_nll_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, const double *w_dev, double gamma, const double *const *md, const double *const *mo, double gvol, int32_t mode, double *nll, double *logz, double *val_dev, double *g_dev);"):
        assert decl in h, decl
    assert "Open: the gradient of the normaliser" not in raw and "the gradient of the normaliser Z, ranks above 128" not in raw
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "Open: the gradient of the normaliser" not in f.read()
    with open(os.path.join(ROOT, "ttcross_amd", "csrc", "ttx_op_plan.h")) as f:
        assert re.search(r"#define TTX_SQN_AUTO_FLOPS", f.read())
    import __graft_entry__ as g
    L = ctypes.CDLL(g.build_lib())
    for sym in ENTRIES:
        assert hasattr(L, sym), sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() == 3                                                 # added without a new version
    for m in ("sq_lognorm_grad", "sq_lognorm_grad_last", "sq_nll", "fit_density"):
        assert callable(getattr(E.TTCross, m)), m
    assert callable(E.mass_tridiag)
    for sym in ENTRIES:
        assert getattr(E.load_library(), sym).argtypes is not None, sym
