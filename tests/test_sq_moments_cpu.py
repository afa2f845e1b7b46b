"""Moments and reduced density matrices of the squared density (ttx_sq_moments, TTCross.sq_moments, density_moments, sq_marginal_pdf): what
can be checked without a GPU -- the numpy restatement (tests/sq_moments_ref.py) against a dense long-double contraction of the full tensor
within the bound derived there, the identities on the restatement, moment_tridiag against Gauss-Legendre, the plan of a call
(tests/sq_moments_plan_main.cpp, plain and under the sanitizers), the seed of the sampler test on the numpy sampler, and the C ABI as
declared and exported."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import sample_sq_real_ref as QR
import sq_moments_ref as M
import sq_norm_ref as S
import tt_ref as R
from ttcross_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = S.U
SHAPES = dict(d2=([5, 7], [1, 3, 1]), mixed=([7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]), ragged=([3, 4, 2, 5], [1, 2, 70, 3, 1]))
SAMPLER_SEED = 2027                                                             # test_gpu_sq_moments.py draws with the same seed


def _data(name, nonneg):
    n, r = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 5)
    cores = [rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1])) for k in range(len(n))] if nonneg else R.rand_train(sum(map(ord, name)), n, r)
    nodes = [np.cumsum(rng.uniform(0.2, 1.0, nk)) - 1.0 for nk in n]
    md, mo = E.mass_tridiag(nodes)
    ad, ao = E.moment_tridiag(nodes, 1)
    a2d, a2o = E.moment_tridiag(nodes, 2)
    if len(n) > 2:
        mo[1], ao[1], a2o[1] = None, None, None                                 # a diagonal mode among the tridiagonal ones
    return cores, md, mo, ad, ao, a2d, a2o


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_restatement_agrees_with_a_dense_long_double_contraction(name):
    """within half of bound() (sq_moments_ref's derivation), the factor 1 + 2^-10 for the long double's own error"""
    for nonneg in (False, True):
        cores, md, mo, ad, ao, a2d, a2o = _data(name, nonneg)
        d = len(cores)
        for drop in (None, 1 if d > 2 else 0):
            adx = list(ad)
            if drop is not None:
                adx[drop] = None
            got = M.moments(cores, md, mo, adx, ao, a2d, a2o)
            bnd = M.bound(cores, md, mo, adx, ao, a2d, a2o, got=got)
            true = M.dense_moments(cores, md, mo, adx, ao, a2d, a2o)
            half = 0.5 * (1.0 + 2.0 ** -10)
            zm, ze, _, _ = S.lognorm_grad(cores, md, mo)
            assert got["z_mant"] == zm and got["z_exp"] == ze
            assert np.all(np.abs(got["m1"] - true["m1"]).astype(np.float64) <= half * bnd["m1"]), (nonneg, drop)
            assert np.all(np.abs(got["c2"] - true["c2"]).astype(np.float64) <= half * bnd["c2"]), (nonneg, drop)
            assert np.array_equal(got["c2"], got["c2"].T)
            if drop is not None:
                assert got["m1"][drop] == 0.0 and not got["c2"][drop].any() and not got["c2"][:, drop].any()
            for k in range(d):
                B = true["B"][k]
                assert np.all(np.abs(got["bd"][k] - np.diag(B)).astype(np.float64) <= half * bnd["bd"][k]), (nonneg, k)
                assert np.all(np.abs(got["bo"][k][:-1] - np.diag(B, 1)).astype(np.float64) <= half * bnd["bo"][k][:-1]) and got["bo"][k][-1] == 0.0
            if nonneg:                                                          # no cancellation: the bound is relative, a dropped term shows
                assert bnd["rho"] <= 1.0 + 1e-9 and all(np.all(b <= 2.0 * U * (2 * bnd["C"] + 2) * np.abs(x) * 1.01) for b, x in zip(bnd["bd"], got["bd"]))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_identities_on_the_restatement(name):
    """sum B_k M_k = 1; m1 from the band; with A_l = M_l, c2[k][l] = m1[k]; with both, 1 -- each within the two sides' bounds and the
    short sum's own rounding"""
    cores, md, mo, ad, ao, a2d, a2o = _data(name, False)
    d = len(cores)
    got = M.moments(cores, md, mo, ad, ao, a2d, a2o)
    bnd = M.bound(cores, md, mo, ad, ao, a2d, a2o, got=got)

    def tr(k, xd, xo):
        return M.band_trace(got["bd"][k], got["bo"][k], bnd["bd"][k], bnd["bo"][k], xd, xo)
    for k in range(d):
        one, a1 = tr(k, md[k], mo[k])
        assert abs(one - 1.0) <= a1, (k, one)
        m, a2 = tr(k, ad[k], ao[k])
        assert abs(m - got["m1"][k]) <= a2 + bnd["m1"][k], k
        s, a3 = tr(k, a2d[k], a2o[k])
        assert abs(s - got["c2"][k, k]) <= a3 + bnd["c2"][k, k], k
    if d > 1:
        mixed = list(ad[:1]) + list(md[1:]), list(ao[:1]) + list(mo[1:])
        g2 = M.moments(cores, md, mo, mixed[0], mixed[1], band=False)
        b2 = M.bound(cores, md, mo, mixed[0], mixed[1], band=False, got=g2)
        for l in range(1, d):
            assert abs(g2["c2"][0, l] - got["m1"][0]) <= b2["c2"][0, l] + bnd["m1"][0]
        g3 = M.moments(cores, md, mo, md, mo, band=False)
        b3 = M.bound(cores, md, mo, md, mo, band=False, got=g3)
        assert np.all(np.abs(g3["c2"] - 1.0)[~np.eye(d, dtype=bool)] <= b3["c2"][~np.eye(d, dtype=bool)]) and np.all(np.abs(g3["m1"] - 1.0) <= b3["m1"])


def test_moment_tridiag_against_gauss_legendre():
    rng = np.random.default_rng(8)
    for n in (2, 3, 9, 40):
        t = np.cumsum(rng.uniform(0.05, 2.0, n)) - 3.0
        assert all(np.array_equal(a, b) for a, b in zip(E.moment_tridiag(t, 0), E.mass_tridiag(t)))
        for power in (0, 1, 2):
            dg, of = E.moment_tridiag(t, power)
            gd, go = M.moment_tridiag_gl(t, power)
            # the closed forms and the rule both round a handful of times per entry relative to the integral of |x|^power phi phi
            ad_, ao_ = M.moment_tridiag_gl(t, 0)
            scale = np.max(np.abs(t)) ** power
            assert dg.shape == (n,) and of.shape == (n - 1,)
            assert np.all(np.abs(dg - gd) <= 32 * U * scale * ad_) and np.all(np.abs(of - go) <= 32 * U * scale * ao_), (n, power)
    lst = E.moment_tridiag([np.array([0.0, 1.0, 3.0]), np.array([2.0])], 2, [None, None])
    assert np.array_equal(lst[0][1], np.array([4.0])) and lst[1][1].size == 0
    held = E.moment_tridiag(np.array([0.0, 1.0, 3.0]), 1, 2.0)
    mh = E.mass_tridiag(np.array([0.0, 1.0, 3.0]), 2.0)
    assert np.array_equal(held[0], 2.0 * mh[0]) and np.array_equal(held[1], 2.0 * mh[1])
    assert all(np.array_equal(a, b) for a, b in zip(E.moment_tridiag(np.array([0.0, 1.0, 3.0]), 0, 2.0), mh))
    with pytest.raises(ValueError):
        E.moment_tridiag(np.array([0.0, 1.0]), 3)


def exact_density_moments(prob):
    """mean and cov of q = (f^2 + gamma) / (Z + gamma V) on the pinned problem, from the restatement: what density_moments computes"""
    cores, nodes, gamma = prob["cores"], prob["nodes"], prob["gamma"]
    ad, ao = E.moment_tridiag(nodes, 1)
    a2d, a2o = E.moment_tridiag(nodes, 2)
    res = M.moments(cores, prob["md"], prob["mo"], ad, ao, a2d, a2o, band=False)
    alpha = res["z_mant"] / (res["z_mant"] + float(np.ldexp(prob["gvol"], -res["z_exp"])))
    lo, hi = np.array([t[0] for t in nodes]), np.array([t[-1] for t in nodes])
    um = 0.5 * (lo + hi)
    usec = np.outer(um, um)
    usec[np.diag_indices(len(nodes))] = (lo * lo + lo * hi + hi * hi) / 3.0
    mean = alpha * res["m1"] + (1.0 - alpha) * um
    return mean, alpha * res["c2"] + (1.0 - alpha) * usec - np.outer(mean, mean), alpha


def test_the_seed_of_the_sampler_test_on_the_numpy_sampler():
    """1e5 points of the numpy restatement of sample_sq_real with the GPU test's seed: mean within 5 standard errors from the moments
    themselves, covariance within 5 from the sample's fourth moments"""
    prob = S.fit_problem()
    mean, cov, alpha = exact_density_moments(prob)
    assert 0.0 < alpha < 1.0 and np.all(np.linalg.eigvalsh(cov) > 0.0)
    u = np.random.default_rng(SAMPLER_SEED).random((100000, 3))
    x, _, _, _, failed = QR.draw(prob["cores"], prob["nodes"], u, None, prob["gamma"])
    assert not failed.any()
    okm, okc, rm, rc = M.sample_check(x, mean, cov)
    print("worst mean ratio", rm, "worst cov ratio", rc)
    assert okm and okc, (rm, rc)


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no host C++ compiler")
    return c


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_plan_of_a_moments_call(cxx, tmp_path, flags):
    exe = str(tmp_path / "sq_moments_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "ttcross_amd", "csrc"), os.path.join(ROOT, "tests", "sq_moments_plan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"sq moments plan: ok \((\d+) plans\)", r.stdout.strip()), r.stdout
    assert int(re.search(r"\((\d+) plans", r.stdout).group(1)) == 3 * 4 * (3 + 32 * 8 + 2 + 5)
    assert M.steps_of([0, 7, 8, 127, 253, 254]) == 254 + 247 + 246 + 127 + 1 and M.steps_of(list(range(63))) == 63 * 62 // 2


def test_header_and_library_declare_the_entry_points():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        raw = f.read()
    h = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw, flags=re.S))
    assert ("int ttx_sq_moments(ttx_engine *h, const double *const *md, const double *const *mo, const double *const *ad, const double *const *ao, "
            "const double *const *a2d, const double *const *a2o, int32_t mode, double *z_mant, int64_t *z_exp, double *bd, double *bo, double *m1 , double *c2 );") in h
    assert "int ttx_sq_moments_last(const ttx_engine *h, double *ms_chains, double *ms_band, double *ms_carry, double *ms_close, double *flops, int64_t *steps, int32_t *mode_ran);" in h
    assert "a Hessian of Z" in raw
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "Open: two-mode marginal densities, higher moments, ranks above 128" in f.read()
    with open(os.path.join(ROOT, "ttcross_amd", "csrc", "ttx_op_plan.h")) as f:
        plan = f.read()
    assert re.search(r"#define TTX_SQM_AUTO_FLOPS", plan) and "PROVISIONAL" in plan and re.search(r"#define TTX_SQM_CAP_BYTES", plan)
    import __graft_entry__ as g
    L = ctypes.CDLL(g.build_lib())
    for sym in ("ttx_sq_moments", "ttx_sq_moments_last"):
        assert hasattr(L, sym), sym
        assert getattr(E.load_library(), sym).argtypes is not None, sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() == 3                                                 # added without a new version
    for m in ("sq_moments", "sq_moments_last", "density_moments", "sq_marginal_pdf"):
        assert callable(getattr(E.TTCross, m)), m
    assert callable(E.moment_tridiag)
