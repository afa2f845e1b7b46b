"""Value and gradient of the train in a function basis (ttx_basis_grad_batch, ttx_basis_grad_tab, ttx_basis_host_d): what can be
checked without a GPU -- the numpy restatement (tests/basis_grad_ref.py) against basis_ref.chain and against the substitution
route, the host derivative tables against their restatements and against mpmath, the LINEAR rules, the C ABI as declared and
exported, and the plan of a call (tests/basis_grad_plan_main.cpp, plain and under the sanitizers)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import basis_grad_ref as G
import basis_ref as B
import coscoeff_util as CU
import tt_ref as R
from ttcross_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ttx_basis_grad_batch", "ttx_basis_grad_batch_dev", "ttx_basis_grad_tab", "ttx_basis_grad_tab_dev", "ttx_basis_host_d", "ttx_basis_grad_last")
SHAPES = [([7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]), ([3, 4, 2, 5], [1, 2, 70, 3, 1]), ([5, 7], [1, 3, 1]), ([5], [1, 1])]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    """bit for bit, every NaN counted as one value"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])


def _data(n, r, seed, nonneg, npts=40):
    rng = np.random.default_rng(seed)
    if nonneg:
        cores = [rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1])) for k in range(len(n))]
        return cores, [rng.uniform(0.0, 1.0, (npts, nk)) for nk in n], [rng.uniform(0.0, 1.0, (npts, nk)) for nk in n]
    return R.rand_train(seed, n, r), [rng.standard_normal((npts, nk)) for nk in n], [rng.standard_normal((npts, nk)) for nk in n]


def test_header_and_library_declare_the_entry_points():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        raw = f.read()
    h = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw, flags=re.S))
    for decl in ("int ttx_basis_grad_batch (ttx_engine *h, int64_t npts, const double *x , const ttx_basis *basis , double *val, double *grad , int32_t mode);",
                 "int ttx_basis_grad_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, double *val_dev, double *grad_dev, int32_t mode);",
                 "int ttx_basis_grad_tab (ttx_engine *h, int64_t npts, const double *phi, const double *dphi , double *val, double *grad, int32_t mode);",
                 "int ttx_basis_grad_tab_dev (ttx_engine *h, int64_t npts, const double *phi_dev, const double *dphi_dev, double *val_dev, double *grad_dev, int32_t mode);",
                 "int ttx_basis_host_d (const ttx_basis *b, int32_t n, int64_t npts, const double *x, int64_t ldx, double *dphi );",
                 "int ttx_basis_grad_last (const ttx_engine *h, double *ms_table, double *ms_back, double *ms_fwd, double *flops, int32_t *mode_ran, int64_t *chunk_ran);"):
        assert decl in h, decl
    assert "derivative tables (gradients)" not in raw
    with open(os.path.join(ROOT, "ttcross_amd", "csrc", "ttx_basis.h")) as f:
        assert "derivative tables," not in f.read().split("#pragma once")[0].split("Open:")[1].split("\n")[0]
    import __graft_entry__ as g
    L = ctypes.CDLL(g.build_lib())
    for sym in ENTRIES:
        assert hasattr(L, sym), sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() == 3
    for m in ("basis_grad_batch", "basis_grad_tab", "basis_grad_last"):
        assert callable(getattr(E.TTCross, m)), m
    assert callable(E.basis_dtable)
    for sym in ENTRIES:
        assert getattr(E.load_library(), sym).argtypes is not None, sym


@pytest.mark.parametrize("n,r", SHAPES)
def test_val_of_grad_chain_is_basis_refs_chain_bit_for_bit(n, r):
    for nonneg in (False, True):
        cores, phis, dphis = _data(n, r, 5 + len(n), nonneg)
        val, grad = G.grad_chain(cores, phis, dphis)
        assert np.array_equal(_bits(val), _bits(B.chain(cores, phis)))
        assert grad.shape == (40, len(n)) and np.isfinite(grad).all()


@pytest.mark.parametrize("n,r", SHAPES)
def test_grad_chain_agrees_with_the_substituted_chain_within_the_bound(n, r):
    """the independent route: basis_ref.chain on tables whose mode m is dphi.  Its own bound (N u B_m with basis_ref's count) and
    grad_chain's (N_g u B_m) add up to no more than 2 N_g u B_m, since N <= N_g."""
    assert G.count(R.rand_train(1, n, r)) >= B.count(R.rand_train(1, n, r))
    for nonneg in (False, True):
        cores, phis, dphis = _data(n, r, 11 + len(n), nonneg)
        _, grad = G.grad_chain(cores, phis, dphis)
        bnd, Ng = G.bound(cores, phis, dphis), G.count(cores)
        for m in range(len(n)):
            sub = B.chain(cores, G.substituted(phis, dphis, m))
            err = np.abs(grad[:, m] - sub)
            assert np.all(err <= bnd[:, m]), (nonneg, m)
            if nonneg:
                assert np.all(sub > 0.0) and np.all(err <= 2 * Ng * B.U * sub), m
                assert np.array_equal(_bits(bnd[:, m]), _bits(2.0 * Ng * B.U * grad[:, m]))     # B_m is grad_m itself on non-negative data


def test_count_is_the_formula_of_the_derivation():
    cores = R.rand_train(2, [3, 4, 2, 5], [1, 2, 70, 3, 1])
    assert G.count(cores) == (3 * 2 + 2) + (4 * 70 + 2) + (2 * 70 + 2) + (5 * 3 + 2) + 70 + 1


def _linear_points(t, rng):
    t = np.asarray(t, dtype=np.float64)
    span = max(t[-1] - t[0], 1.0)
    pts = [t, np.array([t[0] - 1.0, np.nextafter(t[0], -np.inf), t[-1] + 2.5, np.nextafter(t[-1], np.inf), -np.inf, np.inf, np.nan]),
           rng.uniform(t[0] - 0.1 * span, t[-1] + 0.1 * span, 200)]
    if t.size > 1:
        pts += [np.nextafter(t[1:], -np.inf), np.nextafter(t[:-1], np.inf), 0.5 * (t[1:] + t[:-1])]
    return np.concatenate(pts)


@pytest.mark.parametrize("n", [1, 2, 33])
def test_host_linear_derivative_table_and_its_rules(n):
    rng = np.random.default_rng(200 + n)
    t = np.sort(rng.uniform(-3.0, 5.0, n))
    for nodes in (t, np.linspace(0.0, 1.0, n) if n > 1 else np.array([0.25])):
        x = _linear_points(nodes, rng)
        got = E.basis_dtable(("linear", nodes), n, x)
        assert _same(got, G.dlinear_table(nodes, x))
        nan = np.isnan(x)
        assert np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any()      # a NaN coordinate gives a NaN row, nothing else does
        ok = got[~nan]
        assert np.array_equal(ok.sum(axis=1), np.zeros(ok.shape[0]))           # s + (-s): the rows sum to exactly 0
        assert np.all(np.count_nonzero(ok, axis=1) <= 2)
        out = ~nan & ((x <= nodes[0]) | (x >= nodes[-1]))
        assert not got[out].any()                                               # 0 on and outside the end nodes (the first and last node included)
        inside = ~nan & ~out
        assert n == 1 or np.all(np.count_nonzero(got[inside], axis=1) == 2)
        for i in range(1, n - 1):                                               # the first n points are the nodes: the right-hand rule at interior ones
            s = 1.0 / (nodes[i + 1] - nodes[i])
            want = np.zeros(n)
            want[i], want[i + 1] = -s, s
            assert np.array_equal(got[i], want), i
            # and it is the slope of the table itself to the right of the node
            h = 0.25 * (nodes[i + 1] - nodes[i])
            ph = E.basis_table(("linear", nodes), n, [nodes[i], nodes[i] + h])
            assert np.allclose((ph[1] - ph[0]) / h, got[i], rtol=1e-12, atol=0)


def _cos_cases():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(-10.0, 10.0, 300), [-10.0, 10.0, 0.0, -0.0, 0.3], rng.uniform(-40.0, 40.0, 50)])
    return [(-10.0, 10.0, 65, x, True), (-10.0, 10.0, 7, x, False), (0.125, 3.0, 33, rng.uniform(0.125, 3.0, 200), True), (0.0, 1.0, 1, x, True)]


def test_host_cos_derivative_table_is_the_numpy_restatement_with_the_librarys_sine():
    sin = lambda v: CU.vec("ttx_test_sin", v)                                   # noqa: E731
    for a, b, n, x, halve in _cos_cases():
        got = E.basis_dtable(("cos", a, b, halve) if halve else ("cos", a, b), n, x)
        assert _same(got, G.dcos_table(a, b, n, x, sin=sin)), (a, b, n)
        assert not got[:, 0].any()                                              # j = 0 is 0.0, halved or not
    a, b, n = 0.0, 1.0, 9
    x = np.array([0.5, 2.0 ** 18, 2.0 ** 16, np.nan, np.inf, -np.inf, 0.25])
    got = E.basis_dtable(("cos", a, b), n, x)
    assert _same(got, G.dcos_table(a, b, n, x, sin=sin))
    assert np.array_equal(np.isnan(got), np.isnan(E.basis_table(("cos", a, b), n, x)))          # the NaN rule of phi, entry for entry
    assert got[1, 0] == 0.0 and np.isnan(got[1, 1:]).all() and np.isnan(got[3:6]).all()


def test_host_cos_derivative_table_against_mpmath_at_a_derived_bound():
    """dphi_j against -(j pi / (b - a)) sin(j pi (x - a) / (b - a)) in 40-digit arithmetic, D = j pi / (b - a) the true factor.
    The computed argument is within 7 u |arg| of the true one (six relative perturbations, test_basis_cpu.py), and sin moves by
    no more than its argument: 7 u |arg| D in the result.  ttx_sin lies within one ulp of the run-time library's sine, itself
    within one ulp of the true one (ttx_coscoeff.h; ulp <= u for |sin| <= 1): 2 u D.  The factor (double)j * w carries b - a, pi,
    the division and the product, the product with the sine one more rounding: five relative perturbations on a value of at most
    D, ((1 + u)^5 - 1) <= 6 u.  Bound: |dphi_j - true| <= (8 + 7 |arg|) u D, with the constant rounded up by the second-order
    terms' one more u: (9 + 7 |arg|) u D."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 40
    rng = np.random.default_rng(19)
    for a, b, n in ((-10.0, 10.0, 65), (0.125, 3.0, 33)):
        x = rng.uniform(a, b, 40)
        got = E.basis_dtable(("cos", a, b, True), n, x)
        for p, xv in enumerate(x):
            for j in range(n):
                Dj = j * mp.pi / (mp.mpf(b) - mp.mpf(a))
                arg = Dj * (mp.mpf(float(xv)) - mp.mpf(a))
                true = -Dj * mp.sin(arg)
                err, bnd = abs(mp.mpf(float(got[p, j])) - true), (9 + 7 * abs(arg)) * mp.mpf(2) ** -53 * Dj
                assert err <= bnd, (a, b, j, xv, float(err), float(bnd))


def test_host_derivative_table_refuses_what_the_table_refuses():
    for entry, n, match in ((("cos", 1.0, 1.0), 4, "a < b"), (("linear", [0.0, 2.0, 1.0]), 3, "strictly ascending")):
        with pytest.raises(E.TTXError, match=match) as e:
            E.basis_dtable(entry, n, [0.5])
        assert "ttx_basis_host_d" in str(e.value)
    L = E.load_library()
    x, out = np.array([0.5]), np.zeros(4)
    b = E._Basis(7, 0, 0.0, 1.0, None)
    assert L.ttx_basis_host_d(ctypes.byref(b), 4, 1, E._dp(x), 1, E._dp(out)) == 1 and b"unknown basis kind 7" in L.ttx_last_error()
    b = E._Basis(E.TTX_BASIS_COS, 0, 0.0, 1.0, None)
    assert L.ttx_basis_host_d(ctypes.byref(b), 4, 1, None, 1, E._dp(out)) == 1
    assert L.ttx_basis_host_d(ctypes.byref(b), 4, 0, None, 1, None) == 0


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no host C++ compiler")
    return c


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_plan_of_a_gradient_call(cxx, tmp_path, flags):
    exe = str(tmp_path / "basis_grad_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "ttcross_amd", "csrc"), os.path.join(ROOT, "tests", "basis_grad_plan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"basis grad plan: ok \((\d+) plans\)", r.stdout.strip()), r.stdout
    assert int(re.search(r"\((\d+) plans", r.stdout).group(1)) == (12 + 128 + 1) * 4 * 3 * 8 * 6 * 8
