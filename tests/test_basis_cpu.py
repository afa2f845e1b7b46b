"""The train in a function basis (ttx_basis_batch, ttx_basis_tab, ttx_basis_host): what can be checked without a GPU -- the C-ABI
as declared and exported, the host tables against their numpy restatements (tests/basis_ref.py), the refusals that come before
any device call, and the reference chain with unit vectors against the chain of dtt_ijk."""
import ctypes
import os
import re

import numpy as np
import pytest

import basis_ref as B
import coscoeff_util as CU
import oracle_lib as O
import tt_ref as R
from ttcross_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ttx_basis_batch", "ttx_basis_batch_dev", "ttx_basis_tab", "ttx_basis_tab_dev", "ttx_basis_host", "ttx_basis_last")


def _header():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    """bit for bit, every NaN counted as one value"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(_bits(a)[~np.isnan(a)], _bits(b)[~np.isnan(b)])


def test_header_declares_the_entry_points_and_constants():
    h = _header()
    for decl in ("int ttx_basis_batch (ttx_engine *h, int64_t npts, const double *x , const ttx_basis *basis , double *out, int32_t mode);",
                 "int ttx_basis_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, double *out_dev, int32_t mode);",
                 "int ttx_basis_tab (ttx_engine *h, int64_t npts, const double *phi , double *out, int32_t mode);",
                 "int ttx_basis_tab_dev (ttx_engine *h, int64_t npts, const double *phi_dev, double *out_dev, int32_t mode);",
                 "int ttx_basis_host (const ttx_basis *b, int32_t n, int64_t npts, const double *x, int64_t ldx, double *phi );",
                 "int ttx_basis_last (const ttx_engine *h, double *ms_table, double *ms_chain, double *flops, int32_t *mode_ran);",
                 "typedef struct { int32_t kind, flags; double a, b; const double *nodes ; } ttx_basis;"):
        assert decl in h, decl
    for name, val in (("TTX_BASIS_COS", 1), ("TTX_BASIS_LINEAR", 2), ("TTX_BASIS_HALVE_FIRST", 1)):
        assert re.search(rf"#define {name} {val}\b", h), name


def test_library_exports_the_entry_points_and_keeps_its_version():
    import __graft_entry__ as g
    L = ctypes.CDLL(g.build_lib())
    for sym in ENTRIES:
        assert hasattr(L, sym), sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() == 3


def test_engine_module_mirrors_them():
    assert (E.TTX_BASIS_COS, E.TTX_BASIS_LINEAR, E.TTX_BASIS_HALVE_FIRST) == (1, 2, 1)
    assert E.BASIS_KINDS == {"cos": 1, "linear": 2}
    for m in ("basis_batch", "basis_tab", "basis_last"):
        assert callable(getattr(E.TTCross, m)), m
    assert callable(E.basis_table)
    L = E.load_library()
    for sym in ENTRIES:
        assert getattr(L, sym).argtypes is not None, sym
    assert ctypes.sizeof(E._Basis) == 32 and E._Basis.a.offset == 8 and E._Basis.nodes.offset == 24


def _linear_points(t, rng):
    t = np.asarray(t, dtype=np.float64)
    span = max(t[-1] - t[0], 1.0)
    pts = [t, np.array([t[0] - 1.0, t[0] - 1e-300, np.nextafter(t[0], -np.inf), t[-1] + 2.5, np.nextafter(t[-1], np.inf), -np.inf, np.inf, np.nan]),
           rng.uniform(t[0] - 0.1 * span, t[-1] + 0.1 * span, 200)]
    if t.size > 1:
        pts += [np.nextafter(t[1:], -np.inf), np.nextafter(t[:-1], np.inf), 0.5 * (t[1:] + t[:-1])]
    return np.concatenate(pts)


@pytest.mark.parametrize("n", [1, 2, 33])
def test_host_linear_table_is_the_numpy_restatement_bit_for_bit(n):
    rng = np.random.default_rng(100 + n)
    t = np.sort(rng.uniform(-3.0, 5.0, n))
    assert np.all(np.diff(t) > 0)
    for nodes in (t, np.linspace(0.0, 1.0, n) if n > 1 else np.array([0.25])):
        x = _linear_points(nodes, rng)
        got, ref = E.basis_table(("linear", nodes), n, x), B.linear_table(nodes, x)
        assert _same(got, ref)
        assert np.isnan(got[np.isnan(x)]).all() and not np.isnan(got[~np.isnan(x)]).any()
        ok = ~np.isnan(x)
        assert np.all(np.count_nonzero(got[ok], axis=1) <= 2)
        assert np.allclose(got[ok].sum(axis=1), 1.0, rtol=0, atol=4 * B.U)        # a partition of unity: lambda + (1 - lambda)
        on = np.arange(n)                                                          # the first n points are the nodes themselves
        assert np.array_equal(got[on], np.eye(n))


def _cos_cases():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-10.0, 10.0, 300), [-10.0, 10.0, 0.0, -0.0, 0.3], rng.uniform(-40.0, 40.0, 50)])
    return [(-10.0, 10.0, 65, x, True), (-10.0, 10.0, 7, x, False), (0.125, 3.0, 33, rng.uniform(0.125, 3.0, 200), True), (0.0, 1.0, 1, x, True)]


def test_host_cos_table_is_the_numpy_restatement_with_the_librarys_cosine():
    for a, b, n, x, halve in _cos_cases():
        got = E.basis_table(("cos", a, b, halve) if halve else ("cos", a, b), n, x)
        ref = B.cos_table(a, b, n, x, halve, cos=lambda v: CU.vec("ttx_test_cos", v))
        assert _same(got, ref), (a, b, n)
    # beyond the range of ttx_cos and at non-finite coordinates: NaN for exactly the entries the header names
    a, b, n = 0.0, 1.0, 9
    x = np.array([0.5, 2.0 ** 18, 2.0 ** 16, np.nan, np.inf, -np.inf, 0.25])
    got = E.basis_table(("cos", a, b), n, x)
    assert _same(got, B.cos_table(a, b, n, x, cos=lambda v: CU.vec("ttx_test_cos", v)))
    with np.errstate(invalid="ignore"):
        arg = np.arange(n)[None, :] * ((x - a) * (B.PI / (b - a)))[:, None]
        want_nan = ~(np.abs(arg) <= B.TRIG_MAX)
    assert np.array_equal(np.isnan(got), want_nan)
    assert not np.isnan(got[0]).any() and not np.isnan(got[6]).any() and np.isnan(got[3:6]).all()
    assert got[1, 0] == 1.0 and np.isnan(got[1, 1:]).all()                      # j = 0: arg = 0 whatever the (finite) coordinate


def test_host_cos_table_against_mpmath_at_a_derived_bound():
    """phi_j against c_j cos(j pi (x - a)/(b - a)) in 40-digit arithmetic.  The computed argument carries six relative
    perturbations of at most u each -- x - a, b - a, the constant pi (its double is within u relative of pi), the division that
    gives w, the product (x - a) w, the product j y -- so |arg - true| <= ((1 + u)^6 - 1) |true| <= 7 u |true|, and cos moves by no
    more than its argument.  ttx_cos lies within one ulp of the run-time library's cos (test_coscoeff_cpu.py), which is itself
    within one ulp of the true cosine; a value of magnitude at most 1 has ulp <= u, so the cosine adds 2 u.  The halving is exact.
    Bound: |phi_j - true| <= (2 + 7 |arg_true|) u."""
    mpmath = pytest.importorskip("mpmath")
    mp = mpmath.mp
    mp.dps = 40
    rng = np.random.default_rng(17)
    for a, b, n, halve in ((-10.0, 10.0, 65, True), (0.125, 3.0, 33, False)):
        x = rng.uniform(a, b, 40)
        got = E.basis_table(("cos", a, b, halve), n, x)
        for p, xv in enumerate(x):
            for j in range(n):
                arg = j * mp.pi * (mp.mpf(float(xv)) - mp.mpf(a)) / (mp.mpf(b) - mp.mpf(a))
                true = mp.cos(arg) * (mp.mpf(0.5) if (halve and j == 0) else 1)
                err, bnd = abs(mp.mpf(float(got[p, j])) - true), (2 + 7 * abs(arg)) * mp.mpf(2) ** -53
                assert err <= bnd, (a, b, j, xv, float(err), float(bnd))


@pytest.mark.parametrize("entry,n,match", [
    (("cos", 1.0, 1.0), 4, "a < b"), (("cos", 2.0, 1.0), 4, "a < b"), (("cos", 0.0, float("inf")), 4, "a < b"), (("cos", float("nan"), 1.0), 4, "a < b"),
    (("linear", [0.0, 2.0, 1.0]), 3, "strictly ascending"), (("linear", [0.0, 1.0, 1.0]), 3, "strictly ascending"), (("linear", [0.0, float("nan"), 1.0]), 3, "not finite"),
])
def test_host_table_refuses_bad_descriptors(entry, n, match):
    with pytest.raises(E.TTXError, match=match) as e:
        E.basis_table(entry, n, [0.5])
    assert "ttx_basis_host" in str(e.value)


def test_host_table_refuses_an_unknown_kind_and_null_arguments():
    L = E.load_library()
    x, phi = np.array([0.5]), np.zeros(4)
    dp = ctypes.POINTER(ctypes.c_double)
    b = E._Basis(7, 0, 0.0, 1.0, None)
    assert L.ttx_basis_host(ctypes.byref(b), 4, 1, x.ctypes.data_as(dp), 1, phi.ctypes.data_as(dp)) == 1
    assert b"ttx_basis_host" in L.ttx_last_error() and b"unknown basis kind 7" in L.ttx_last_error()
    b = E._Basis(E.TTX_BASIS_COS, 0, 0.0, 1.0, None)
    assert L.ttx_basis_host(ctypes.byref(b), 4, 1, None, 1, phi.ctypes.data_as(dp)) == 1
    assert L.ttx_basis_host(ctypes.byref(b), 4, -1, x.ctypes.data_as(dp), 1, phi.ctypes.data_as(dp)) == 1
    assert L.ttx_basis_host(None, 4, 1, x.ctypes.data_as(dp), 1, phi.ctypes.data_as(dp)) == 1
    assert L.ttx_basis_host(ctypes.byref(b), 4, 0, None, 1, None) == 0          # an empty batch
    b = E._Basis(E.TTX_BASIS_LINEAR, 0, 0.0, 0.0, None)
    assert L.ttx_basis_host(ctypes.byref(b), 4, 1, x.ctypes.data_as(dp), 1, phi.ctypes.data_as(dp)) == 1
    assert b"without nodes" in L.ttx_last_error()


def test_python_wrappers_refuse_malformed_entries():
    for bad in (("sin", 0.0, 1.0), ("cos", 0.0), ("linear",), "cos", ("linear", [0.0, 1.0, 2.0])):
        with pytest.raises(ValueError):
            E.basis_table(bad, 4, [0.5])


def _ind(n, seed, npts=64):
    rng = np.random.default_rng(seed)
    n = np.asarray(n)
    return np.vstack([rng.integers(0, 2 ** 31 - 1, (npts, n.size)) % n + 1, np.ones((1, n.size), np.int64), n[None, :]]).astype(np.int32)


@pytest.mark.parametrize("n,r", [([7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]), ([4, 5, 3, 2], [1, 16, 33, 65, 1]), ([5, 7], [1, 3, 1])])
def test_chain_with_unit_vectors_is_the_chain_of_dtt_ijk_bit_for_bit(n, r):
    """0.0 + 1.0 * t adds nothing: against the oracle's dtt_ijk (sums from 0.0 over ascending k, the chain ttx_ijk_batch's exact mode
    restates) on random trains, and against tt_ref.element on a train of small integers, where every order gives the same bits."""
    cores = R.rand_train(3 + len(n), n, r)
    ind = _ind(n, 9)
    ot = O.OracleTT(cores)
    want = np.array([ot.ijk(row) for row in ind])
    got = B.chain(cores, B.unit_tables(n, ind))
    assert np.array_equal(got, want)                                            # == : the sign of a zero is not compared
    rng = np.random.default_rng(4)
    ints = [rng.integers(-3, 4, c.shape).astype(np.float64) for c in cores]
    got = B.chain(ints, B.unit_tables(n, ind))
    assert np.array_equal(got, np.array([R.element(ints, row) for row in ind]))


def test_reference_bound_holds_for_a_blocked_evaluation():
    """the bound of basis_ref against another summation order (einsum over whole cores), random signs and non-negative data"""
    n, r = [7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]
    rng = np.random.default_rng(8)
    for nonneg in (False, True):
        cores = [rng.uniform(0.0, 1.0, c.shape) if nonneg else c for c in R.rand_train(21, n, r)]
        phis = [rng.uniform(0.0, 1.0, (50, nk)) if nonneg else rng.standard_normal((50, nk)) for nk in n]
        ref = B.chain(cores, phis)
        x = np.ones((50, 1))
        for c, ph in zip(cores[::-1], phis[::-1]):
            x = np.einsum("ajk,pj,pk->pa", c, ph, x, optimize=True)
        assert np.all(np.abs(x[:, 0] - ref) <= B.bound(cores, phis))
        if nonneg:
            assert np.all(np.abs(x[:, 0] - ref) <= 2 * B.count(cores) * B.U * ref)
