"""dtt_ort / dtt_svd / dtt_norm / dtt_lognrm on the device at the edges of the double range and of the spectra, held to the
independent reference of tests/tt_ref.py (not the oracle): gauged and uniformly scaled trains (exactly the same tensor,
powers of two), on shapes that reach every QR path (k_qr_own, tall-skinny QR, k_qr<true>/<false>, the tall branch of
svd_impl); rank deficiency, flat and graded spectra, chop thresholds, rmax, zero trains, tol >= 1; argument checks;
lognorm of trains whose norm leaves the double range."""
import math

import numpy as np
import pytest

import tt_ref as R
from test_ttops_ref_cpu import BASE, GAUGES, SCALES, SCALE_SHAPES, TOLS, assert_round, spectra_cases
from ttcross_amd import engine as E

pytestmark = pytest.mark.gpu

W_COS = lambda n: [np.cos(np.arange(1, k + 1)) for k in n]       # noqa: E731


def _cores(t):
    return [t.core(k) for k in range(1, t.d + 1)]


def _round(cores, tol, rmax=0):
    t = E.TTCross.from_cores(cores).svd(tol, rmax)
    return _cores(t), list(t.ranks())


# QR paths: (id, n, r, env).  k_qr_own: small; TSQR: 1632 x 32 unfoldings; without k_qr_own: k_qr<true> (6 x 6 and 36 x 100
# unfoldings, in LDS) and k_qr<false> (3000 x 40 streams from L2 with TSQR off); the tall branch of svd_impl: r(k-1) > n r(k)
PATHS = [("own", list(BASE[0]), list(BASE[1]), {}),
         ("tsqr", [51, 51, 51], [1, 32, 32, 1], {}),
         ("qr_lds", [6, 6, 6], [1, 6, 100, 1], {"TTX_QR_OWN": "0", "TTX_SVD_POLL": "0"}),
         ("qr_stream", [75, 75, 4], [1, 40, 40, 1], {"TTX_QR_OWN": "0", "TTX_TSQR": "0"}),
         ("tall_svd", [5, 3, 2], [1, 5, 12, 1], {})]


def _env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("e", GAUGES)
@pytest.mark.parametrize("path", PATHS, ids=lambda p: p[0])
def test_gauge_invariance(monkeypatch, path, e):
    name, n, r, env = path
    _env(monkeypatch, env)
    c0 = R.rand_train(100 + len(n), n, r)
    d = len(n)
    nrm = R.norm(c0)
    w = W_COS(n)
    q0 = R.quad(c0, w)
    ind = R.probe_indices(n, 4)
    refs = {tol: R.tt_svd_ref(c0, tol, prec="f64") for tol in TOLS}
    for bond in sorted({1, (d + 1) // 2, d - 1}):
        c = R.gauge(c0, bond, e)
        what = f"{name}: gauge 2^{e} at bond {bond}"
        t = E.TTCross.from_cores(c)
        assert abs(t.norm() - nrm) <= 1e-12 * nrm, what
        assert abs(t.quad(w) - q0) <= 1e-12 * nrm, what
        for i in ind:
            assert abs(t.tijk(i) - R.element(c0, i)) <= 1e-12 * nrm, what
        t.ort()
        assert list(t.ranks()) == R.ort_ranks(c), what
        co = _cores(t)
        assert R.rel_dist(co, c0) <= 1e-12, what
        assert R.orthonormality(co) <= 1e-12, what
        for tol, ref in refs.items():
            if min(ref["margin"]) < 1e-8:
                continue
            co, ro = _round(c, tol)
            assert_round(co, ro, c0, tol, 0, ref, f"{what}, svd({tol})", tol_rel=1e-11)
            assert abs(E.TTCross.from_cores(c).norm(tol) - R.norm(co)) <= 1e-12 * nrm, what


@pytest.mark.parametrize("d", sorted(SCALE_SHAPES))
@pytest.mark.parametrize("e", SCALES)
def test_uniform_scale(monkeypatch, e, d):
    """the results times 2^-e are the unscaled results; d = 2, e = -1000 puts every core near 1e-150 (Jacobi test)"""
    n, r = SCALE_SHAPES[d]
    c0 = R.rand_train(30 + d, n, r)
    c = R.scale(c0, e)
    nrm = R.norm(c0)
    t = E.TTCross.from_cores(c)
    assert abs(math.ldexp(t.norm(), -e) - nrm) <= (1e-12 + 2e-16 * abs(e) * math.log(2)) * nrm
    assert abs(t.lognorm() - R.log10_norm(c)) <= 1e-12 * abs(R.log10_norm(c))
    t.ort()
    co = _cores(t)
    assert R.rel_dist(co, c0, shift=e) <= 1e-12
    assert R.orthonormality(co) <= 1e-12
    for tol in TOLS:
        ref = R.tt_svd_ref(c0, tol)
        assert min(ref["margin"]) >= 1e-6, "the case sits on a chop threshold"
        co, ro = _round(c, tol)
        assert ro == ref["ranks"], (tol, ro, ref["ranks"])
        err = R.rel_dist(co, c0, shift=e)
        assert err <= math.sqrt(d - 1) * tol * (1 + 1e-9) + 1e-11
        if ref["err"] >= 1e-9:
            assert abs(err - ref["err"]) <= 1e-6 * ref["err"]


@pytest.mark.parametrize("case", [c for c in spectra_cases() if len(c[1]) > 1], ids=lambda c: c[0])   # (the engine takes d >= 2)
def test_spectra(case):
    name, c, tols = case
    for tol, rmax in tols:
        ref = R.tt_svd_ref(c, tol, rmax)
        assert min(ref["margin"], default=math.inf) >= 1e-6
        co, ro = _round(c, tol, rmax)
        assert all(np.isfinite(x).all() for x in co), name
        assert_round(co, ro, c, tol, rmax, ref, f"{name} tol {tol} rmax {rmax}", tol_rel=1e-11)
    nrm = R.norm(c)
    t = E.TTCross.from_cores(c)
    assert np.isfinite(t.norm()) and abs(t.norm() - nrm) <= 1e-12 * nrm
    t.ort()
    co = _cores(t)
    assert all(np.isfinite(x).all() for x in co), name
    assert R.rel_dist(co, c) <= 1e-12 if nrm > 0 else R.norm(co) == 0.0


# rank sweep across the path boundaries.  Train n = [12, n2, 4 rk + 1], r = [1, min(rk, 12), rk, 1]:
#   ort:  core 2's unfolding has >= 4 rk rows and rk columns -- tall-skinny QR up to 96 columns, k_qr_own's 512 / 256-row caps,
#         k_qr<true>'s 150 KB of LDS, k_qr<false> beyond;
#   svd:  core 3's unfolding is rk x (4 rk + 1): QR of its (4 rk + 1) x rk transpose (the same QR paths), then the Jacobi SVD of
#         an rk x rk triangle -- odd q (15, 17, 31, ...: the dummy player), X and V in LDS up to q = 94 and in global memory above
#         (96, 97, 127, 128: the 140 KB limit), MFMA GEMM sizes that are not multiples of 16 or 4
SWEEP = [1, 2, 15, 16, 17, 31, 33, 63, 64, 65, 96, 97, 127, 128]


@pytest.mark.parametrize("rk", SWEEP)
def test_shape_sweep(rk, monkeypatch, capfd):
    r1 = min(rk, 12)
    n = [12, (4 * rk + r1 - 1) // r1 + 1, 4 * rk + 1]
    c = R.rand_train(200 + rk, n, [1, r1, rk, 1])
    nrm = R.norm(c)
    t = E.TTCross.from_cores(c)
    assert abs(t.norm() - nrm) <= 1e-12 * nrm
    t.ort()
    assert list(t.ranks()) == R.ort_ranks(c) == [1, r1, rk, 1]
    co = _cores(t)
    assert R.rel_dist(co, c) <= 1e-12
    assert R.orthonormality(co) <= 1e-12
    checked = 0
    for tol in (3e-1, 1e-1, 1e-12):
        ref = R.tt_svd_ref(c, tol, prec="f64")
        if min(ref["margin"]) < 1e-8:
            continue
        checked += 1
        monkeypatch.setenv("TTX_JAC_TRACE", "1")
        capfd.readouterr()
        co, ro = _round(c, tol)
        monkeypatch.delenv("TTX_JAC_TRACE")
        assert f"svd core 3: {rk} x {rk}," in capfd.readouterr().err    # the Jacobi SVD ran on the whole rk x rk triangle
        assert ro == ref["ranks"], (rk, tol, ro, ref["ranks"])
        err = R.rel_dist(co, c)
        assert err <= math.sqrt(2) * tol * (1 + 1e-9) + 1e-11
        if ref["err"] >= 1e-9:
            assert abs(err - ref["err"]) <= 1e-6 * ref["err"]
    assert checked >= 2, f"rk {rk}: the tolerances sit on chop thresholds"


@pytest.mark.parametrize("tol", [1.0, 1.5, 10.0])
def test_tol_at_least_one_keeps_rank_one(tol):
    c = R.rand_train(40, [5, 6, 4, 5], [1, 4, 6, 3, 1])
    co, ro = _round(c, tol)
    assert ro == [1, 1, 1, 1, 1] == R.tt_svd_ref(c, tol)["ranks"]
    assert all(np.isfinite(x).all() for x in co)


def test_svd_argument_checks():
    """a NaN or negative tol, or a negative rmax, is refused before any launch: the train is left as it was"""
    c = R.rand_train(41, [4, 5, 4], [1, 3, 4, 1])
    t = E.TTCross.from_cores(c)
    for tol, rmax in [(float("nan"), 0), (-1e-3, 0), (-0.0 - 1.0, 3), (1e-3, -1)]:
        with pytest.raises(E.TTXError, match="dtt_svd"):
            t.svd(tol, rmax)
        assert list(t.ranks()) == [1, 3, 4, 1]
        assert all(np.array_equal(t.core(k), c[k - 1]) for k in range(1, 4))
    nrm = R.norm(c)
    assert abs(t.norm(-1.0) - nrm) <= 1e-12 * nrm                    # ttx_norm: tol < 0 still means "absent"
    assert abs(t.norm(None) - nrm) <= 1e-12 * nrm


@pytest.mark.parametrize("sign", [1, -1])
def test_lognorm_beyond_the_double_range(sign):
    """d = 40, core norms 10^(+-10): log10 |A| = +-400 where norm() is inf / 0"""
    rng = np.random.default_rng(50 + sign)
    d, n, r = 40, [3] * 40, [1] + [4] * 39 + [1]
    c = [rng.standard_normal((r[k], n[k], r[k + 1])) for k in range(d)]
    c = [x * (10.0 ** (10 * sign) / np.linalg.norm(x)) for x in c]
    ref = R.log10_norm(c)
    t = E.TTCross.from_cores(c)
    got = t.lognorm()
    assert abs(got - ref) <= 1e-12 * abs(ref), (got, ref)
    assert abs(t.lognorm(1e-14) - ref) <= 1e-12 * abs(ref)
    assert list(t.ranks()) == r                                       # the train itself is left unchanged
    c2 = R.rand_train(52, [4, 5, 3], [1, 3, 4, 1])
    t2 = E.TTCross.from_cores(c2)
    assert abs(t2.lognorm() - math.log10(t2.norm())) <= 1e-14 * 10
