"""The oracle's tt_lib restatement (oracle/ttx_oracle_tt.c) against the independent reference of tests/tt_ref.py at the edges
of the double range and of the spectra: gauged and uniformly scaled trains (powers of two, so the same tensor), rank
deficiency, flat and graded spectra, tolerances on both sides of a chop threshold, rmax, zero trains, tol >= 1.
The case lists are shared with tests/test_gpu_ttops_edges.py, which holds the device to the same checks."""
import math

import numpy as np
import pytest

import oracle_lib as O
import tt_ref as R

BASE = ([5, 6, 4, 5], [1, 4, 6, 3, 1])
GAUGES = [300, -300, 560, -560, 900, -900]
SCALES = [-1000, -600, 600, 1000]
SCALE_SHAPES = {2: ([6, 5], [1, 4, 1]), 3: ([4, 5, 3], [1, 4, 3, 1]), 6: ([3, 2, 3, 2, 3, 2], [1, 3, 4, 5, 4, 3, 1])}
TOLS = [1e-2, 1e-6, 1e-12]


def spectra_cases():
    """(id, cores, [(tol, rmax), ...]) with the mpmath reference"""
    out = [("rank_deficient", R.rank_deficient(11, [4, 5, 4, 3]), [(1e-10, 0), (1e-3, 0), (0.0, 0)]),
           # equal singular values: which of them survive a cut is arbitrary, so cuts only where a single bond is cut
           ("flat", R.flat(12, [4, 3, 3, 4], 4), [(1e-10, 0), (0.0, 0)]),
           ("flat_d2", R.flat(21, [5, 4], 4), [(0.6, 0), (0.0, 2)]),
           ("graded", R.graded(13, [6, 3, 3, 6], 6, bond=2), [(1e-5, 0), (1e-9, 0), (1e-13, 0), (1e-5, 2)]),
           ("rmax_only", R.rand_train(14, [4, 5, 4], [1, 4, 5, 1]), [(0.0, 2), (1e-1, 3), (1e-14, 1)]),
           ("zero", R.zero_train([3, 4, 3], [1, 2, 3, 1]), [(1e-3, 0), (0.0, 0)]),
           ("zero_core", R.one_zero_core(15, [3, 4, 3, 2], [1, 3, 4, 2, 1], 2), [(1e-3, 0)]),
           ("rank1", R.rand_train(16, [4, 5, 6], [1, 1, 1, 1]), [(1e-8, 0)]),
           ("n1_modes", R.rand_train(17, [1, 5, 1, 4], [1, 3, 3, 2, 1]), [(1e-8, 0), (1e-1, 0)]),
           ("d2", R.rand_train(18, [7, 6], [1, 5, 1]), [(1e-8, 0), (2e-1, 0)]),
           ("d1", R.rand_train(19, [9], [1, 1]), [(1e-8, 0)])]
    # the exact chop threshold at the last bond of a random train, times 1 -+ 1e-6: one rank apart
    c = R.rand_train(20, [4, 5, 4, 3], [1, 4, 6, 3, 1])
    thr = threshold_tol(c, bond=3, keep=2)
    out.append(("threshold", c, [(thr * (1 - 1e-6), 0), (thr * (1 + 1e-6), 0)]))
    return out


def threshold_tol(cores, bond, keep):
    """the tol at which the chop of bond `bond` (the first one the right-to-left pass meets, bond d-1, must be it) goes
    from keeping `keep` + 1 to `keep` singular values: tol^2 |s|^2 = the tail beyond `keep`"""
    assert bond == len(cores) - 1
    ref = R.tt_svd_ref(cores, 1e-30)
    s2 = [x * x for x in ref["spectra"][bond - 1]]
    return math.sqrt(sum(s2[keep:]))


def assert_round(cores_out, ranks_out, cores_in, tol, rmax, ref, what, tol_rel=1e-12):
    """the checks of a rounded train against the reference: ranks, tensor, truncation error"""
    assert list(ranks_out) == list(ref["ranks"]), f"{what}: ranks {list(ranks_out)} vs reference {ref['ranks']}"
    err = R.rel_dist(cores_out, cores_in)
    assert np.isfinite(err), what
    d = len(cores_in)
    if rmax == 0:
        assert err <= math.sqrt(d - 1) * tol * (1 + 1e-9) + tol_rel, f"{what}: error {err} above sqrt(d-1) tol"
    if ref["err"] >= 1e-9:
        assert abs(err - ref["err"]) <= 1e-6 * ref["err"], f"{what}: error {err} vs reference {ref['err']}"
    else:
        assert err <= ref["err"] + tol_rel, f"{what}: error {err} vs reference {ref['err']}"


def _oracle_round(cores, tol, rmax):
    o = O.OracleTT(cores)
    o.svd(tol, rmax)
    return o.cores(), o.ranks


@pytest.mark.parametrize("bond", ["first", "middle", "last"])
@pytest.mark.parametrize("e", GAUGES)
def test_oracle_gauge_invariance(oracle_built, e, bond):
    n, r = BASE
    c0 = R.rand_train(1, n, r)
    k = {"first": 1, "middle": 2, "last": 3}[bond]
    c = R.gauge(c0, k, e)
    nrm = R.norm(c0)
    o = O.OracleTT(c)
    assert abs(o.norm() - nrm) <= 1e-12 * nrm
    o.ort()
    assert list(o.ranks) == R.ort_ranks(c)
    assert R.rel_dist(o.cores(), c0) <= 1e-12
    assert R.orthonormality(o.cores()) <= 1e-12
    for tol in TOLS:
        ref = R.tt_svd_ref(c0, tol)
        assert min(ref["margin"]) >= 1e-6
        co, ro = _oracle_round(c, tol, 0)
        assert_round(co, ro, c0, tol, 0, ref, f"gauge 2^{e} at bond {k}, tol {tol}")
        assert abs(O.OracleTT(c).norm(tol) - R.norm(co)) <= 1e-12 * nrm


@pytest.mark.parametrize("d", sorted(SCALE_SHAPES))
@pytest.mark.parametrize("e", SCALES)
def test_oracle_uniform_scale(oracle_built, e, d):
    n, r = SCALE_SHAPES[d]
    c0 = R.rand_train(30 + d, n, r)
    c = R.scale(c0, e)
    nrm = R.norm(c0)
    got = math.ldexp(O.OracleTT(c).norm(), -e)
    assert abs(got - nrm) <= (1e-12 + 2e-16 * abs(e) * math.log(2)) * nrm, (got, nrm)
    o = O.OracleTT(c)
    o.ort()
    assert R.rel_dist(o.cores(), c0, shift=e) <= 1e-12
    assert R.orthonormality(o.cores()) <= 1e-12
    for tol in TOLS:
        ref = R.tt_svd_ref(c0, tol)
        assert min(ref["margin"]) >= 1e-6, "the case sits on a chop threshold"
        co, ro = _oracle_round(c, tol, 0)
        assert list(ro) == ref["ranks"]
        err = R.rel_dist(co, c0, shift=e)
        assert err <= math.sqrt(d - 1) * tol * (1 + 1e-9) + 1e-12
        if ref["err"] >= 1e-9:
            assert abs(err - ref["err"]) <= 1e-6 * ref["err"]


@pytest.mark.parametrize("case", spectra_cases(), ids=lambda c: c[0])
def test_oracle_spectra(oracle_built, case):
    name, c, tols = case
    for tol, rmax in tols:
        ref = R.tt_svd_ref(c, tol, rmax)
        assert min(ref["margin"], default=math.inf) >= 1e-6, f"{name}: the case sits on a chop threshold"
        co, ro = _oracle_round(c, tol, rmax)
        assert all(np.isfinite(x).all() for x in co), name
        assert_round(co, ro, c, tol, rmax, ref, f"{name} tol {tol} rmax {rmax}")


@pytest.mark.parametrize("tol", [1.0, 1.5, 10.0])
def test_oracle_tol_at_least_one_keeps_rank_one(oracle_built, tol):
    """lib/mat.f90's chop has no floor: at tol >= 1 it would read before the spectrum; the rank stops at 1"""
    c = R.rand_train(40, [5, 6, 4, 5], [1, 4, 6, 3, 1])
    co, ro = _oracle_round(c, tol, 0)
    assert list(ro) == [1, 1, 1, 1, 1] == R.tt_svd_ref(c, tol)["ranks"]
    assert all(np.isfinite(x).all() for x in co)


def test_reference_self_consistency():
    """tt_ref's two precisions agree on a well-conditioned train, and its contractions on the dense tensor"""
    c = R.rand_train(50, [4, 5, 3, 4], [1, 3, 5, 2, 1])
    full = np.einsum("aib,bjc,ckd,dle->ijkl", *c)
    assert abs(R.norm(c) - np.linalg.norm(full)) <= 1e-14 * np.linalg.norm(full)
    assert abs(R.element(c, [2, 3, 1, 4]) - full[1, 2, 0, 3]) <= 1e-14 * np.abs(full).max()
    w = [np.cos(np.arange(1, k + 1)) for k in [4, 5, 3, 4]]
    assert abs(R.quad(c, w) - np.einsum("ijkl,i,j,k,l->", full, *w)) <= 1e-13 * np.abs(full).sum()
    for tol in TOLS:
        a, b = R.tt_svd_ref(c, tol), R.tt_svd_ref(c, tol, prec="f64")
        assert a["ranks"] == b["ranks"]
        assert all(np.allclose(x, y, rtol=0, atol=1e-13) for x, y in zip(a["spectra"], b["spectra"]))
    g = R.gauge(c, 2, -900)
    assert abs(R.norm_log2(g) - R.norm_log2(c)) <= 1e-14
    assert abs(R.log10_norm(R.scale(c, 3000)) - (R.log10_norm(c) + 3000 * math.log10(2))) <= 1e-12
