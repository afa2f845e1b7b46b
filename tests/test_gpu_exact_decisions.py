"""The decisions of ttx_topk and ttx_sample at exact ties, on integer trains (tests/exact_cases.py).

Every product and sum of either call is an exact double on these trains, so plain loops, v_mfma_f64_16x16x4_f64, numpy and the
marginals kernels give the same bits and the definitions of include/ttx.h have ONE answer: every comparison here is equality with
topk_ref.search / sample_ref.draw as they stand, with no allowance and no excluded case.  Two numbers are not sums of integers:
bound, a square root that rounds once (2^-52 relative: topk_ref's own allowance with its accumulated term E = 0), and logq
(test_gpu_sample.py's _logq_bound).  tests/test_exact_decisions_cpu.py asserts on the references alone that the cut of every
selection falls inside a group of equal scores, that the groups cross chunks of 4096 positions, and that every t lies exactly on
an edge of the CDF, where sample_ref.verify calls more than 90 % of the samples undecided."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import exact_cases as X
import sample_ref as S
import topk_ref as R
from test_gpu_sample import _logq_bound                                         # d (4 N u + 8 u (1 + |log term|)): its docstring derives it
from ttcross_amd import engine as E

MODES = ("exact", "mfma")
EINVAL = 1


@functools.lru_cache(maxsize=None)
def train(name):
    return E.TTCross.from_cores(X.topk_case(name))


def _raw(tt, K, which="abs", fixed=None, mode="exact"):
    """ttx_topk itself on buffers full of a sentinel: (nfound, ind [K][d], val [K], bound)"""
    L = E.load_library()
    ind, val = np.full((K, tt.d), -7, np.int32), np.full(K, -7.0)
    nf, bd = ctypes.c_int32(-7), ctypes.c_double(-7.0)
    fx = None if fixed is None else np.ascontiguousarray(fixed, dtype=np.int32)
    rc = L.ttx_topk(tt._h, K, E.TOPK_WHICH[which], E._ip(fx), E.EVAL_MODES[mode], ctypes.byref(nf), E._ip(ind), E._dp(val), ctypes.byref(bd))
    assert rc == 0, (rc, L.ttx_last_error())
    return nf.value, ind, val, bd.value


def _digest(res):
    return res["ind"].tobytes() + res["val"].tobytes() + np.float64(res["bound"]).tobytes()


def _check_against(tt, ref, K, which="abs", fixed=None):
    """both modes against a reference search; returns the digest the two modes share"""
    out = []
    for mode in MODES:
        res = tt.topk(K, which=which, fixed=fixed, mode=mode)
        assert tt.topk_last()["mode"] == mode
        assert res["ind"].dtype == np.int32 and np.array_equal(res["ind"], ref["ind"]), (K, which, mode)
        assert res["val"].tobytes() == ref["val"].tobytes()
        assert res["val"].tobytes() == tt.tijk_batch(res["ind"], "exact").tobytes()
        assert res["certified"] == ref["certified"]
        print(f"K={K} {which} {mode}: bound {res['bound']:.17g} ref {ref['bound']:.17g}")
        assert abs(res["bound"] - ref["bound"]) <= 2.0 ** -52 * ref["bound"], (K, mode, res["bound"], ref["bound"])
        nf, ind, val, bd = _raw(tt, K, which, fixed, mode)
        assert nf == ref["nfound"] and np.array_equal(ind[:nf], ref["ind"]) and val[:nf].tobytes() == ref["val"].tobytes()
        assert not ind[nf:].any() and not val[nf:].any()                        # the tail rows are zeros
        assert bd == res["bound"]
        out.append(_digest(res))
    assert out[0] == out[1]                                                     # the scores are exact in both modes
    return out[0]


@pytest.mark.parametrize("name,K", [(name, K) for name, c in X.TOPK.items() for K in c["K"]])
def test_topk_keeps_the_references_rows_at_exact_ties(name, K):
    tt = train(name)
    _check_against(tt, X.topk_search(name, K), K)


@pytest.mark.parametrize("name,K", X.WHICH_CASES)
def test_topk_orders_rows_that_tie_in_abs_val(name, K):
    tt = train(name)
    for which in ("abs", "max", "min"):
        _check_against(tt, X.topk_search(name, K, which), K, which)


def test_topk_with_a_fixed_mode():
    name, K, fixed = X.FIXED_CASE
    ref = X.topk_search(name, K, "abs", fixed)
    _check_against(train(name), ref, K, "abs", list(fixed))
    assert np.all(ref["ind"][:, 1] == fixed[1])


@pytest.mark.parametrize("name", list(X.TOPK))
def test_topk_repeats_bit_for_bit(name):
    tt, K = train(name), X.TOPK[name]["K"][-1]
    for mode in MODES:
        assert _digest(tt.topk(K, mode=mode)) == _digest(tt.topk(K, mode=mode))


def test_topk_refuses_a_sheet_one_mode_size_too_large():
    """n = (3, 4097): K = 4096 would need 2^24 + 4096 pairs; K = 4095 on the same engine then runs, and keeps the reference's rows"""
    L = E.load_library()
    cores = X.refusal_train()
    tt = E.TTCross.from_cores(cores)
    K = 4096
    ind, val = np.full((K, 2), -7, np.int32), np.full(K, -7.0)
    nf, bd = ctypes.c_int32(-7), ctypes.c_double(-7.0)
    for mode in MODES:
        rc = L.ttx_topk(tt._h, K, 0, None, E.EVAL_MODES[mode], ctypes.byref(nf), E._ip(ind), E._dp(val), ctypes.byref(bd))
        assert rc == EINVAL and b"sheet" in L.ttx_last_error()
        assert nf.value == -7 and bd.value == -7.0 and np.all(ind == -7) and np.all(val == -7.0)      # nothing was written
        with pytest.raises(E.TTXError):
            tt.topk(K, mode=mode)
    assert tt.topk_last()["mode"] is None                                       # and nothing ran
    _check_against(tt, R.search(cores, 4095), 4095)


# ---- sampling --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sampler(name):
    return E.TTCross.from_cores(X.sample_case(name)[0])


def _check_samples(tt, cores, u, w=None):
    ref_ind, ref_logq, ref_val, ref_failed = S.draw(cores, u, w)
    assert not ref_failed.any()
    res = tt.sample(u, w)
    assert tt.sample_last()["failed"] == 0
    off = np.flatnonzero(np.any(res["ind"] != ref_ind, axis=1))
    assert off.size == 0, (off.size, [(int(s), u[s].tolist(), res["ind"][s].tolist(), ref_ind[s].tolist()) for s in off[:5]])
    assert res["val"].tobytes() == tt.tijk_batch(res["ind"], "exact").tobytes()
    assert res["val"].tobytes() == ref_val.tobytes()                            # integers: the reference's own bits too
    chk = S.verify(cores, u, w, None, res["ind"])
    assert np.array_equal(chk["logq"], ref_logq)
    bound = _logq_bound(len(cores), chk["N"], chk["maxlog"])
    diff = np.abs(res["logq"] - ref_logq)
    print("max |logq - ref| / bound", float((diff / bound).max()), "undecided for verify", chk["undecided"], "of", u.shape[0])
    assert np.all(diff <= bound)
    return res


@pytest.mark.parametrize("name", list(X.SAMPLE))
def test_sample_draws_the_definitions_index_on_every_edge(name):
    c = X.SAMPLE[name]
    cores, u = X.sample_case(name)
    res = _check_samples(sampler(name), cores, u)
    assert np.array_equal(res["ind"], X.edge_closed_form(c["n"], c["q"], c["zero"], u))


@pytest.mark.parametrize("name", list(X.SAMPLE))
def test_sample_one_ulp_below_every_edge(name):
    cores, u = X.sample_case(name)
    v = X.below(u)
    assert np.all(v[u > 0.0] < u[u > 0.0]) and np.array_equal(v[u == 0.0], u[u == 0.0])
    _check_samples(sampler(name), cores, v)


def test_sample_with_power_of_two_weights_and_zeros():
    cores, u = X.sample_case(X.WEIGHTED)
    w = list(X.weights(X.WEIGHTED))
    tt = sampler(X.WEIGHTED)
    res = _check_samples(tt, cores, u, w)
    for k, q in enumerate(w):
        assert np.all(q[res["ind"][:, k] - 1] > 0.0)
    _check_samples(tt, cores, X.below(u), w)
