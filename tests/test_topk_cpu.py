"""ttx_topk / ttx_topk_last without a GPU: the symbols and the Python methods exist, the refusals that precede any device call
(include/ttx.h) are answered, the reference of tests/topk_ref.py is checked against the dense tensor, and the conditions the GPU
tests rely on are asserted on the reference alone."""
import ctypes

import numpy as np
import pytest

import topk_ref as R
from ttcross_amd import engine as E

EINVAL, ESTATE = 1, 4


def test_the_symbols_and_methods_exist():
    L = E.load_library()
    for name in ("ttx_topk", "ttx_topk_last"):
        assert hasattr(L, name)
    assert callable(E.TTCross.topk) and callable(E.TTCross.topk_last)
    assert E.TOPK_WHICH == {"abs": 0, "max": 1, "min": 2}


def test_refusals_before_any_device_call():
    L = E.load_library()
    ind, val = np.zeros((4, 3), np.int32), np.zeros(4)
    nf, bd = ctypes.c_int32(), ctypes.c_double()
    nul_d, nul_i = ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_int32)()

    def call(K=4, which=0, mode=0, nfound=None, i=None, v=None, b=None):
        return L.ttx_topk(None, K, which, nul_i, mode, ctypes.pointer(nf) if nfound is None else nfound, E._ip(ind) if i is None else i,
                          E._dp(val) if v is None else v, ctypes.pointer(bd) if b is None else b)

    assert call(nfound=nul_i) == EINVAL
    assert call(i=nul_i) == EINVAL
    assert call(v=nul_d) == EINVAL
    assert call(b=nul_d) == EINVAL
    for K in (0, -1, 4097):
        assert call(K=K) == EINVAL
        assert b"K =" in L.ttx_last_error()
    for which in (-1, 3):
        assert call(which=which) == EINVAL
    for mode in (-1, 3):
        assert call(mode=mode) == EINVAL
    assert L.ttx_topk_last(None, None, None, None, None, None) == EINVAL
    # sound arguments and no engine: the state error, still without a device
    assert call() == ESTATE
    assert call(K=4096, which=2, mode=2) == ESTATE


def test_python_argument_checks_need_no_engine():
    tt = E.TTCross.__new__(E.TTCross)
    tt.d = 3
    with pytest.raises(ValueError):
        E.TTCross.topk(tt, 4, which="largest")
    with pytest.raises(ValueError):
        E.TTCross.topk(tt, 0)
    with pytest.raises(ValueError):
        E.TTCross.topk(tt, 4, fixed=[0, 0])
    with pytest.raises(ValueError):
        E.TTCross.topk(tt, 4, mode="fast")


@pytest.mark.parametrize("name", R.cases())
def test_shapes_of_the_cases(name):
    cores = R.case(name)
    n, r = R.SHAPES[name]
    assert [c.shape for c in cores] == [(r[k], n[k], r[k + 1]) for k in range(len(n))]
    assert R.dense_of(name).size <= 60000
    if name != "rank1":                                                         # no two modes share a factor
        flat = [c.ravel() for c in cores]
        assert all(a.size != b.size or not np.array_equal(a, b) for j, a in enumerate(flat) for b in flat[:j])


@pytest.mark.parametrize("name", R.cases())
def test_reference_against_the_dense_tensor(name):
    T = R.dense_of(name)
    for K in R.KS:
        res = R.search_of(name, K)
        assert res["nfound"] == min(K, T.size)
        assert np.all((res["ind"] >= 1) & (res["ind"] <= np.array(T.shape)[None, :]))
        assert len({tuple(row) for row in res["ind"]}) == res["nfound"]
        got = T[tuple(res["ind"].T - 1)]
        assert np.allclose(got, res["val"], rtol=1e-12, atol=1e-13 * np.abs(T).max())
        assert np.all(np.diff(np.abs(res["val"])) <= 0)
        # the bound property: everything not returned is at most bound (+ the allowance)
        rest = np.abs(T).copy()
        rest[tuple(res["ind"].T - 1)] = 0.0
        assert rest.max() <= res["bound"] + res["tol_bound"], (K, rest.max(), res["bound"])
        if res["certified"] == "all":
            di, dv = R.dense_topk(T, K)
            assert np.array_equal(di, res["ind"])


def test_rank1_at_k_1_is_the_dense_maximum():
    T = R.dense_of("rank1")
    res = R.search_of("rank1", 1)
    assert tuple(res["ind"][0] - 1) == np.unravel_index(np.argmax(np.abs(T)), T.shape)


@pytest.mark.parametrize("name", ("tiny", "d4"))
def test_k_beyond_the_dense_size_returns_everything_in_order(name):
    T = R.dense_of(name)
    K = 4096
    assert T.size <= K
    for which in ("abs", "max", "min"):
        res = R.search(R.case(name), K, which)
        di, dv = R.dense_topk(T, K, which)
        assert res["nfound"] == T.size and res["bound"] == 0.0
        assert np.array_equal(res["ind"], di)
        assert np.allclose(res["val"], dv, rtol=1e-12, atol=1e-13 * np.abs(T).max())


def test_fixed_modes_search_the_dense_slice():
    T = R.dense_of("d6")
    fixed = [0, 3, 0, 0, 5, 0]
    res = R.search(R.case("d6"), 4096, "abs", fixed)
    di, dv = R.dense_topk(T, 4096, "abs", fixed)
    assert res["nfound"] == 5 ** 4 and np.array_equal(res["ind"], di)


# ---- the conditions the GPU tests rely on ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.cases())
def test_the_gpu_cases_are_decided(name):
    """for every (case, K) of test_gpu_topk.py the score gap at the cut of every mode exceeds twice the derived allowance"""
    for K in R.GPU_KS[name]:
        res = R.search_of(name, K)
        assert not res["nan"]
        worst = min(res["gap"].values())
        assert worst > 1.0, (name, K, res["gap"])


def test_the_gpu_cases_cover_the_issue_s_list():
    assert set(R.GPU_KS) == set(R.cases())
    assert all(set(ks) <= set(R.KS) for ks in R.GPU_KS.values())


def test_the_certificates_on_peaked_are_not_vacuous():
    assert R.search_of("peaked", 16)["certified"] == "all"
    assert R.search_of("peaked", 1)["certified"] == "max"
    one = R.search_of("peaked", 1)
    assert one["bound"] <= abs(one["val"][0])
    # and on a random signed train the bound proves nothing at a small K: both cases are visible to the caller
    assert R.search_of("d4", 4)["certified"] is None
