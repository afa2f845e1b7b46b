"""ttx_topk on the device against the numpy restatement of its definition (tests/topk_ref.py) and against the dense tensor.

The cases and the K of this file are topk_ref's; test_topk_cpu.py asserts on the reference alone that every (case, K) pair is
decided -- the score gap at the cut of every mode exceeds twice the derived allowance -- so the rows must be the reference's rows
in either scoring mode, and that the certificates on `peaked` are not vacuous.  Allowances: topk_ref's docstring."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import topk_ref as R
from ttcross_amd import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("exact", "mfma")


@functools.lru_cache(maxsize=None)
def train(name):
    return E.TTCross.from_cores(R.case(name))


def check_bound_property(T, res, tol, fixed=None):
    """every element (at the fixed indices) that is not returned is <= bound + tol"""
    rest = np.abs(T).copy()
    rest[tuple(res["ind"].T - 1)] = 0.0
    if fixed is not None:
        rest = rest[tuple(slice(None) if not f else slice(f - 1, f) for f in fixed)]
    assert rest.max() <= res["bound"] + tol, (rest.max(), res["bound"], tol)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", R.cases())
def test_rows_values_and_bound_are_the_references(name, mode):
    tt, T = train(name), R.dense_of(name)
    L = E.load_library()
    for K in R.GPU_KS[name]:
        ref = R.search_of(name, K)
        res = tt.topk(K, mode=mode)
        assert tt.topk_last()["mode"] == mode
        assert res["ind"].shape == (min(K, T.size), tt.d) and res["ind"].dtype == np.int32
        assert np.array_equal(res["ind"], ref["ind"]), (name, K, mode)
        assert res["val"].tobytes() == tt.tijk_batch(res["ind"], "exact").tobytes()
        assert res["val"].tobytes() == ref["val"].tobytes()
        print(f"{name} K={K} {mode}: bound {res['bound']:.17g} ref {ref['bound']:.17g} allowance {ref['tol_bound']:.3g}")
        assert abs(res["bound"] - ref["bound"]) <= ref["tol_bound"], (name, K, mode, res["bound"], ref["bound"], ref["tol_bound"])
        assert res["certified"] == ref["certified"] or abs(res["bound"] - np.abs(res["val"])).min() <= ref["tol_bound"]
        check_bound_property(T, res, ref["tol_bound"])
        # the raw entry: nfound, and the tail rows are zeros
        ind, val = np.full((K, tt.d), -7, np.int32), np.full(K, -7.0)
        nf, bd = ctypes.c_int32(), ctypes.c_double()
        assert L.ttx_topk(tt._h, K, 0, None, E.EVAL_MODES[mode], ctypes.byref(nf), E._ip(ind), E._dp(val), ctypes.byref(bd)) == 0
        assert nf.value == min(K, T.size) and np.array_equal(ind[:nf.value], ref["ind"])
        assert not ind[nf.value:].any() and not val[nf.value:].any()
        assert bd.value == res["bound"]


@pytest.mark.parametrize("name", ("d4", "d4_pos", "d3_wide"))
def test_bound_property_after_ort(name):
    """the device's own output against the dense tensor, on the train as built (above) and again after ort()"""
    tt = E.TTCross.from_cores(R.case(name)).ort()
    cores = [tt.core(k) for k in range(1, tt.d + 1)]
    T = R.dense(cores)
    for K in (1, 17, 100):
        ref = R.search(cores, K)
        for mode in MODES:
            res = tt.topk(K, mode=mode)
            assert res["val"].tobytes() == tt.tijk_batch(res["ind"], "exact").tobytes()
            check_bound_property(T, res, ref["tol_bound"])
            if min(ref["gap"].values()) > 1.0:
                assert np.array_equal(res["ind"], ref["ind"])
                assert abs(res["bound"] - ref["bound"]) <= ref["tol_bound"]


def test_certificates_on_peaked():
    tt, T = train("peaked"), R.dense_of("peaked")
    for mode in MODES:
        assert tt.topk(1, mode=mode)["certified"] == "max"
        res = tt.topk(16, mode=mode)
        assert res["certified"] == "all"
        for K in R.KS:
            res = tt.topk(K, mode=mode)
            if res["certified"] == "all":
                di, dv = R.dense_topk(T, K)
                assert np.array_equal(res["ind"], di)
            if res["certified"] is not None:
                assert np.array_equal(res["ind"][0], R.dense_topk(T, 1)[0][0])


def test_which_orders_the_same_survivors_by_signed_value():
    tt = train("d4")
    for K in (5, 64):
        by = {w: tt.topk(K, which=w, mode="exact") for w in ("abs", "max", "min")}
        rows = {w: sorted(map(tuple, by[w]["ind"])) for w in by}
        assert rows["abs"] == rows["max"] == rows["min"]
        assert np.all(np.diff(by["max"]["val"]) <= 0) and np.all(np.diff(by["min"]["val"]) >= 0)
        assert by["max"]["val"].tobytes() == by["min"]["val"][::-1].tobytes()
        for w in ("max", "min"):
            ref = R.search_of("d4", K, w)
            assert np.array_equal(by[w]["ind"], ref["ind"]) and by[w]["bound"] == by["abs"]["bound"]
            assert np.array_equal(tt.topk(K, which=w, mode="mfma")["ind"], ref["ind"])


def test_fixed_modes():
    tt, T = train("d6"), R.dense_of("d6")
    fixed = [0, 3, 0, 0, 5, 0]
    for mode in MODES:
        res = tt.topk(4096, fixed=fixed, mode=mode)
        di, dv = R.dense_topk(T, 4096, "abs", fixed)
        assert res["ind"].shape == (5 ** 4, 6) and res["bound"] == 0.0
        assert np.array_equal(res["ind"], di) and np.all(res["ind"][:, 1] == 3) and np.all(res["ind"][:, 4] == 5)
        ref = R.search(R.case("d6"), 17, "abs", fixed)
        assert min(ref["gap"].values()) > 1.0
        res = tt.topk(17, fixed=fixed, mode=mode)
        assert np.array_equal(res["ind"], ref["ind"]) and abs(res["bound"] - ref["bound"]) <= ref["tol_bound"]
        check_bound_property(T, res, ref["tol_bound"], fixed)
        every = [2, 3, 1, 4, 5, 2]
        res = tt.topk(4, fixed=every, mode=mode)
        assert res["ind"].tolist() == [every] and res["bound"] == 0.0
        assert res["val"].tobytes() == tt.tijk_batch(np.array([every], np.int32), "exact").tobytes()


def test_a_call_repeats_bit_for_bit():
    def digest(res):
        return res["ind"].tobytes() + res["val"].tobytes() + np.float64(res["bound"]).tobytes()

    for name, K in (("d3_wide", 100), ("d6", 64)):
        tt, other = train(name), E.TTCross.from_cores(R.case(name))
        for mode in MODES:
            a = digest(tt.topk(K, mode=mode))
            assert digest(tt.topk(K, mode=mode)) == a
            assert digest(other.topk(K, mode=mode)) == a
            tt.sample(50, seed=1)                                               # shared work space
            tt.marginals()
            assert digest(tt.topk(K, mode=mode)) == a
        assert np.array_equal(tt.topk(K, mode="exact")["ind"], tt.topk(K, mode="mfma")["ind"])


def test_non_finite_cores_in_a_process_of_its_own():
    p = subprocess.run([sys.executable, os.path.join(HERE, "topk_worker.py")], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    out = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert out[mode] == dict(rows=17, in_range=True, distinct=17, bound_is_nan=True, certified=None), out


def test_topk_last():
    tt = E.TTCross.from_cores(R.case("d3_wide"))
    assert tt.topk_last()["mode"] is None
    n, r = R.SHAPES["d3_wide"]
    K = 100
    for mode in MODES:
        tt.topk(K, mode=mode)
        last = tt.topk_last()
        assert last["mode"] == mode and last["ms_gram"] > 0 and last["ms_score"] > 0 and last["ms_select"] > 0
        flops, c = 0.0, 1
        for k in range(len(n) - 1, -1, -1):
            flops += 2.0 * c * n[k] * r[k] * (r[k + 1] + r[k])
            c = min(K, c * n[k])
        assert last["flops"] == flops
    tt.topk(K, mode="auto")
    assert tt.topk_last()["mode"] in MODES


def test_refusals_with_an_engine():
    tt = train("tiny")
    with pytest.raises(E.TTXError, match="fixed"):
        tt.topk(4, fixed=[0, 3, 0])
    with pytest.raises(E.TTXError, match="fixed"):
        tt.topk(4, fixed=[-1, 0, 0])


def test_fortran_topk_rows_equal_the_python_result():
    from conftest import fortran_exe
    exe = fortran_exe("test_tt_topk")
    cores = R.case("d4")
    path = os.path.join(HERE, "_build", "topk_d4.tt")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    tt = train("d4")
    tt.write(path)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    res = tt.topk(4)
    rows = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("row")]
    assert len(rows) == 4 and len(cores) == 4
    for j, f in enumerate(rows):
        assert [int(v) for v in f[1:5]] == res["ind"][j].tolist()
        assert float(f[5]) == res["val"][j]
    bound = [float(ln.split()[1]) for ln in p.stdout.splitlines() if ln.startswith("bound")]
    assert bound == [res["bound"]]
