"""Sums and elementwise products of trains (ttx_lincomb, ttx_hadamard): what can be checked without a GPU -- the numpy reference
of tests/algebra_ref.py against dense tensors at the bounds its docstring derives, the C-ABI as declared and as exported, and
the refusals that come before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

import algebra_ref as A
import tt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
N = [4, 5, 3, 4]
TERMS = {"x": [1, 3, 6, 2, 1], "y": [1, 2, 1, 4, 1], "z": [1, 5, 3, 3, 1]}


def _train(name):
    return R.rand_train(sum(map(ord, name)), N, TERMS[name])


@pytest.mark.parametrize("names,coefs", [(("x",), [-2.5]), (("x", "y"), [1.0, -1.0]), (("x", "y", "x"), [0.5, 3.0, -0.25]), (("x", "y", "z"), [1e3, -1e-3, 7.0])])
def test_lincomb_reference_expands_to_the_sum_of_the_dense_tensors(names, coefs):
    trains = [_train(nm) for nm in names]
    new = A.lincomb_cores(coefs, trains)
    assert A.ranks(new) == A.lincomb_ranks(trains) == [1] + [sum(TERMS[nm][k] for nm in names) for k in range(1, 4)] + [1]
    assert [c.shape[1] for c in new] == N
    want = sum(np.float64(c) * A.dense(x) for c, x in zip(coefs, trains))
    bound = 2.0 * A.n_lincomb(new, len(names)) * A.U * A.dense(A.lincomb_abs(coefs, trains))
    got = A.dense(new)
    assert got.shape == want.shape == tuple(N) and np.all(bound > 0)
    print(names, "max |diff| / bound", float(np.max(np.abs(got - want) / bound)))
    assert np.all(np.abs(got - want) <= bound)


def test_lincomb_reference_layout():
    x, y = _train("x"), _train("y")
    new = A.lincomb_cores([2.0, -3.0], [x, y])
    assert np.array_equal(new[0][:, :, :3], 2.0 * x[0]) and np.array_equal(new[0][:, :, 3:], -3.0 * y[0])
    assert np.array_equal(new[1][:3, :, :6], x[1]) and np.array_equal(new[1][3:, :, 6:], y[1])
    assert not new[1][:3, :, 6:].any() and not new[1][3:, :, :6].any()
    assert np.array_equal(new[3][:2], x[3]) and np.array_equal(new[3][2:], y[3])
    one = A.lincomb_cores([1.0], [x])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, x))


@pytest.mark.parametrize("names", [("x", "y"), ("y", "x"), ("x", "x"), ("z", "y")])
def test_hadamard_reference_expands_to_the_product_of_the_dense_tensors(names):
    x, y = _train(names[0]), _train(names[1])
    new = A.hadamard_cores(x, y)
    assert A.ranks(new) == A.hadamard_ranks(x, y) == [a * b for a, b in zip(TERMS[names[0]], TERMS[names[1]])]
    want = A.dense(x) * A.dense(y)
    bound = 2.0 * A.n_hadamard(new) * A.U * A.dense(A.hadamard_abs(x, y))
    got = A.dense(new)
    print(names, "max |diff| / bound", float(np.max(np.abs(got - want) / bound)))
    assert got.shape == want.shape and np.all(np.abs(got - want) <= bound)
    # the x index runs fastest on both bonds
    k, j = 1, 3
    rx0, rx1 = x[k].shape[0], x[k].shape[2]
    ia, ka, ib, kb = rx0 - 1, rx1 - 1, y[k].shape[0] - 1, y[k].shape[2] - 1
    assert new[k][ib * rx0 + ia, j, kb * rx1 + ka] == x[k][ia, j, ka] * y[k][ib, j, kb]


def test_header_declares_the_three_prototypes():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        h = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))
    assert "int ttx_lincomb(int32_t m, const double *coef , ttx_engine *const *x , ttx_engine **out);" in h
    assert "int ttx_hadamard(ttx_engine *x, ttx_engine *y, ttx_engine **out);" in h
    assert "int ttx_algebra_last(const ttx_engine *h, double *ms, double *bytes_read, double *bytes_written);" in h


def _lib():
    import __graft_entry__ as g
    return ctypes.CDLL(g.build_lib())


def test_library_exports_the_three_symbols_and_keeps_version_3():
    L = _lib()
    for sym in ("ttx_lincomb", "ttx_hadamard", "ttx_algebra_last"):
        assert hasattr(L, sym), sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() == 3


def test_refusals_that_need_no_device():
    """null pointers and m < 1 are answered before any device call, with *out NULL"""
    L = _lib()
    L.ttx_last_error.restype = ctypes.c_char_p
    vp, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
    L.ttx_lincomb.argtypes = [ctypes.c_int32, dp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    L.ttx_hadamard.argtypes = [vp, vp, ctypes.POINTER(vp)]
    L.ttx_algebra_last.argtypes = [vp, dp, dp, dp]
    coef = (ctypes.c_double * 2)(1.0, -1.0)
    hs = (vp * 2)(None, None)
    out = vp(12345)
    fake = vp(8)                                                       # never dereferenced: the null operand is refused first
    for m, c, x in ((2, None, hs), (2, coef, None), (0, coef, hs), (-3, coef, hs), (2, coef, hs)):
        out.value = 12345
        assert L.ttx_lincomb(m, c, x, ctypes.byref(out)) == EINVAL and not out.value, (m, c, x)
        assert b"ttx_lincomb" in L.ttx_last_error()
    assert L.ttx_lincomb(2, coef, hs, None) == EINVAL
    for x, y in ((None, None), (None, fake), (fake, None)):
        out.value = 12345
        assert L.ttx_hadamard(x, y, ctypes.byref(out)) == EINVAL and not out.value
        assert b"ttx_hadamard" in L.ttx_last_error()
    assert L.ttx_hadamard(None, None, None) == EINVAL
    v = ctypes.c_double()
    assert L.ttx_algebra_last(None, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v)) == EINVAL


def test_engine_class_has_the_methods_and_no_operators():
    from ttcross_amd import engine as E
    for name in ("lincomb", "axpby", "hadamard", "dist", "wdot", "algebra_last"):
        assert callable(getattr(E.TTCross, name)), name
    for op in ("__add__", "__sub__", "__mul__", "__rmul__", "__neg__"):
        assert not hasattr(E.TTCross, op), op
