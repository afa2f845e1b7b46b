"""Matrices applied to chosen modes (ttx_mode_apply): what can be checked without a GPU -- the numpy reference of
tests/modeapply_ref.py against np.einsum on dense tensors and against contract_ref, drivers.cos_matrix against the COS sum, the C-ABI
as declared and as exported, and the refusals that come before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

import contract_ref as C
import modeapply_ref as M
import tt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = 1
SYMBOLS = ("ttx_mode_apply", "ttx_mode_apply_dev", "ttx_mode_apply_last")


def _dense(cores):
    t, e = R.scaled_dense(cores)
    return np.ldexp(t, e)


@pytest.mark.parametrize("n,r,m", [([4, 3, 5], [1, 3, 2, 1], [6, 0, 2]), ([3, 2, 4, 3], [1, 2, 4, 3, 1], [1, 5, 0, 7]), ([2, 3, 2], [1, 2, 2, 1], [3, 3, 3])])
def test_reference_against_einsum_on_the_dense_tensor(n, r, m):
    d = len(n)
    cores = R.rand_train(d + sum(m), n, r)
    rng = np.random.default_rng(sum(n))
    mats = [rng.standard_normal((mk, nk)) if mk else None for mk, nk in zip(m, n)]
    new = M.apply_cores(cores, mats)
    assert [c.shape for c in new] == [(r[k], m[k] or n[k], r[k + 1]) for k in range(d)]
    ab = M.abs_cores(cores, mats)
    for k in range(d):
        if mats[k] is None:
            assert new[k].tobytes() == cores[k].tobytes()
            continue
        want = np.einsum("ji,aib->ajb", mats[k], cores[k])
        bound = 2.0 * (n[k] + 1) * M.U * ab[k]                          # the core-level bound of modeapply_ref
        print("core", k + 1, "max |diff| / bound", float(np.max(np.abs(new[k] - want) / bound)))
        assert np.all(np.abs(new[k] - want) <= bound)
    # the dense tensor: the train of the new cores against the n-mode products of the dense source
    letters, big = "abcd"[:d], "ABCD"[:d]
    ops, subs, res = [_dense(cores)], [letters], ""
    for k in range(d):
        if mats[k] is None:
            res += letters[k]
        else:
            ops.append(mats[k])
            subs.append(big[k] + letters[k])
            res += big[k]
    want = np.einsum(",".join(subs) + "->" + res, *ops)
    terms = int(np.prod([n[k] for k in range(d) if mats[k] is not None]))
    bound = (3.0 * M.count(cores, mats) + terms) * M.U * _dense(ab)    # reference, dense source and einsum's own sums
    assert np.all(np.abs(_dense(new) - want) <= bound)


def test_one_row_per_mode_is_the_contraction_of_contract_ref():
    n, r = [4, 3, 5, 2], [1, 3, 2, 4, 1]
    cores = R.rand_train(11, n, r)
    rng = np.random.default_rng(5)
    w = [rng.standard_normal(nk) for nk in n]
    for keep in ([1, 0, 0, 1], [0, 1, 1, 0], [1, 0, 1, 0]):
        mats = [None if kp else q[None, :] for kp, q in zip(keep, w)]
        new = M.apply_cores(cores, mats)
        assert [c.shape[1] for c in new] == [nk if kp else 1 for nk, kp in zip(n, keep)]
        got, want = _dense(new).reshape([nk for nk, kp in zip(n, keep) if kp]), _dense(C.contract_cores(cores, keep, w))
        bound = 2.0 * C.count(cores, keep) * C.U * _dense(C.abs_bound(cores, keep, w))
        assert M.count(cores, mats) == C.count(cores, keep)
        assert np.all(np.abs(got - want) <= bound)


def test_cos_matrix_is_the_synthesis_of_cos_approximate():
    from ttcross_amd import drivers as D
    a, b, nt = 0.5, 8.5, 24
    xs = np.linspace(a, b, 13)
    phis = np.exp(-0.5 * (np.arange(nt) * np.pi / (b - a) * 0.7) ** 2) * np.exp(1j * np.arange(nt) * np.pi / (b - a) * 4.0)
    w = np.arange(nt) * (np.pi / (b - a))
    c = 2.0 / (b - a) * np.real(phis * np.exp(-1j * w * a))
    c[0] /= 2.0
    A = D.cos_matrix(xs, nt, a, b)
    assert A.shape == (13, nt) and np.array_equal(A[:, 0], np.ones(13))
    want = D.cos_approximate(xs, phis, a, b)
    assert np.all(np.abs(A @ c - want) <= 2.0 * (nt + 1) * M.U * (np.abs(A) @ np.abs(c)))
    # d = 1 written as a two-core train with a mode of size 1: applying the matrix to the coefficient core gives the density
    cores = [c.reshape(1, nt, 1), np.ones((1, 1, 1))]
    new = M.apply_cores(cores, [A, None])
    assert np.all(np.abs(new[0][0, :, 0] - want) <= 2.0 * (nt + 1) * M.U * (np.abs(A) @ np.abs(c)))


def test_header_declares_the_three_prototypes():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        h = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))
    assert "int ttx_mode_apply (ttx_engine *h, const int32_t *m , const double *A, int32_t mode, ttx_engine **out);" in h
    assert "int ttx_mode_apply_dev(ttx_engine *h, const int32_t *m, const double *A_dev, int32_t mode, ttx_engine **out);" in h
    assert "int ttx_mode_apply_last(const ttx_engine *h, double *ms, double *bytes_read, double *bytes_written, double *flops, int32_t *mode_ran);" in h


def test_library_exports_the_three_symbols_and_keeps_version_3():
    from ttcross_amd import engine as E
    L = E.load_library()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert getattr(L, sym).argtypes
    assert L.ttx_version() == 3
    for name in ("mode_apply", "mode_apply_last"):
        assert callable(getattr(E.TTCross, name)), name


def test_refusals_that_need_no_device():
    """null h, m or out, a negative m(k) and an unknown mode are answered with TTX_EINVAL and a message before any device call, with
    *out NULL.  This machine has no engine to pass (ttx_create needs a device), so the negative m and the unknown mode arrive with
    the null engine; with an engine they are checked in tests/test_gpu_modeapply.py."""
    import __graft_entry__ as g
    L = ctypes.CDLL(g.build_lib())
    L.ttx_last_error.restype = ctypes.c_char_p
    vp, ip, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    for f in (L.ttx_mode_apply, L.ttx_mode_apply_dev):
        f.argtypes = [vp, ip, dp, ctypes.c_int32, ctypes.POINTER(vp)]
    L.ttx_mode_apply_last.argtypes = [vp, dp, dp, dp, dp, ip]
    m, neg = (ctypes.c_int32 * 3)(2, 0, 2), (ctypes.c_int32 * 3)(2, -1, 2)
    A = (ctypes.c_double * 64)()
    out = vp(12345)
    fake = vp(8)                                                        # never dereferenced: the null m and the mode are refused first
    for name in ("ttx_mode_apply", "ttx_mode_apply_dev"):
        f = getattr(L, name)
        for h, mm, mode in ((None, m, 0), (fake, None, 1), (None, neg, 0), (fake, m, 3), (fake, m, -1), (None, m, 7)):
            out.value = 12345
            assert f(h, mm, A, mode, ctypes.byref(out)) == EINVAL and not out.value, (name, h, mode)
            assert name.encode() in L.ttx_last_error()
        assert f(fake, m, A, 0, None) == EINVAL and name.encode() in L.ttx_last_error()
        out.value = 12345
        assert f(fake, m, A, 5, ctypes.byref(out)) == EINVAL and b"mode 5" in L.ttx_last_error()
    assert L.ttx_mode_apply_last(None, None, None, None, None, None) == EINVAL
