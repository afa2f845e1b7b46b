"""Batched element evaluation (ttx_ijk_batch, ttx_ijk_batch_dev, ttx_value_batch): what can be checked without a GPU -- the
C-ABI as declared and as exported, and the host restatement of dtt_value's index digits (lib/tt.f90:702-728)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_header_declares_the_batch_entry_points():
    h = re.sub(r"\s+", " ", _header())
    assert "int ttx_ijk_batch(ttx_engine *h, int64_t npts, const int32_t *ind , double *out , int32_t mode);" in h
    assert "int ttx_ijk_batch_dev(ttx_engine *h, int64_t npts, const int32_t *ind_dev, double *out_dev, int32_t mode);" in h
    assert "int ttx_value_batch(ttx_engine *h, int64_t npts, int32_t dd, const double *x , double *out, int32_t mode);" in h
    for name, val in (("TTX_EVAL_EXACT", 0), ("TTX_EVAL_MFMA", 1), ("TTX_EVAL_AUTO", 2)):
        assert re.search(rf"#define {name} {val}\b", h), name


def test_library_exports_the_batch_entry_points_and_version_3():
    import __graft_entry__ as g
    L = ctypes.CDLL(g.build_lib())
    for sym in ("ttx_ijk_batch", "ttx_ijk_batch_dev", "ttx_value_batch", "ttx_eval_last_mode"):
        assert hasattr(L, sym), sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() == 3


def test_engine_module_mirrors_the_mode_constants():
    from ttcross_amd import engine as E
    assert (E.TTX_EVAL_EXACT, E.TTX_EVAL_MFMA, E.TTX_EVAL_AUTO) == (0, 1, 2)
    assert E.EVAL_MODES == {"exact": 0, "mfma": 1, "auto": 2}
    assert callable(E.TTCross.tijk_batch) and callable(E.TTCross.value_batch)


def _value_indices_loop(n, x):
    """dtt_value's digit loop, one point at a time, as the reference writes it (1-based positions kept)"""
    d, dd = len(n), len(x)
    ind = [0] * d
    mm = d // dd
    for idx in range(1, dd + 1):
        xx = float(x[idx - 1])
        if xx < 0.0:
            return None
        if xx > 1.0:
            xx = xx - int(xx)
        for j in range(1, mm + 1):
            pos = 1 + (idx - 1) * mm + mm - j
            i = int(n[pos - 1] * xx)
            if i == n[pos - 1]:
                i = n[pos - 1] - 1
            ind[pos - 1] = i + 1
            xx = xx * n[pos - 1] - i
    return ind


def test_value_indices_hand_cases():
    from ttcross_amd.engine import value_indices
    n = [4, 4, 4, 4, 4, 4]
    ind, neg = value_indices(n, [[0.0, 0.0]])
    assert ind.dtype == np.int32 and ind.tolist() == [[1] * 6] and neg.tolist() == [False]
    ind, neg = value_indices(n, [[1.0, 1.0]])                       # x = 1: the last index in every digit
    assert ind.tolist() == [[4] * 6] and not neg[0]
    a, _ = value_indices(n, [[1.25, 3.25]])                         # x > 1: the digits of the fractional part
    b, _ = value_indices(n, [[0.25, 0.25]])
    assert a.tolist() == b.tolist() == [[1, 1, 2, 1, 1, 2]]         # 0.25 = 0.100 in base 4, most significant digit in the LAST mode of a group
    ind, neg = value_indices(n, [[0.5, -1e-300], [0.5, 0.5]])       # x < 0 is flagged, the other point untouched
    assert neg.tolist() == [True, False] and ind[1].tolist() == [1, 1, 3, 1, 1, 3]
    ind, neg = value_indices([3, 3, 3, 3, 3], [[0.5, 0.5]])         # d = 5, dd = 2: mm = 2, the fifth mode gets no digit
    assert ind.tolist() == [[2, 2, 2, 2, 0]]
    ind, neg = value_indices([3, 3], [[0.5, 0.5, 0.5]])             # dd > d: mm = 0, no digit at all
    assert ind.tolist() == [[0, 0]]
    ind, neg = value_indices([2, 3, 5, 7], [[0.7, 0.3]])            # unequal mode sizes
    assert ind.tolist() == [_value_indices_loop([2, 3, 5, 7], [0.7, 0.3])] == [[1, 3, 1, 3]]
    with pytest.raises(ValueError):
        value_indices(n, [[float("nan"), 0.0]])


@pytest.mark.parametrize("n,dd", [([5] * 12, 3), ([2, 3, 5, 7, 11, 13, 4], 2), ([101] * 9, 9), ([7] * 10, 1), ([3, 4, 5], 4)])
def test_value_indices_random_against_the_loop(n, dd):
    from ttcross_amd.engine import value_indices
    rng = np.random.default_rng(len(n) * 100 + dd)
    x = rng.uniform(-0.05, 1.6, (1000, dd))
    x[::37] = rng.integers(0, 3, (x[::37].shape[0], dd)).astype(float)        # exact 0, 1, 2
    x[5::53] = rng.integers(0, 5, (x[5::53].shape[0], dd)) / 4.0
    ind, neg = value_indices(n, x)
    for p in range(x.shape[0]):
        want = _value_indices_loop(n, x[p])
        if want is None:
            assert neg[p] and not ind[p].any()
        else:
            assert not neg[p] and ind[p].tolist() == want, (p, x[p])
