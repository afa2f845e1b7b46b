"""Matrices applied to chosen modes on the device: ttx_mode_apply (ttcross_amd/csrc/ttx_modeapply.h).

The checker is tests/modeapply_ref.py (numpy float64).  TTX_EVAL_EXACT is compared bit for bit.  The tolerance of TTX_EVAL_MFMA is
derived, not measured: any order of the n_k products and sums of one element, fused or not, stays within (n_k + 1) u S of the
true value, S = sum_i |A_k(j, i)| |G_k(a, i, b)|, u = 2^-53, and the reference does too: |got - ref| <= 2 (n_k + 1) u S, equal
where S = 0.  Elements read through tijk_batch / quad carry the counting of contract_ref: 2 N u B with
N = sum_k (r_k + 1) + sum_applied (n_k + 1) and B the same quantity on absolute values."""
import ctypes
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import contract_ref as C
import modeapply_ref as M
import tt_ref as R
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

U = M.U
MODES = ("exact", "mfma")
# name: (n, ranks, m with 0 = untouched)
CASES = {
    "d3": ([5, 7, 4], [1, 3, 2, 1], [6, 0, 9]),
    "kmod": ([1, 2, 3, 6], [1, 4, 4, 4, 1], [3, 1, 17, 2]),
    "tiles": ([9, 33, 10], [1, 17, 65, 1], [15, 65, 16]),
    "r128": ([4, 5, 4, 5], [1, 128, 128, 128, 1], [7, 3, 0, 130]),
    "longk": ([1030, 6], [1, 3, 1], [5, 2000]),
    "d40": ([3] * 40, [1] + [8] * 39 + [1], [4 if k % 2 == 0 else 0 for k in range(40)]),     # the odd modes, counted from 1
}
_cache, _results = {}, {}


def _cores(tt):
    return [tt.core(k) for k in range(1, tt.d + 1)]


def _case(name):
    """source engine, its cores, the matrices, the reference cores and the S of the bound: made once and never changed"""
    if name not in _cache:
        n, r, m = CASES[name]
        cores = R.rand_train(sum(map(ord, name)), n, r)
        rng = np.random.default_rng(len(name))
        mats = [rng.standard_normal((mk, nk)) if mk else None for mk, nk in zip(m, n)]        # mixed sign
        _cache[name] = (E.TTCross.from_cores(cores), cores, mats, M.apply_cores(cores, mats), M.abs_cores(cores, mats))
    return _cache[name]


def _result(name, mode):
    if (name, mode) not in _results:
        tt, _, mats, _, _ = _case(name)
        new = tt.mode_apply(mats, mode)
        _results[name, mode] = (new, _cores(new), tt.mode_apply_last())
    return _results[name, mode]


def _check_cores(tag, got, ref, S, mats, n, mode):
    worst = 0.0
    for k, (g, w) in enumerate(zip(got, ref)):
        assert g.shape == w.shape
        if mode == "exact" or mats[k] is None:
            assert g.tobytes() == w.tobytes(), (tag, k + 1)
            continue
        diff, bound = np.abs(g - w), 2.0 * (n[k] + 1) * U * S[k]
        with np.errstate(divide="ignore", invalid="ignore"):
            worst = max(worst, float(np.max(np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf)))))
        assert np.all(diff <= bound), (tag, k + 1)
        assert np.array_equal(g[S[k] == 0], w[S[k] == 0])
    print(tag, mode, "largest |got - ref| / bound", worst)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_cores_against_the_reference(name, mode):
    n, r, m = CASES[name]
    tt, cores, mats, ref, S = _case(name)
    new, got, last = _result(name, mode)
    assert new.ranks().tolist() == tt.ranks().tolist() == r
    assert new._n.tolist() == [mk or nk for mk, nk in zip(m, n)]
    assert last["mode"] == mode
    _check_cores(name, got, ref, S, mats, n, mode)
    for k in range(len(n)):                                             # untouched cores: the source's bits
        if mats[k] is None:
            assert got[k].tobytes() == cores[k].tobytes()


@pytest.mark.parametrize("name", ["d3", "r128", "d40"])
def test_all_zero_m_is_a_bit_identical_deep_copy(name):
    tt, cores, _, _, _ = _case(name)
    for mode in MODES + ("auto",):
        new = tt.mode_apply([None] * tt.d, mode)
        assert new.ranks().tolist() == tt.ranks().tolist() and new._n.tolist() == tt._n.tolist()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_cores(new), cores))
        last = tt.mode_apply_last()
        assert last["ms"] == 0.0 and last["bytes_read"] == 0.0 and last["bytes_written"] == 0.0 and last["flops"] == 0.0
        new.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_cores(tt.mode_apply({})), cores))


def _abs_quad(cores, w):
    v = np.ones((1, 1))
    for c, q in zip(cores, w):
        v = v @ np.einsum("ajb,j->ab", np.abs(c), np.abs(q))
    return float(v[0, 0])


@pytest.mark.parametrize("name", ["tiles", "d3"])
def test_elements_against_quad_of_the_source(name):
    """new(j) = sum_i prod_k A_k(j_k, i_k) source(i): the quadrature of the source with the matrix rows as weights"""
    n, r, m = CASES[name]
    tt, cores, mats, _, _ = _case(name)
    new = _result(name, "exact")[0]
    rng = np.random.default_rng(7)
    ind = np.ascontiguousarray(np.stack([rng.integers(1, int(nk) + 1, 200) for nk in new._n], axis=1).astype(np.int32))
    got = new.tijk_batch(ind, "exact")
    N = M.count(cores, mats)
    worst = 0.0
    for row, g in zip(ind, got):
        w = [mats[k][row[k] - 1, :] if mats[k] is not None else np.eye(n[k])[row[k] - 1] for k in range(len(n))]
        want, bound = tt.quad(w), 2.0 * N * U * _abs_quad(cores, w)
        assert bound > 0 and abs(g - want) <= bound, (row, g, want, bound)
        worst = max(worst, abs(g - want) / bound)
    print(name, "200 elements against quad: largest |diff| / bound", worst)


def test_contract_of_an_applied_mode_is_contract_with_the_column_sums():
    tt, cores, mats, _, _ = _case("d3")
    A = mats[0]
    new = tt.mode_apply({1: A}, "exact")
    keep = [0, 1, 1]
    w = [np.ones(A.shape[0]), np.ones(7), np.ones(4)]
    ws = [A.T @ np.ones(A.shape[0]), np.ones(7), np.ones(4)]
    a, b = new.contract(keep, w), tt.contract(keep, ws)
    assert a.ranks().tolist() == b.ranks().tolist() and a._n.tolist() == b._n.tolist() == [7, 4]
    ind = np.ascontiguousarray(np.array([[i, j] for i in range(1, 8) for j in range(1, 5)], dtype=np.int32))
    N = C.count(cores, keep) + A.shape[0] + 1                           # the sum over the m_1 new indices on top of contract's count
    bound = 2.0 * N * U * C.elements(C.abs_bound(cores, keep, [np.abs(A).T @ np.ones(A.shape[0]), ws[1], ws[2]]), ind)
    got, want = a.tijk_batch(ind, "exact"), b.tijk_batch(ind, "exact")
    print("contract after apply: largest |diff| / bound", float(np.max(np.abs(got - want) / bound)))
    assert np.all(bound > 0) and np.all(np.abs(got - want) <= bound)


@pytest.mark.parametrize("name", ["d3", "tiles", "longk"])
def test_a_call_repeats_bit_for_bit_and_leaves_the_source_alone(name):
    tt, cores, mats, _, _ = _case(name)
    rng = np.random.default_rng(11)
    ind = np.ascontiguousarray(np.stack([rng.integers(1, int(nk) + 1, 50) for nk in tt._n], axis=1).astype(np.int32))
    keep = [1] * (tt.d - 1) + [0] if tt.d > 2 else None
    before = tt.tijk_batch(ind, "exact")
    ct_before = _cores(tt.contract(keep)) if keep else None
    for mode in MODES:
        first = _result(name, mode)[1]
        again = tt.mode_apply(mats, mode)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, _cores(again)))
        again.close()
        assert tt.ranks().tolist() == CASES[name][1]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(_cores(tt), cores))
        assert tt.tijk_batch(ind, "exact").tobytes() == before.tobytes()
        if keep:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(_cores(tt.contract(keep)), ct_before))


@pytest.mark.parametrize("mode", MODES)
def test_device_matrices_give_the_bits_of_the_host_entry(mode):
    """torch tensors by data_ptr() through ttx_mode_apply_dev, in a child process (modeapply_dev_worker.py says why)"""
    import json
    import os
    import sys
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "modeapply_dev_worker.py"), mode],
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["ranks"] == [1, 17, 65, 1] and res["modes"] == [15, 33, 16]
    assert res["equal"] and res["ran"] == mode and res["float32_refused"]


@pytest.mark.parametrize("name", ["d3", "r128", "longk"])
def test_mode_apply_last_reports_the_stated_figures(name):
    n, r, m = CASES[name]
    tt, _, mats, _, _ = _case(name)
    rd = 8.0 * sum(r[k] * n[k] * r[k + 1] + m[k] * n[k] for k in range(len(n)) if m[k])
    wr = 8.0 * sum(r[k] * m[k] * r[k + 1] for k in range(len(n)) if m[k])
    fl = 2.0 * sum(r[k] * r[k + 1] * n[k] * m[k] for k in range(len(n)) if m[k])
    for mode in MODES + ("auto",):
        tt.mode_apply(mats, mode).close()
        last = tt.mode_apply_last()
        assert last["bytes_read"] == rd and last["bytes_written"] == wr and last["flops"] == fl
        assert last["ms"] > 0
        assert last["mode"] == mode if mode != "auto" else last["mode"] in MODES


def _still_works(tt, name):
    new = tt.mode_apply(_case(name)[2], "exact")
    assert all(a.tobytes() == b.tobytes() for a, b in zip(_cores(new), _result(name, "exact")[1]))
    new.close()


def test_refusals():
    tt, _, mats, _, _ = _case("d3")
    with pytest.raises(E.TTXError, match=r"m\(1\) = 32001"):
        tt.mode_apply({1: np.zeros((32001, 5))})
    _still_works(tt, "d3")
    big = _case("r128")[0]
    with pytest.raises(E.TTXError, match=r"m\(2\) = 1025"):
        big.mode_apply({2: np.zeros((1025, 5))})
    _still_works(big, "r128")
    for bad in ([np.zeros((3, 4)), None, None], [None, np.zeros(7), None], [None, None], {4: np.zeros((2, 4))}, [np.zeros((0, 5)), None, None]):
        with pytest.raises(ValueError):
            tt.mode_apply(bad)
    with pytest.raises(ValueError):
        tt.mode_apply(mats, "fast")
    # the C entry with an engine: a negative m(k), an unknown mode, null matrices
    L = E.load_library()
    out = ctypes.c_void_p(12345)
    flat = np.zeros(200)
    for m, A, mode, text in (([2, -1, 0], flat, 0, b"m(2) = -1"), ([2, 0, 0], flat, 3, b"mode 3"), ([2, 0, 0], None, 0, b"null")):
        out.value = 12345
        rc = L.ttx_mode_apply(tt._h, E._ip(np.array(m, dtype=np.int32)), E._dp(A), mode, ctypes.byref(out))
        assert rc == 1 and not out.value and text in L.ttx_last_error(), (m, mode, L.ttx_last_error())
    _still_works(tt, "d3")
    s = D.ising_setup("c", 6, 33)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=1, accuracy=s["acc"], quad=s["quad"], tru=s["tru"])
    with pytest.raises(E.TTXError, match="no tensor train"):
        fresh.mode_apply([np.zeros((2, int(fresh._n[0])))] + [None] * (fresh.d - 1))
    fresh.close()


@pytest.mark.parametrize("mode", MODES)
def test_nan_and_inf_stay_in_their_columns(mode):
    tt, cores, mats, _, _ = _case("d3")
    bad = [None if a is None else a.copy() for a in mats]
    bad[0][2, 3] = np.nan
    bad[2][4, 1] = np.inf
    bad[2][7, 0] = -np.inf
    with np.errstate(invalid="ignore"):
        ref = M.apply_cores(cores, bad)
    new = tt.mode_apply(bad, mode)
    got = _cores(new)
    for k in (0, 2):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])) and np.array_equal(np.isinf(got[k]), np.isinf(ref[k]))
        fin = np.isfinite(ref[k])
        assert np.array_equal(got[k][~fin], ref[k][~fin], equal_nan=True)
    assert np.isnan(got[0][:, 2, :]).all() and np.isfinite(np.delete(got[0], 2, axis=1)).all()
    assert np.isfinite(np.delete(got[2], [4, 7], axis=1)).all() and not np.isfinite(got[2][:, [4, 7], :]).any()
    assert got[1].tobytes() == cores[1].tobytes() and np.isfinite(got[1]).all()
    _still_works(tt, "d3")


def test_cos_coefficients_to_values_on_a_grid():
    s = D.coscoeff_setup(3, 17)
    tt = E.TTCross(s["n"], E.TTX_FUN_COSCOEFF, [], 8, pivoting=1, accuracy=s["acc"], aux=s["aux"]).run()
    cores = _cores(tt)
    xs = np.linspace(D.COS_A, D.COS_B, 9)
    A = D.cos_matrix(xs, 17, D.COS_A, D.COS_B)
    mats = [A] * 3
    ind = np.ascontiguousarray(np.array([[i, j, k] for i in range(1, 10) for j in range(1, 10) for k in range(1, 10)], dtype=np.int32))
    dense = [np.einsum("ji,aib->ajb", A, c) for c in cores]
    want = np.einsum("aib,bjc,ckd->ijk", *dense).reshape(-1)
    B = np.einsum("aib,bjc,ckd->ijk", *M.abs_cores(cores, mats)).reshape(-1)
    bound = 2.0 * M.count(cores, mats) * U * B
    for mode in MODES:
        new = tt.mode_apply(mats, mode)
        assert new._n.tolist() == [9, 9, 9] and new.ranks().tolist() == tt.ranks().tolist()
        got = new.tijk_batch(ind, "exact")
        print("cos values", mode, "largest |diff| / bound", float(np.max(np.abs(got - want) / bound)))
        assert np.all(np.isfinite(got)) and np.all(np.abs(got - want) <= bound)
        mg = new.marginals()
        assert len(mg) == 3 and all(q.shape == (9,) and np.all(np.isfinite(q)) for q in mg)
        new.close()
    tt.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_fortran_modeapply(tmp_path, mode):
    from conftest import fortran_exe
    exe = fortran_exe("test_tt_modeapply")
    n, r = [5, 7, 4, 6], [1, 3, 2, 4, 1]
    cores = R.rand_train(44, n, r)
    tt = E.TTCross.from_cores(cores)
    path = str(tmp_path / "src.tt")
    tt.write(path)
    p = subprocess.run([exe, path, str(mode)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("done"), p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.split()]
    m = [n[0] + 1, 0, n[2] + 1, 0]
    mats = [None if not mk else np.cos((0.3 * np.arange(1, mk + 1))[:, None] * np.arange(1, nk + 1)[None, :] + 0.1 * (k + 1)) - 0.25
            for k, (mk, nk) in enumerate(zip(m, n))]                   # (0.3 j) i + 0.1 k, the program's own order
    new = tt.mode_apply(mats, "exact" if mode == 0 else "mfma")
    assert [ln for ln in lines if ln[0] == "ranks"] == [["ranks"] + [str(x) for x in r]]
    assert [ln for ln in lines if ln[0] == "modes"] == [["modes"] + [str(x) for x in new._n.tolist()]]
    el = np.array([float(ln[2]) for ln in lines if ln[0] == "elem"])
    assert el.shape == (24,)
    ind = np.array([[1 + (p_ * (2 * k + 1) + k) % int(new._n[k - 1]) for k in range(1, 5)] for p_ in range(1, 25)], dtype=np.int32)
    want = new.tijk_batch(ind, "exact")
    # the cos of numpy and of the Fortran runtime may differ by an ulp or two: a matrix entry moves by at most 2 u <= 2 u (|A| + 1),
    # so with two applied modes an element moves by at most 4 u B', B' the element bound with |A| + 1 for |A|; the rounding of the
    # two evaluations, 2 N u B, lies below 2 N u B' as well
    Bnd = C.elements(M.abs_cores(cores, [None if a is None else np.abs(a) + 1.0 for a in mats]), ind)
    print("fortran", mode, "largest |diff| / bound", float(np.max(np.abs(el - want) / ((2.0 * M.count(cores, mats) + 4.0) * U * Bnd))))
    assert np.all(np.abs(el - want) <= (2.0 * M.count(cores, mats) + 4.0) * U * Bnd)
    tt.close()
    new.close()
