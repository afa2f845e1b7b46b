"""Partial contraction on the device: ttx_contract / ttx_marginals (ttcross_amd/csrc/ttx_contract.h).

The checker is tests/contract_ref.py (numpy float64).  The tolerance is derived, not measured: an element of the contracted
train is a product of d matrices whose entries are, for a contracted mode, sums of n_k products; for every order of the sums
and products |computed - true| <= N u B with u = 2^-53, N = sum_(k=0..d) (r_k + 1) + sum_(contracted k) (n_k + 1) and B the
same quantity on |cores| and |w|.  Device against reference is therefore <= 2 N u B per element, and equal where B = 0.
Device elements are read with tijk_batch(..., "exact"): its chain over the kept cores is part of the d products counted in N."""
import ctypes
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import contract_ref as C
import tt_ref as R
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

NPTS = 2000
U = C.U


def _cores(tt):
    return [tt.core(k) for k in range(1, tt.d + 1)]


def _points(n, seed, npts=NPTS):
    """npts random multi-indices (1-based), or every multi-index when there are fewer"""
    n = np.asarray(n, dtype=np.int64)
    if float(np.prod(n.astype(np.float64))) <= npts:
        return np.ascontiguousarray(np.array(list(itertools.product(*[range(1, int(k) + 1) for k in n])), dtype=np.int32))
    rng = np.random.default_rng(seed)
    ind = (rng.integers(0, 2 ** 31 - 1, (npts - 2, n.size)) % n + 1).astype(np.int32)
    return np.ascontiguousarray(np.vstack([ind, np.ones((1, n.size), np.int32), n[None, :].astype(np.int32)]))


def _weights(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(int(k)) for k in n]                    # mixed sign


def _keep(d, kept1):
    """keep flags from 1-based kept modes"""
    return [int(k + 1 in kept1) for k in range(d)]


def _chain(d, r):
    return [1] + [r] * (d - 1) + [1]


def _check_elements(tag, got, want, bound):
    """every point: |got - want| <= bound, equal where the bound is 0"""
    diff = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf))
    print(tag, "points", got.size, "max |diff| / bound", float(ratio.max()))
    assert np.all(np.isfinite(got)) and np.all(diff <= bound)
    assert np.array_equal(got[bound == 0], want[bound == 0])


def _check_contract(tag, tt, cores, keep, w, seed=3):
    ct = tt.contract(keep, w)
    ref = C.contract_cores(cores, keep, w)
    assert ct.ranks().tolist() == C.stated_ranks(cores, keep) == C.ranks(ref)
    assert ct._n.tolist() == [c.shape[1] for c in ref]
    ind = _points(ct._n, seed)
    bound = 2.0 * C.count(cores, keep) * U * C.elements(C.abs_bound(cores, keep, w), ind)
    _check_elements(tag, ct.tijk_batch(ind, "exact"), C.elements(ref, ind), bound)
    return ct


def _check_marginals(tag, tt, cores, w):
    got = tt.marginals(w)
    want, ab = C.marginals(cores, w), C.marginals_abs(cores, w)
    d = len(cores)
    assert len(got) == d
    for k in range(d):
        assert got[k].shape == (cores[k].shape[1],)
        _check_elements(f"{tag} marginal {k + 1}", got[k], want[k], 2.0 * C.count(cores, [int(j == k) for j in range(d)]) * U * ab[k])
    return got


CASES = {
    "d3": ([5, 7, 4], [1, 3, 2, 1], [(1, 2), (1, 3), (2, 3)]),
    "d6_modes_of_size_1_rank_1_bond": ([4, 1, 6, 1, 5, 3], [1, 3, 5, 1, 4, 2, 1],
                                       [(3, 4, 5, 6), (1, 2, 3, 4), (1, 2, 4, 5, 6), (1, 2, 5, 6), (3, 4), (1, 6)]),
    "d8_unequal_ranks": ([3, 5, 2, 7, 4, 6, 3, 5], [1, 3, 17, 64, 65, 9, 128, 2, 1], [(1, 8), (4, 5), (2, 7), (3, 6)]),
    "d63_r32": ([3] * 63, _chain(63, 32), [(1, 63), (31, 32), (10, 50), tuple(range(8, 63, 8))]),
    "d5_r128": ([4] * 5, _chain(5, 128), [(3, 4), (1, 5)]),
    "d6_r65": ([5] * 6, _chain(6, 65), [(3, 4), (1, 6)]),
}
_cache = {}


def _case(name):
    """the source train of a case, uploaded once and never changed (test_nothing_else_moves checks that contract changes nothing)"""
    if name not in _cache:
        n, r, _ = CASES[name]
        cores = R.rand_train(sum(map(ord, name)), n, r)
        _cache[name] = (E.TTCross.from_cores(cores), cores, _weights(n, len(name)))
    return _cache[name]


@pytest.mark.parametrize("name,kept", [(nm, kp) for nm in CASES for kp in CASES[nm][2]], ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else v)
def test_contract_against_the_reference(name, kept):
    tt, cores, w = _case(name)
    _check_contract(f"{name} kept {kept}", tt, cores, _keep(tt.d, kept), w)


def test_keep_all_is_a_bit_identical_copy():
    tt, cores, w = _case("d3")
    ct = tt.contract([1, 1, 1], w)
    assert ct.ranks().tolist() == tt.ranks().tolist()
    for a, b in zip(_cores(ct), cores):
        assert a.tobytes() == b.tobytes()
    tt8, cores8, w8 = _case("d8_unequal_ranks")
    for a, b in zip(_cores(tt8.contract([True] * 8)), cores8):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["d3", "d6_modes_of_size_1_rank_1_bond", "d8_unequal_ranks"])
def test_no_weights_are_weights_of_ones_bit_for_bit(name):
    tt, cores, _ = _case(name)
    ones = [np.ones(c.shape[1]) for c in cores]
    for kept in CASES[name][2]:
        keep = _keep(tt.d, kept)
        for a, b in zip(_cores(tt.contract(keep)), _cores(tt.contract(keep, ones))):
            assert a.tobytes() == b.tobytes()
    for a, b in zip(tt.marginals(), tt.marginals(ones)):
        assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", ["d3", "d6_modes_of_size_1_rank_1_bond", "d8_unequal_ranks", "d63_r32"])
def test_quad_of_the_contracted_train_is_quad_of_the_source(name):
    tt, cores, w = _case(name)
    full = tt.quad(w)
    absq = R.quad([np.abs(c) for c in cores], [np.abs(q) for q in w])
    for kept in CASES[name][2]:
        keep = _keep(tt.d, kept)
        part = tt.contract(keep, w).quad([w[k - 1] for k in kept])
        bound = 2.0 * (C.count(cores, [0] * tt.d)) * U * absq
        print(name, kept, "|quad - quad| / bound", abs(part - full) / bound)
        assert abs(part - full) <= bound


@pytest.mark.parametrize("name", ["d3", "d6_modes_of_size_1_rank_1_bond", "d8_unequal_ranks", "d63_r32"])
def test_slices_are_elements_of_the_source(name):
    """unit vectors as weights: the contracted train is the source with those indices fixed"""
    tt, cores, _ = _case(name)
    n = [c.shape[1] for c in cores]
    rng = np.random.default_rng(len(name))
    for kept in CASES[name][2]:
        keep = _keep(tt.d, kept)
        fix = [int(rng.integers(1, nk + 1)) for nk in n]
        w = [np.eye(nk)[j - 1] for nk, j in zip(n, fix)]
        ct = tt.contract(keep, w)
        ind = _points(ct._n, 11, 500)
        src = np.tile(np.array(fix, np.int32), (ind.shape[0], 1))
        src[:, [k - 1 for k in kept]] = ind
        bound = 2.0 * C.count(cores, keep) * U * C.elements(C.abs_bound(cores, keep, w), ind)
        _check_elements(f"{name} slice kept {kept}", ct.tijk_batch(ind, "exact"), tt.tijk_batch(np.ascontiguousarray(src), "exact"), bound)


@pytest.mark.parametrize("name", ["d2", "d3", "d6_modes_of_size_1_rank_1_bond", "d63_r32"])
def test_marginals_against_the_reference_and_quad(name):
    if name == "d2":
        cores = R.rand_train(22, [5, 7], [1, 3, 1])
        tt, w = E.TTCross.from_cores(cores), _weights([5, 7], 2)
    else:
        tt, cores, w = _case(name)
    for ww in (w, None):
        got = _check_marginals(name, tt, cores, ww)
        wv = ww if ww is not None else [np.ones(c.shape[1]) for c in cores]
        full = tt.quad(ww)
        bound = 2.0 * C.count(cores, [0] * tt.d) * U * R.quad([np.abs(c) for c in cores], [np.abs(q) for q in wv])
        for k in range(tt.d):
            assert abs(float(np.dot(wv[k], got[k])) - full) <= bound, k


def _sweep_ising_c():
    s = D.ising_setup("c", 6, 33)
    return s, E.TTCross(s["n"], s["fun_id"], s["par"], 12, pivoting=2, accuracy=s["acc"], quad=s["quad"], tru=s["tru"]).run()


def test_a_sweeps_train_with_its_own_quadrature_weights():
    s, tt = _sweep_ising_c()
    cores = _cores(tt)
    w = [np.asarray(q, dtype=np.float64) for q in s["quad"]]
    _check_marginals("ising_c", tt, cores, w)
    _check_contract("ising_c kept (2, 4)", tt, cores, _keep(tt.d, (2, 4)), w)


def test_downstream_use_of_the_contracted_train(tmp_path):
    tt, cores, w = _case("d63_r32")
    kept = tuple(range(8, 63, 8))
    keep = _keep(tt.d, kept)
    wk = [w[k - 1] for k in kept]
    ct = tt.contract(keep, w)
    q0 = ct.quad(wk)
    nrm = ct.norm()
    assert np.isfinite(nrm) and nrm > 0
    p = os.path.join(str(tmp_path), "c.tt")
    ct.write(p)
    back = E.TTCross.read(p)
    assert back.ranks().tolist() == ct.ranks().tolist()
    for a, b in zip(_cores(back), _cores(ct)):
        assert a.tobytes() == b.tobytes()
    ct.svd(1e-8)
    assert abs(ct.norm() - nrm) <= 1e-6 * nrm
    assert abs(ct.quad(wk) - q0) <= 1e-6 * nrm * float(np.prod([np.linalg.norm(q) for q in wk]))      # Cauchy-Schwarz on the rounding error
    # and the contracted train can be contracted again
    again = ct.contract([1, 0, 0, 1, 0, 0, 1], wk)
    assert again.d == 3 and np.isfinite(again.quad([wk[0], wk[3], wk[6]]))


def test_two_calls_give_the_same_bytes():
    for name in ("d8_unequal_ranks", "d63_r32", "d5_r128"):
        tt, cores, w = _case(name)
        for kept in CASES[name][2]:
            keep = _keep(tt.d, kept)
            a, b = tt.contract(keep, w), tt.contract(keep, w)
            assert [c.tobytes() for c in _cores(a)] == [c.tobytes() for c in _cores(b)]
        assert [m.tobytes() for m in tt.marginals(w)] == [m.tobytes() for m in tt.marginals(w)]


def test_nothing_else_moves():
    s, tt = _sweep_ising_c()
    w = [np.asarray(q, dtype=np.float64) for q in s["quad"]]
    ind = _points(tt._n, 5, 50)

    def state():
        return tt.ranks().tobytes(), [c.tobytes() for c in _cores(tt)], tt.quad(s["quad"]), tt.norm(), tt.tijk(ind[3]), tt.tijk_batch(ind, "exact").tobytes()

    before = state()
    tt.contract([0, 1, 0, 1, 0], w)
    assert state() == before
    tt.marginals(w)
    assert state() == before
    tt.contract([1] * tt.d)
    tt.marginals()
    assert state() == before


def test_argument_errors():
    L = E.load_library()
    EINVAL, ESTATE = 1, 4
    tt = E.TTCross.from_cores(R.rand_train(2, [3, 3, 3], [1, 2, 2, 1]))
    out = ctypes.c_void_p(12345)
    marg = np.zeros(9)
    nul_i, nul_d = ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_double)()

    def contract(h, keep):
        out.value = 12345
        k = np.asarray(keep, dtype=np.int32)
        rc = L.ttx_contract(h, E._ip(k), None, ctypes.byref(out))
        assert rc != 0 and not out.value                              # *out is null after a refusal
        return rc

    out.value = 12345
    assert L.ttx_contract(tt._h, nul_i, None, ctypes.byref(out)) == EINVAL and not out.value
    assert L.ttx_contract(tt._h, E._ip(np.ones(3, np.int32)), None, None) == EINVAL
    assert L.ttx_marginals(tt._h, None, nul_d) == EINVAL
    assert contract(tt._h, [1, 2, 1]) == EINVAL
    assert contract(tt._h, [1, -1, 1]) == EINVAL
    assert contract(tt._h, [0, 1, 0]) == EINVAL
    assert "ttx_marginals" in L.ttx_last_error().decode() and "ttx_quad" in L.ttx_last_error().decode()
    assert contract(tt._h, [0, 0, 0]) == EINVAL
    with pytest.raises(E.TTXError):
        tt.contract([1, 0, 0])
    with pytest.raises(ValueError):
        tt.contract([1, 1])
    with pytest.raises(ValueError):
        tt.contract([1, 1, 0], [np.ones(3)] * 2)
    # an engine that has not run
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    assert contract(fresh._h, [1, 1, 0, 0, 0]) == ESTATE
    assert L.ttx_marginals(fresh._h, None, E._dp(np.zeros(45))) == ESTATE
    # the two-process engine of the tijk test: whatever ttx_ijk answers
    mp = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"], nproc=2, world_rank=0, world_size=2)
    i5, v = np.ones((1, 5), np.int32), ctypes.c_double()
    want = L.ttx_ijk(mp._h, E._ip(i5), ctypes.byref(v))
    assert want != 0
    assert contract(mp._h, [1, 1, 0, 0, 0]) == want
    assert L.ttx_marginals(mp._h, None, E._dp(np.zeros(45))) == want
    # the engine is still good
    assert L.ttx_marginals(tt._h, None, E._dp(marg)) == 0 and np.all(np.isfinite(marg))


@pytest.mark.parametrize("name,kept", [("d63_r32", (10, 50)), ("d63_r32", tuple(range(8, 63, 8))), ("d8_unequal_ranks", (3, 6)), ("d5_r128", (3, 4)), ("d6_r65", (1, 6))],
                         ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else v)
def test_sharp_bound_on_non_negative_trains(name, kept):
    """cores >= 0 and weights >= 0: B equals the value, so the same bound is a relative tolerance 2 N u of about 1e-12 -- on the
    mixed-sign trains above B exceeds the values by many orders where the train is long"""
    n, r, _ = CASES[name]
    rng = np.random.default_rng(len(name) + len(kept))
    cores = [rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1])) / (0.5 * r[k + 1]) for k in range(len(n))]
    w = [rng.uniform(0.0, 1.0, nk) for nk in n]
    tt = E.TTCross.from_cores(cores)
    keep = _keep(tt.d, kept)
    ct = tt.contract(keep, w)
    ind = _points(ct._n, 5)
    want = C.elements(C.contract_cores(cores, keep, w), ind)
    tol = 2.0 * C.count(cores, keep) * U
    got = ct.tijk_batch(ind, "exact")
    print(name, kept, "relative tolerance", tol, "max relative difference", float(np.max(np.abs(got - want) / want)))
    assert np.all(want > 0) and np.all(np.abs(got - want) <= tol * want)
    mg, mw = tt.marginals(w), C.marginals(cores, w)
    for k in range(tt.d):
        assert np.all(np.abs(mg[k] - mw[k]) <= 2.0 * C.count(cores, [int(j == k) for j in range(tt.d)]) * U * mw[k]), k


def test_fortran_contract_and_marginals_equal_the_programs_own_loops():
    """the drop-in tt_lib: contract(tt, keep, res, w) and marginals(tt, marg, w) against sums the program forms itself over
    tijk(tt, ind); ranks by the stated rule; 1e-12 of the element scale, the tolerance of the Fortran tijk test"""
    import subprocess
    from conftest import fortran_exe
    exe = fortran_exe("test_contract")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("done"), p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.split()]
    ranks = [ln for ln in lines if ln[0] == "ranks"]
    assert ranks == [["ranks", "m", "3", "r", "1", "3", "3", "1", "n", "5", "6", "4"]]    # r' = (1, r(2), r(4), 1), modes 2, 4 and 5 kept
    el = np.array([[float(x) for x in ln[2:]] for ln in lines if ln[0] == "elem"])
    assert el.shape == (40, 2)
    scale = np.abs(el[:, 1]).max()
    assert scale > 0.1 and len(set(el[:, 1])) > 30
    assert np.all(np.abs(el[:, 0] - el[:, 1]) <= 1e-12 * scale)
    mg = np.array([[float(x) for x in ln[3:]] for ln in lines if ln[0] == "marg"])
    assert mg.shape == (3 + 6 + 2 + 4, 2)
    scale = np.abs(mg[:, 1]).max()
    assert scale > 0.1 and np.all(np.abs(mg[:, 0] - mg[:, 1]) <= 1e-12 * scale)
