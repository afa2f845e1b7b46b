"""A rounded sum of resident trains on the device: ttx_lincomb_round (ttcross_amd/csrc/ttx_roundsum.h).

The checker is tests/roundsum_ref.py (numpy float64): the definition restated with the same Omega, and the allowances derived in
its docstring -- allowance = c(d, n, l) u max_k cond(Z_k) sum_t |c_t| |x_t|_F between the device's train and the reference's as
dense tensors (Frobenius norm), the same without the condition number against the dense sum where the sketch ranks reach the rank
of the sum.  tests/test_roundsum_cpu.py holds two independent numpy evaluations against a quarter of it.  An element differs by
no more than the Frobenius norm of the difference, so "every element within the allowance" is asserted through that norm."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import algebra_ref as A
import roundsum_ref as RS
from ttcross_amd import engine as E

MODES = ["exact", "mfma"]
HERE = os.path.dirname(os.path.abspath(__file__))
_eng = {}


def _up(key, cores):
    """a source train, uploaded once and never changed"""
    if key not in _eng:
        _eng[key] = E.TTCross.from_cores(cores)
    return _eng[key]


def _cores(tt):
    return [tt.core(k) for k in range(1, tt.d + 1)]


def _all_indices(n):
    return np.ascontiguousarray(np.array(list(itertools.product(*[range(1, k + 1) for k in n])), dtype=np.int32))


def _edge(name):
    if name == "d2":
        coefs, _, L, exact = RS.D2
        trains = RS.d2_trains()
        return coefs, trains, [_up(("d2", t), x) for t, x in enumerate(trains)], L, exact
    coefs, names, L, exact = RS.EDGE[name]
    trains = [RS.edge_train(x) for x in names]
    return coefs, trains, [_up(x, RS.edge_train(x)) for x in names], L, exact


_ref = {}


def _reference(key, coefs, trains, L, seed=RS.SKETCH_SEED):
    if key not in _ref:
        _ref[key] = RS.roundsum(coefs, trains, L, seed)
    return _ref[key]


def _check(tag, got, want, allow):
    diff = float(np.linalg.norm(got - want))
    print(tag, "|device - reference|_F", diff, "allowance", allow, "ratio", diff / allow if allow > 0 else np.inf)
    assert np.all(np.isfinite(got)), tag
    assert diff <= allow, (tag, diff, allow)


_today = {}


def _fails_today():
    if not _today:
        coefs, terms = RS.case_fails_today()
        _today.update(coefs=coefs, terms=terms, eng=[_up(("today", t), x) for t, x in enumerate(terms)], dense=RS.dense_sum(coefs, terms),
                      ref=RS.roundsum(coefs, terms, 16, RS.SKETCH_SEED))
    return _today


@pytest.mark.parametrize("mode", MODES)
def test_the_sum_that_lincomb_refuses(mode):
    c = _fails_today()
    L = E.load_library()
    out = ctypes.c_void_p(12345)
    cf = np.ascontiguousarray(c["coefs"], dtype=np.float64)
    hs = (ctypes.c_void_p * 12)(*[t._h for t in c["eng"]])
    assert L.ttx_lincomb(12, E._dp(cf), hs, ctypes.byref(out)) == 1 and not out.value and b"add up to 144" in L.ttx_last_error()
    new = E.TTCross.lincomb_round(c["coefs"], c["eng"], rank=16, seed=RS.SKETCH_SEED, mode=mode)
    assert new.ranks().tolist() == c["ref"]["l"] and max(new.ranks()) <= 16
    allow = RS.allowance(c["coefs"], c["terms"], c["ref"], True)
    got = new.tijk_batch(_all_indices([4] * 6), "exact")
    _check("fails today " + mode, got, c["dense"].reshape(-1), allow)
    assert np.all(np.abs(got - c["dense"].reshape(-1)) <= allow)
    new.close()
    cut = E.TTCross.lincomb_round(c["coefs"], c["eng"], rank=16, tol=1e-12, seed=RS.SKETCH_SEED, mode=mode)
    assert max(cut.ranks()) <= 12, cut.ranks()
    # the truncation at 1e-12 of the norm on top of the allowance
    _check("fails today, tol " + mode, RS.dense(_cores(cut)), c["dense"], allow + 5 ** 0.5 * 1e-12 * float(np.linalg.norm(c["dense"])))
    cut.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(RS.EDGE) + ["d2"])
def test_edge_shapes(name, mode):
    coefs, trains, eng, L, exact = _edge(name)
    ref = _reference(name, coefs, trains, L)
    new = E.TTCross.lincomb_round(coefs, eng, rank=L, seed=RS.SKETCH_SEED, mode=mode)
    assert new.ranks().tolist() == ref["l"], (new.ranks(), ref["l"])
    assert eng[0].roundsum_last()["l"] == ref["l"] and eng[0].roundsum_last()["mode"] == mode
    want = RS.dense_sum(coefs, trains) if exact else RS.dense(ref["cores"])
    _check(f"{name} {mode}", RS.dense(_cores(new)), want, RS.allowance(coefs, trains, ref, exact))
    new.close()


@pytest.mark.parametrize("L", RS.DECAY_RANKS)
def test_truncation_of_a_decaying_sum(L):
    coefs, trains = RS.decay_terms(RS.DECAY_SEED)
    eng = [_up(("decay", t), x) for t, x in enumerate(trains)]
    ref = _reference(("decay", L), coefs, trains, L)
    S = RS.dense_sum(coefs, trains)
    new = E.TTCross.lincomb_round(coefs, eng, rank=L, seed=RS.SKETCH_SEED, mode="mfma")
    got = RS.dense(_cores(new))
    new.close()
    allow = RS.allowance(coefs, trains, ref, False)
    assert allow <= 1e-9 * np.linalg.norm(S)
    _check(f"decay L={L}", got, RS.dense(ref["cores"]), allow)
    err, best = float(np.linalg.norm(got - S)), float(np.linalg.norm(RS.dense(RS.tt_svd(S, ref["l"])) - S))
    print("decay", L, "device error / TT-SVD error", err / best)
    assert err <= 10.0 * best


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["ranks_1_3_5_17_63_rank_128", "x_minus_x_plus_y", "rank_7", "d2", "true_rank_98_rank_72"])
def test_new_cores_are_left_orthogonal(name, mode):
    coefs, trains, eng, L, _ = _edge(name)
    n = [c.shape[1] for c in trains[0]]
    new = E.TTCross.lincomb_round(coefs, eng, rank=L, tol=-1.0, seed=RS.SKETCH_SEED, mode=mode)
    l = RS.sketch_ranks(n, RS.rank_sums(trains), L if L else 128)
    assert eng[0].roundsum_last()["l"] == l and new.ranks().tolist() == l
    for k, g in enumerate(_cores(new)[:-1]):
        q = g.reshape((-1, g.shape[2]), order="F")
        dev = float(np.max(np.abs(q.T @ q - np.eye(q.shape[1]))))
        print(name, mode, "core", k + 1, q.shape, "|Q^T Q - I|_max / (4 rows u)", dev / (4.0 * q.shape[0] * RS.U))
        assert dev <= 4.0 * q.shape[0] * RS.U
    new.close()


def test_a_long_train_needs_the_common_power_of_two():
    coefs, trains = RS.long_train()
    d, n = len(trains[0]), [4] * len(trains[0])
    eng = [_up(("long", t), x) for t, x in enumerate(trains)]
    new = E.TTCross.lincomb_round(coefs, eng, rank=8, seed=RS.SKETCH_SEED, mode="mfma")
    assert new.ranks().tolist() == RS.sketch_ranks(n, RS.rank_sums(trains), 8)
    rng = np.random.default_rng(5)
    ind = np.ascontiguousarray(rng.integers(1, 5, (2000, d)), dtype=np.int32)
    got = new.tijk_batch(ind, "exact")
    want = sum(np.float64(c) * t.tijk_batch(ind, "exact") for c, t in zip(coefs, eng))
    newcores = _cores(new)
    new.close()
    bound = 2.0 * A.n_lincomb(newcores, len(trains)) * A.U * A.elements(A.lincomb_abs(coefs, trains), ind)
    assert np.all(np.isfinite(got)) and np.all(want != 0.0)
    A.check("long train", got, want, bound)


def test_a_call_repeats_bit_for_bit_and_another_seed_gives_the_same_tensor():
    c = _fails_today()
    allow = RS.allowance(c["coefs"], c["terms"], c["ref"], True)
    a = E.TTCross.lincomb_round(c["coefs"], c["eng"], rank=16, seed=11, mode="mfma")
    b = E.TTCross.lincomb_round(c["coefs"], c["eng"], rank=16, seed=11, mode="mfma")
    o = E.TTCross.lincomb_round(c["coefs"], c["eng"], rank=16, seed=12, mode="mfma")
    ca, cb, co = _cores(a), _cores(b), _cores(o)
    for t in (a, b, o):
        t.close()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ca, cb))
    assert any(x.tobytes() != y.tobytes() for x, y in zip(ca, co))
    _check("seed 11", RS.dense(ca), c["dense"], allow)
    _check("seed 12", RS.dense(co), c["dense"], allow)


@pytest.mark.parametrize("name", ["ranks_1_3_5_17_63_rank_128", "rank_7", "d2"] + list(RS.MULTI_TILE))
def test_the_two_modes_agree(name):
    coefs, trains, eng, L, exact = _edge(name)
    ref = _reference(name, coefs, trains, L)
    got = []
    for mode in MODES:
        new = E.TTCross.lincomb_round(coefs, eng, rank=L, seed=RS.SKETCH_SEED, mode=mode)
        got.append(RS.dense(_cores(new)))
        new.close()
    _check(name + " exact against mfma", got[0], got[1], RS.allowance(coefs, trains, ref, exact))


def test_operands_stay_and_a_refusal_leaves_nothing_allocated():
    hip = E.load_library()          # hipMemGetInfo of the HIP runtime the engine itself is linked to (a process may hold a second one)

    def free_bytes():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    coefs, trains, eng, L, _ = _edge("same_engine_repeated")
    before = [[g.tobytes() for g in _cores(t)] for t in eng]
    E.TTCross.lincomb_round(coefs, eng, rank=L, seed=3).close()
    assert before == [[g.tobytes() for g in _cores(t)] for t in eng]
    lib = E.load_library()
    big, other = _up("r63", RS.edge_train("r63")), _up(("d2", 0), RS.d2_trains()[0])
    m = 66                                                                      # 66 x 63 = 4158 > 4096
    hs = (ctypes.c_void_p * m)(*[big._h] * m)
    cf = np.ones(m)
    out = ctypes.c_void_p(12345)
    free0 = free_bytes()
    rc = lib.ttx_lincomb_round(m, E._dp(cf), hs, 16, -1.0, 0, 0, 2, ctypes.byref(out))
    assert rc == 1 and not out.value and b"bond 1" in lib.ttx_last_error() and b"4158" in lib.ttx_last_error(), lib.ttx_last_error()
    with pytest.raises(E.TTXError, match="dimensions not match"):
        E.TTCross.lincomb_round([1.0, 1.0], [big, other], rank=4)
    assert free_bytes() == free0
    assert before == [[g.tobytes() for g in _cores(t)] for t in eng]


def test_a_failure_after_the_new_engine_exists_releases_it():
    """A rank-128 train with a mode of 1024 points: the unfolding of 131072 rows and 128 columns is one the engine's QR refuses (as
    ttx_ort does on such a train), after the new engine, its work buffers and the operand's work space exist.  The work space stays
    with the operand by design, so the second failing call starts from what the first left: it must leave the same free memory."""
    hip = E.load_library()

    def free_bytes():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    cores = RS.rand_train(77, [200, 1024, 200], [1, 128, 128, 1])
    x = E.TTCross.from_cores(cores)
    first = x.core(2).tobytes()
    left = []
    for _ in range(2):
        with pytest.raises(E.TTXError, match="does not fit"):
            E.TTCross.lincomb_round([1.0], [x], rank=128, seed=1)
        left.append(free_bytes())
    assert left[0] == left[1], left
    assert x.core(2).tobytes() == first
    small = E.TTCross.lincomb_round([2.0], [x], rank=64, seed=1)                # the operand and its work space still serve
    assert small.ranks().tolist() == [1, 64, 64, 1]
    small.close()
    x.close()


def test_a_nan_core_gives_a_nan_train_and_no_fault():
    """in a process of its own, as the other NaN tests (tests/nan_worker.py says why)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "roundsum_nan_worker.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def test_fortran_roundsum(tmp_path):
    from conftest import fortran_exe
    exe = fortran_exe("test_tt_roundsum")
    names = ["r3", "r5", "r17"]
    paths = []
    for x in names:
        paths.append(str(tmp_path / (x + ".tt")))
        _up(x, RS.edge_train(x)).write(paths[-1])
    p = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("done"), p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.split()]
    coefs, trains = [1.5, -0.5, 0.25], [RS.edge_train(x) for x in names]
    ref = RS.roundsum(coefs, trains, 17, 5)
    assert [ln for ln in lines if ln[0] == "ranks"] == [["ranks"] + [str(x) for x in ref["l"]]]
    trunc = [[int(x) for x in ln[1:]] for ln in lines if ln[0] == "trunc"]
    # tol = 1d-10 on the same sum: r17 is a block assembly of r5, r3 and r1, so the sum's true ranks are at most 5 + 3 + 1 = 9
    assert len(trunc) == 1 and len(trunc[0]) == 8 and trunc[0][0] == trunc[0][-1] == 1 and all(1 <= a <= b for a, b in zip(trunc[0], ref["l"]))
    assert max(trunc[0]) <= 9, trunc
    el = np.array([float(ln[2]) for ln in lines if ln[0] == "elem"])
    assert el.shape == (24,)
    ind = np.array([[1 + (p_ * (2 * k + 1) + k) % RS.EDGE_N[k - 1] for k in range(1, 8)] for p_ in range(1, 25)], dtype=np.int32)
    S = RS.dense_sum(coefs, trains)
    want = np.array([S[tuple(i - 1 for i in row)] for row in ind])
    allow = RS.allowance(coefs, trains, ref, True) + 24 * A.n_ijk(ref["cores"]) * A.U * float(np.linalg.norm(S))   # + the chain that reads an element
    print("fortran: largest |diff| / allowance", float(np.max(np.abs(el - want))) / allow)
    assert np.all(np.abs(el - want) <= allow)
