"""Sums and elementwise products of resident trains on the device: ttx_lincomb / ttx_hadamard (ttcross_amd/csrc/ttx_algebra.h).

The checker is tests/algebra_ref.py (numpy float64).  Cores are compared BIT FOR BIT: every element of a new core is a copy, a
zero or one rounded product.  Comparisons of elements and sums use derived bounds, not measured ones (algebra_ref's docstring):
an element read with tijk_batch(..., "exact") is a chain of matrix-vector steps over the new cores, N_chain = sum_(k=0..d) r'_k
operations on a chain of absolute values; the first new core of a lincomb carries one more rounding, every core of a Hadamard
product one.  The value it is compared with -- sum_t c_t tijk(x_t), or tijk(x) tijk(y), formed from the device's own elements of
the operands -- carries the operands' shorter chains plus its own multiplies and additions.  Both stay below
    N_lincomb = N_chain + m + 1,   N_hadamard = N_chain + d + 2
times u = 2^-53 times B, B the same element of the train of |new cores| (|coef| included), so the two differ by at most 2 N u B,
and are equal where B = 0.  quad(lincomb) against sum_t c_t quad(x_t) is the same argument with reduce_ref's N_quad = sum_k (n_k +
r_(k-1)) in the place of N_chain; wdot against the reference's Hadamard cores is reduce_ref.quad_bound itself, the device's
Hadamard cores being the reference's bit for bit.
dist: |x.dist(y) - tt_ref.norm(block train of x - y)| <= 1e-12 (|x| + |y|) -- 1e-12 of the norm is the tolerance of the device
against tt_ref.norm in tests/test_gpu_ttops_edges.py (e.g. test_rank_sweep_across_the_paths); here it is taken relative to
|x| + |y|, the scale of the numbers that enter the QR of the difference train.  tt_ref.norm is Gram based and cancels itself:
that comparison runs at the scale of z where the reference's own error is a hundredth of the tolerance (the test's docstring);
at |x - y| = 1e-9 |x| the same dist is compared with the norm of the dense difference."""
import ctypes
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import algebra_ref as A
import reduce_ref as Q
import tt_ref as R
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

NPTS = 2000
U = A.U
NORM_TOL = 1e-12


def _chain(d, r):
    return [1] + [r] * (d - 1) + [1]


# name -> (n, r)
TRAINS = {
    "d2_r3": ([5, 7], [1, 3, 1]),
    "d2_r4": ([5, 7], [1, 4, 1]),
    "d3_a": ([5, 7, 4], [1, 3, 2, 1]),
    "d3_b": ([5, 7, 4], [1, 2, 5, 1]),
    "d3_r1": ([5, 7, 4], [1, 1, 1, 1]),
    "d3_r16": ([5, 7, 4], [1, 16, 7, 1]),
    "d6_a": ([4, 1, 6, 1, 5, 3], [1, 3, 5, 1, 4, 2, 1]),           # the d6_modes_of_size_1_rank_1_bond shape of the contract test
    "d6_b": ([4, 1, 6, 1, 5, 3], [1, 6, 2, 7, 1, 3, 1]),
    "d4_r63": ([3, 4, 5, 3], _chain(4, 63)),
    "d4_r2": ([3, 4, 5, 3], _chain(4, 2)),
    "d4_r65": ([3, 4, 5, 3], _chain(4, 65)),
    "d4_r64": ([3, 4, 5, 3], _chain(4, 64)),
    "d4_r10": ([3, 4, 5, 3], [1, 3, 10, 2, 1]),
    "d4_r13": ([3, 4, 5, 3], [1, 2, 13, 5, 1]),
    "d5_r64": ([4] * 5, _chain(5, 64)),
    "d5_r64'": ([4] * 5, _chain(5, 64)),
    "d5_r127": ([4] * 5, _chain(5, 127)),
    "d5_r1": ([4] * 5, _chain(5, 1)),
    "d5_r2": ([4] * 5, _chain(5, 2)),
    "d5_r8": ([4] * 5, [1, 4, 8, 8, 3, 1]),
    "d5_r16": ([4] * 5, [1, 5, 16, 16, 7, 1]),
    "d5_r11": ([4] * 5, [1, 4, 11, 11, 3, 1]),
    "d63_r2": ([3] * 63, _chain(63, 2)),
    "d63_r3": ([3] * 63, _chain(63, 3)),
}
_cache = {}


def _tt(name):
    """a source train, uploaded once and never changed (test_nothing_else_moves checks that the operations change nothing)"""
    if name not in _cache:
        n, r = TRAINS[name]
        cores = R.rand_train(sum(map(ord, name)), n, r)
        _cache[name] = (E.TTCross.from_cores(cores), cores)
    return _cache[name]


def _cores(tt):
    return [tt.core(k) for k in range(1, tt.d + 1)]


def _points(n, seed, npts=NPTS):
    """npts - 2 random multi-indices (1-based) plus the two corners, or every multi-index when there are fewer"""
    n = np.asarray(n, dtype=np.int64)
    if float(np.prod(n.astype(np.float64))) <= npts:
        return np.ascontiguousarray(np.array(list(itertools.product(*[range(1, int(k) + 1) for k in n])), dtype=np.int32))
    rng = np.random.default_rng(seed)
    ind = (rng.integers(0, 2 ** 31 - 1, (npts - 2, n.size)) % n + 1).astype(np.int32)
    return np.ascontiguousarray(np.vstack([ind, np.ones((1, n.size), np.int32), n[None, :].astype(np.int32)]))


def _same_bytes(tag, tt, ref):
    assert tt.ranks().tolist() == A.ranks(ref), tag
    assert tt._n.tolist() == [c.shape[1] for c in ref], tag
    for k, (a, b) in enumerate(zip(_cores(tt), ref)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, "core", k + 1)


LINCOMB = {
    "d2_no_interior_core": ([1.5, -0.75], ["d2_r3", "d2_r4"]),
    "d3": ([2.0, 3.0], ["d3_a", "d3_b"]),
    "d6_modes_of_size_1_rank_1_bond": ([-1.0, 0.3], ["d6_a", "d6_b"]),
    "ranks_63_plus_2": ([1.0, -1.0], ["d4_r63", "d4_r2"]),
    "ranks_2_plus_63": ([0.1, 7.0], ["d4_r2", "d4_r63"]),
    "ranks_64_plus_64": ([1.0, 1e-3], ["d5_r64", "d5_r64'"]),
    "ranks_127_plus_1": ([-2.0, 0.5], ["d5_r127", "d5_r1"]),
    "ranks_1_plus_127": ([-2.0, 0.5], ["d5_r1", "d5_r127"]),
    "three_terms_one_engine_twice": ([0.5, 3.0, -0.25], ["d3_a", "d3_b", "d3_a"]),
    "x_plus_x": ([1.0, 1.0], ["d6_a", "d6_a"]),
    "one_term_coef_1": ([1.0], ["d6_b"]),
    "one_term_coef_-2.5": ([-2.5], ["d4_r63"]),
    "long_thin_d63": ([1.25, -3.0], ["d63_r2", "d63_r3"]),
    "coef_zero": ([0.0, 1.0], ["d3_a", "d3_b"]),
    "coef_nan": ([float("nan"), 1.0], ["d3_a", "d3_b"]),
}
HADAMARD = {
    "rank_1_times_rank_r": ("d3_r1", "d3_r16"),
    "rank_r_times_rank_1": ("d3_r16", "d3_r1"),
    "d3": ("d3_a", "d3_b"),
    "8_times_16": ("d5_r8", "d5_r16"),
    "16_times_8": ("d5_r16", "d5_r8"),
    "11_times_11_same_engine": ("d5_r11", "d5_r11"),
    "64_times_2": ("d5_r64", "d5_r2"),
    "2_times_64": ("d5_r2", "d5_r64"),
    "unequal_ranks_modes_of_size_1": ("d6_a", "d6_b"),
    "long_thin_d63": ("d63_r2", "d63_r3"),
}


@pytest.mark.parametrize("case", sorted(LINCOMB))
def test_lincomb_cores_bit_for_bit(case):
    coefs, names = LINCOMB[case]
    tts = [_tt(nm)[0] for nm in names]
    src = [_tt(nm)[1] for nm in names]
    got = E.TTCross.lincomb(coefs, tts)
    assert got.ranks().tolist() == A.lincomb_ranks(src)
    _same_bytes(case, got, A.lincomb_cores(coefs, src))
    if case == "one_term_coef_1":
        for a, b in zip(_cores(got), src[0]):
            assert a.tobytes() == b.tobytes()
    ms, rd, wr = tts[0].algebra_last()
    assert ms > 0 and rd == 8.0 * sum(c.size for x in src for c in x) and wr == 8.0 * sum(c.size for c in A.lincomb_cores(coefs, src))


def test_axpby_is_lincomb_of_two():
    (x, cx), (y, cy) = _tt("d3_a"), _tt("d3_b")
    _same_bytes("axpby", x.axpby(0.5, -4.0, y), A.lincomb_cores([0.5, -4.0], [cx, cy]))


@pytest.mark.parametrize("case", sorted(HADAMARD))
def test_hadamard_cores_bit_for_bit(case):
    (x, cx), (y, cy) = _tt(HADAMARD[case][0]), _tt(HADAMARD[case][1])
    got = x.hadamard(y)
    assert got.ranks().tolist() == A.hadamard_ranks(cx, cy)
    ref = A.hadamard_cores(cx, cy)
    _same_bytes(case, got, ref)
    ms, rd, wr = x.algebra_last()
    assert ms > 0 and rd == 8.0 * (sum(c.size for c in cx) + sum(c.size for c in cy)) and wr == 8.0 * sum(c.size for c in ref)


@pytest.mark.parametrize("case", ["d2_no_interior_core", "d3", "d6_modes_of_size_1_rank_1_bond", "ranks_63_plus_2", "ranks_127_plus_1",
                                  "three_terms_one_engine_twice", "one_term_coef_-2.5", "long_thin_d63", "coef_zero"])
def test_lincomb_elements(case):
    coefs, names = LINCOMB[case]
    tts = [_tt(nm)[0] for nm in names]
    src = [_tt(nm)[1] for nm in names]
    got = E.TTCross.lincomb(coefs, tts)
    ind = _points(got._n, 7)
    want = sum(np.float64(c) * t.tijk_batch(ind, "exact") for c, t in zip(coefs, tts))
    new = A.lincomb_cores(coefs, src)
    bound = 2.0 * A.n_lincomb(new, len(names)) * U * A.elements(A.lincomb_abs(coefs, src), ind)
    A.check(case, got.tijk_batch(ind, "exact"), want, bound)


@pytest.mark.parametrize("case", ["rank_1_times_rank_r", "d3", "8_times_16", "11_times_11_same_engine", "2_times_64", "unequal_ranks_modes_of_size_1", "long_thin_d63"])
def test_hadamard_elements(case):
    (x, cx), (y, cy) = _tt(HADAMARD[case][0]), _tt(HADAMARD[case][1])
    got = x.hadamard(y)
    ind = _points(got._n, 8)
    want = x.tijk_batch(ind, "exact") * y.tijk_batch(ind, "exact")
    bound = 2.0 * A.n_hadamard(A.hadamard_cores(cx, cy)) * U * A.elements(A.hadamard_abs(cx, cy), ind)
    A.check(case, got.tijk_batch(ind, "exact"), want, bound)


def _weights(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(int(k)) for k in n]


@pytest.mark.parametrize("case", ["d3", "d6_modes_of_size_1_rank_1_bond", "three_terms_one_engine_twice", "ranks_63_plus_2", "long_thin_d63"])
def test_quad_of_a_lincomb_is_the_lincomb_of_the_quads(case):
    coefs, names = LINCOMB[case]
    tts = [_tt(nm)[0] for nm in names]
    src = [_tt(nm)[1] for nm in names]
    for w in (_weights(tts[0]._n, 4), None):
        got = E.TTCross.lincomb(coefs, tts).quad(w)
        want = sum(np.float64(c) * t.quad(w) for c, t in zip(coefs, tts))
        bound = 2.0 * A.n_quad_lincomb(A.lincomb_cores(coefs, src), len(names)) * U * Q.quad_abs(A.lincomb_abs(coefs, src), w)
        A.check(f"{case} quad", got, want, bound)


@pytest.mark.parametrize("case", ["rank_1_times_rank_r", "d3", "8_times_16", "11_times_11_same_engine", "unequal_ranks_modes_of_size_1", "long_thin_d63"])
def test_wdot_against_quad_of_the_reference_cores(case):
    (x, cx), (y, cy) = _tt(HADAMARD[case][0]), _tt(HADAMARD[case][1])
    ref = A.hadamard_cores(cx, cy)
    for w in (_weights(x._n, 5), None):
        Q.check(f"{case} wdot", x.wdot(y, w), Q.quad(ref, w), Q.quad_bound(ref, w))


@pytest.mark.parametrize("name", ["d3_a", "d6_a", "d5_r16"])
def test_hadamard_with_the_train_of_ones_has_the_cores_of_x(name):
    x, cx = _tt(name)
    ones = E.TTCross.from_cores([np.ones((1, c.shape[1], 1)) for c in cx])
    for a, b in zip(_cores(x.hadamard(ones)), cx):
        assert a.tobytes() == b.tobytes()


DIST = [("d3_a", "d3_b"), ("d6_a", "d6_b"), ("d5_r8", "d5_r16")]
Z_LOG2 = 20         # z = 2^20 z0 for the comparison with tt_ref.norm (its docstring); z = z0 for the dense difference
_dist = {}


def _dist_case(name, zname, e):
    """x, y = x + 1e-9 z built on the host with z = 2^e times the train `zname`, and what is compared: computed once per case"""
    if (name, zname, e) not in _dist:
        x, cx = _tt(name)
        cz = _tt(zname)[1]
        cz = [np.ldexp(cz[0], e)] + cz[1:]
        cy = A.lincomb_cores([1.0, 1e-9], [cx, cz])
        y = E.TTCross.from_cores(cy)
        _dist[(name, zname, e)] = dict(cx=cx, cy=cy, scale=R.norm(cx) + R.norm(cy), got=x.dist(y),
                                       dense=float(np.linalg.norm(A.dense(cx) - A.dense(cy))))
    c = _dist[(name, zname, e)]
    print(name, zname, "z * 2^%d" % e, "dist", c["got"], "norm of the dense difference", c["dense"], "|x| + |y|", c["scale"])
    return c


@pytest.mark.parametrize("name,zname", DIST)
def test_dist_against_tt_ref_norm_of_the_block_train(name, zname):
    """x.dist(y), y = x + 1e-9 z, against tt_ref.norm of the reference's block train for x - y, to 1e-12 (|x| + |y|).
    The scale of z is chosen from the reference's own error.  tt_ref.norm contracts the Gram matrix of the block train [x, -y]:
    it forms |x|^2 - 2 <x, y> + |y|^2 with a rounding error of a few u (|x| + |y|)^2 and its square root is off by that error
    divided by 2 |x - y|.  With |z| about |x| (|x - y| about 1e-9 |x|) it is off by 1.7e-09 (|x| + |y|) on d3_a / d3_b -- it
    returns 1.2636e-07 for a difference whose dense norm is 3.5028e-08 -- and on the other two pairs the Gram sum comes out
    negative (math domain error): no computed dist could be compared with it at 1e-12.  Its error against the norm of the dense
    difference, both formed on the host, falls as |x - y| grows: about 1e-13 (|x| + |y|) at z * 2^12, 5e-14 at 2^16, 7e-15 or
    less at 2^20 (all three pairs), 2e-16 at 2^24.  z * 2^20 -- |x - y| about 1e-3 |x| -- is the smallest of these steps where
    the reference is good to a hundredth of the tolerance; the test asserts that first, without the device.  The small
    differences (z * 2^0), where dist matters most, are compared with the dense difference in the next test."""
    c = _dist_case(name, zname, Z_LOG2)
    block = R.norm(A.lincomb_cores([1.0, -1.0], [c["cx"], c["cy"]]))
    print("tt_ref.norm of the block train", block, "its own error / (|x| + |y|)", abs(block - c["dense"]) / c["scale"],
          "|dist - tt_ref.norm| / (|x| + |y|)", abs(c["got"] - block) / c["scale"], "tolerance", NORM_TOL)
    assert abs(block - c["dense"]) <= 0.01 * NORM_TOL * c["scale"]               # the reference itself, on the host
    assert block > 0 and abs(c["got"] - block) <= NORM_TOL * c["scale"]


@pytest.mark.parametrize("name,zname", DIST)
def test_dist_against_the_norm_of_the_dense_difference(name, zname):
    """|z| about |x|, so |x - y| is about 1e-9 |x|, below what sqrt(dot(x,x) - 2 dot(x,y) + dot(y,y)) resolves.  x and y are small
    enough to expand: dense(x) - dense(y) elementwise has no cancellation between large sums (each dense element is within
    n_ijk u |x|(i), about 1e-14 |x| in the norm), so its norm is a reference at the same tolerance"""
    c = _dist_case(name, zname, 0)
    print("|diff| / (|x| + |y|)", abs(c["got"] - c["dense"]) / c["scale"], "tolerance", NORM_TOL)
    assert c["dense"] > 0 and abs(c["got"] - c["dense"]) <= NORM_TOL * c["scale"]


@pytest.mark.parametrize("name", ["d3_a", "d6_a", "d5_r8"])
def test_dist_of_a_train_to_itself(name):
    x, cx = _tt(name)
    nx, same = R.norm(cx), x.dist(x)
    print(name, "dist(x, x) / 2|x|", same / (2.0 * nx))
    assert 0.0 <= same <= NORM_TOL * 2.0 * nx


def test_downstream_use_of_the_results(tmp_path):
    x, cx = _tt("d5_r8")                                               # ranks no unfolding can lower: svd returns to them
    two = E.TTCross.lincomb([1.0, 1.0], [x, x])
    had = x.hadamard(_tt("d5_r16")[0])
    for name, t in (("sum", two), ("product", had)):
        p = os.path.join(str(tmp_path), name + ".tt")
        t.write(p)
        back = E.TTCross.read(p)
        assert back.ranks().tolist() == t.ranks().tolist()
        for a, b in zip(_cores(back), _cores(t)):
            assert a.tobytes() == b.tobytes()
    nrm = x.norm()
    two.svd(1e-8)
    assert two.ranks().tolist() == x.ranks().tolist()
    assert abs(two.norm() - 2.0 * nrm) <= 1e-6 * 2.0 * nrm
    # and the results are operands again
    again = E.TTCross.lincomb([1.0, -2.0], [two, x])
    assert again.ranks().tolist() == [1] + [2 * r for r in x.ranks().tolist()[1:-1]] + [1]
    assert np.isfinite(again.norm())


def test_two_calls_give_the_same_bytes():
    for case in ("ranks_63_plus_2", "ranks_64_plus_64", "long_thin_d63"):
        coefs, names = LINCOMB[case]
        tts = [_tt(nm)[0] for nm in names]
        a, b = E.TTCross.lincomb(coefs, tts), E.TTCross.lincomb(coefs, tts)
        assert [c.tobytes() for c in _cores(a)] == [c.tobytes() for c in _cores(b)]
    for case in ("8_times_16", "11_times_11_same_engine", "long_thin_d63"):
        x, y = _tt(HADAMARD[case][0])[0], _tt(HADAMARD[case][1])[0]
        a, b = x.hadamard(y), x.hadamard(y)
        assert [c.tobytes() for c in _cores(a)] == [c.tobytes() for c in _cores(b)]


def test_nothing_else_moves():
    s = D.ising_setup("c", 6, 33)
    x = E.TTCross(s["n"], s["fun_id"], s["par"], 8, pivoting=2, accuracy=s["acc"], quad=s["quad"], tru=s["tru"]).run()
    y = E.TTCross.from_cores(R.rand_train(5, [int(k) for k in x._n], _chain(x.d, 3)))
    ind = _points(x._n, 5, 50)

    def state(t):
        return (t.ranks().tobytes(), [c.tobytes() for c in _cores(t)], t.quad(s["quad"]), t.norm(), t.tijk(ind[3]), t.tijk_batch(ind, "exact").tobytes(),
                [m.tobytes() for m in t.marginals()])

    bx, by = state(x), state(y)
    E.TTCross.lincomb([2.0, -1.0], [x, y])
    assert state(x) == bx and state(y) == by
    x.hadamard(y)
    y.hadamard(x)
    assert state(x) == bx and state(y) == by
    E.TTCross.lincomb([1.0, -1.0, 0.5], [x, x, y])                      # the same engine twice
    x.hadamard(x)
    x.dist(x)
    x.wdot(y, s["quad"])
    assert state(x) == bx and state(y) == by


def test_argument_errors():
    L = E.load_library()
    EINVAL, ESTATE = 1, 4
    vp = ctypes.c_void_p
    x, y = _tt("d3_a")[0], _tt("d3_b")[0]
    out = vp(12345)

    def lincomb(coefs, hs, m=None):
        out.value = 12345
        c = np.asarray(coefs, dtype=np.float64)
        arr = (vp * len(hs))(*hs)
        rc = L.ttx_lincomb(len(hs) if m is None else m, E._dp(c), arr, ctypes.byref(out))
        assert rc != 0 and not out.value                              # *out is null after a refusal
        return rc

    def hadamard(a, b):
        out.value = 12345
        rc = L.ttx_hadamard(a, b, ctypes.byref(out))
        assert rc != 0 and not out.value
        return rc

    two = (vp * 2)(x._h, y._h)
    c2 = np.array([1.0, 1.0])
    out.value = 12345
    assert L.ttx_lincomb(2, None, two, ctypes.byref(out)) == EINVAL and not out.value
    out.value = 12345
    assert L.ttx_lincomb(2, E._dp(c2), None, ctypes.byref(out)) == EINVAL and not out.value
    assert L.ttx_lincomb(2, E._dp(c2), two, None) == EINVAL
    assert lincomb([1.0, 1.0], [x._h, None]) == EINVAL
    assert lincomb([1.0, 1.0], [x._h, y._h], m=0) == EINVAL
    assert lincomb([1.0, 1.0], [x._h, y._h], m=-1) == EINVAL
    assert hadamard(x._h, None) == EINVAL and hadamard(None, y._h) == EINVAL
    assert L.ttx_hadamard(x._h, y._h, None) == EINVAL
    v = ctypes.c_double()
    assert L.ttx_algebra_last(x._h, None, ctypes.byref(v), ctypes.byref(v)) == EINVAL
    # unequal d, unequal mode sizes
    d4, d2 = _tt("d4_r2")[0], _tt("d2_r3")[0]
    other_n = E.TTCross.from_cores(R.rand_train(3, [5, 6, 4], [1, 2, 2, 1]))
    for bad in (d4, d2, other_n):
        assert lincomb([1.0, 1.0], [x._h, bad._h]) == EINVAL
        assert hadamard(x._h, bad._h) == EINVAL and hadamard(bad._h, x._h) == EINVAL
    with pytest.raises(E.TTXError):
        x.hadamard(other_n)
    with pytest.raises(E.TTXError):
        x.axpby(1.0, 1.0, d4)
    with pytest.raises(ValueError):
        E.TTCross.lincomb([1.0], [x, y])
    with pytest.raises(ValueError):
        E.TTCross.lincomb([], [])
    # ranks beyond the engine's cap: the message names the bond and the value
    assert lincomb([1.0, 1.0], [_tt("d4_r65")[0]._h, _tt("d4_r64")[0]._h]) == EINVAL
    msg = L.ttx_last_error().decode()
    assert "bond 1" in msg and "129" in msg, msg
    assert hadamard(_tt("d4_r10")[0]._h, _tt("d4_r13")[0]._h) == EINVAL
    msg = L.ttx_last_error().decode()
    assert "bond 2" in msg and "130" in msg, msg
    # an engine that has not run
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    assert lincomb([1.0], [fresh._h]) == ESTATE
    assert hadamard(fresh._h, fresh._h) == ESTATE
    # the two-process engine of the tijk test: whatever ttx_ijk answers
    mp = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"], nproc=2, world_rank=0, world_size=2)
    i5, val = np.ones((1, 5), np.int32), ctypes.c_double()
    want = L.ttx_ijk(mp._h, E._ip(i5), ctypes.byref(val))
    assert want != 0
    assert lincomb([1.0], [mp._h]) == want
    assert hadamard(mp._h, mp._h) == want
    # the engines are still good
    _same_bytes("after the refusals", x.axpby(1.0, 1.0, y), A.lincomb_cores([1.0, 1.0], [_tt("d3_a")[1], _tt("d3_b")[1]]))


def test_fortran_axpby_and_hadamard():
    """the drop-in tt_lib: axpby(alpha,x,beta,y) has the cores of the host alpha*x + beta*y bit for bit; ranks by the stated rules;
    elements of the results against the same values formed from tijk of the operands to 1e-12 of the element scale, the
    tolerance of the Fortran contract test"""
    import subprocess
    from conftest import fortran_exe
    exe = fortran_exe("test_tt_algebra")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("done"), p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.split()]
    same = [ln for ln in lines if ln[0] == "same"]
    assert [ln[1] for ln in same] == ["axpby", "axpby2"] and all(ln[2] == "T" for ln in same), same
    ranks = {ln[1]: [int(v) for v in ln[3:]] for ln in lines if ln[0] == "ranks"}
    assert ranks == {"axpby": [1, 5, 5, 5, 5, 1], "axpby2": [1, 8, 8, 8, 8, 1], "hadamard": [1, 6, 6, 6, 6, 1]}     # x rank 3, y rank 2
    el = np.array([[float(v) for v in ln[2:]] for ln in lines if ln[0] == "elem"])
    assert el.shape == (120, 2)
    for blk in np.split(el, 3):
        scale = np.abs(blk[:, 1]).max()
        assert scale > 0.1 and len(set(blk[:, 1])) > 30
        assert np.all(np.abs(blk[:, 0] - blk[:, 1]) <= 1e-12 * scale)
