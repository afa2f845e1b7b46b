"""The full reductions of a resident train -- ttx_dot, ttx_quad, ttx_zquad and the single-element ttx_ijk -- on unlike trains.

The checker is tests/reduce_ref.py (numpy float64): |device - reference| <= 2 N u B with N the derived operation count and B the
same quantity on absolute values, equal where B = 0 (derivation in that module; tests/test_reductions_ref_cpu.py shows that the
bound rejects a dropped weight, rank index or tail of an inner product at these very shapes).  On the non-negative twins B is the
value itself and the bound is a relative tolerance of about 1e-13.

ttx_dot(x, y) works in the scratch of x, which is sized by x's own maxrank RM and largest mode NM: it refuses a y whose cores or
interface matrices do not fit ("ranks of y exceed the work space of x").  _fits restates that rule from the sizes documented in
ttx_dot; every pair is compared in each order the rule admits -- at least one, asserted -- and the other order must be refused."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import reduce_ref as Q
import tt_ref as R
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

_cache = {}


def _cores(tt):
    return [tt.core(k) for k in range(1, tt.d + 1)]


def _up(name, nonneg=False):
    """(engine, cores, maxrank) of a train of reduce_ref.SHAPES, uploaded once and never changed (the tests of this module only read)"""
    key = (name, nonneg)
    if key not in _cache:
        cores = Q.train(name, nonneg)
        _cache[key] = (E.TTCross.from_cores(cores), cores, max(Q.ranks(cores)))
    return _cache[key]


SWEEP_RM = 8


def _sweep(nproc):
    """Ising C_7 on 9 nodes, maxrank 8, pivoting 2, in one group or in three (a single process); cores as read back"""
    key = ("sweep", nproc)
    if key not in _cache:
        s = D.ising_setup("c", 7, 9)
        tt = E.TTCross(s["n"], s["fun_id"], s["par"], SWEEP_RM, pivoting=2, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=nproc).run()
        _cache[key] = (tt, _cores(tt), SWEEP_RM)
    return _cache[key]


def _fits(x, rmx, y):
    """the rule of ttx_dot: y's packed core, phi times it and the interface matrices fit the scratch of x (maxrank rmx)"""
    cs = rmx * max(Q.modes(x)) * rmx
    return all(cx.shape[2] * cy.shape[2] <= rmx * rmx and cx.shape[0] * cy.shape[0] <= rmx * rmx and
               cx.shape[0] * cx.shape[1] * cy.shape[2] <= cs and cy.shape[0] * cy.shape[1] * cy.shape[2] <= cs for cx, cy in zip(x, y))


def _state(tt):
    return tt.ranks().tobytes(), [c.tobytes() for c in _cores(tt)]


def _check_dot(tag, X, Y):
    """x.dot(y) against the reference where the work space of x admits y, the refusal where it does not; returns 1 if compared"""
    (tx, x, rmx), (ty, y, _) = X, Y
    if not _fits(x, rmx, y):
        with pytest.raises(E.TTXError, match="work space of x"):
            tx.dot(ty)
        print(tag, "refused: work space of x")
        return 0
    Q.check(tag, tx.dot(ty), Q.dot(x, y), Q.dot_bound(x, y))
    return 1


def _check_both_orders(tag, X, Y):
    before = _state(X[0]), _state(Y[0])
    assert _check_dot(f"dot {tag} x.y", X, Y) + _check_dot(f"dot {tag} y.x", Y, X) >= 1
    _check_dot(f"dot {tag} x.x", X, X)
    _check_dot(f"dot {tag} y.y", Y, Y)
    assert (_state(X[0]), _state(Y[0])) == before                    # nothing moves, refused or not


# ---- dot --------------------------------------------------------------------------------------------------------------
DOT_PAIRS = [("A", "A'", False), ("B", "B'", False), ("C", "C'", False), ("E64", "E64'", False), ("L", "L'", False),
             ("A", "A'", True), ("E64", "E64'", True), ("L", "L'", True)]


@pytest.mark.parametrize("nx,ny,nonneg", DOT_PAIRS, ids=[f"{a}_{b}_{'nonneg' if s else 'mixed'}" for a, b, s in DOT_PAIRS])
def test_dot_of_two_different_trains(nx, ny, nonneg):
    _check_both_orders(f"{nx} {ny}{' nonneg' if nonneg else ''}", _up(nx, nonneg), _up(ny, nonneg))


def test_dot_of_unlike_engines():
    """y of small ranks in an engine of large maxrank: the svd truncation of E64' (n = 3: its ranks drop to 9 at most, RM stays 66),
    against E64 and E64' in both roles; the reference takes the cores read back from that engine"""
    ts = E.TTCross.from_cores(Q.train("E64'")).svd(1e-2)
    S = (ts, _cores(ts), 66)
    assert max(Q.ranks(S[1])) <= 9
    for other in ("E64", "E64'"):
        O = _up(other)
        assert _fits(S[1], 66, O[1]) and _fits(O[1], O[2], S[1])         # small ranks in x's role and in y's
        _check_both_orders(f"svd(E64') {other}", S, O)


def test_dot_refuses_what_does_not_fit_and_stays_usable():
    x = E.TTCross.from_cores(R.rand_train(12, [3, 3, 3], [1, 12, 12, 1]))
    y = E.TTCross.from_cores(R.rand_train(40, [3, 3, 3], [1, 3, 40, 1]))
    cx, cy = _cores(x), _cores(y)
    before = x.dot(x), x.quad(), _state(x), _state(y)
    with pytest.raises(E.TTXError, match="work space of x"):
        x.dot(y)
    Q.check("dot refusal y.x", y.dot(x), Q.dot(cy, cx), Q.dot_bound(cy, cx))
    assert (x.dot(x), x.quad(), _state(x), _state(y)) == before          # bit for bit
    Q.check("dot refusal x.x", before[0], Q.dot(cx, cx), Q.dot_bound(cx, cx))


@pytest.mark.parametrize("nproc", [1, 3])
def test_dot_of_a_sweep_result_and_a_loaded_train(nproc):
    X = _sweep(nproc)
    assert X[0].ranks().tolist() == Q.ranks(X[1]) and max(Q.ranks(X[1])) == SWEEP_RM
    y = R.rand_train(77, Q.modes(X[1]), [1, 3, 5, 7, 5, 3, 1])
    Y = (E.TTCross.from_cores(y), y, 7)
    assert _fits(X[1], SWEEP_RM, y)
    _check_both_orders(f"sweep nproc {nproc} loaded", X, Y)
    # the same y in an engine with room for x in y's role: maxrank 8 from a duplicated rank index that svd removes again
    pad = [c.copy() for c in y]
    pad[2] = np.concatenate([pad[2], pad[2][:, :, -1:]], axis=2)
    pad[3] = np.concatenate([pad[3], pad[3][-1:]], axis=0)
    pad[3][-2:] *= 0.5
    tz = E.TTCross.from_cores(pad).svd(1e-10)
    Z = (tz, _cores(tz), 8)
    assert Q.ranks(Z[1]) == [1, 3, 5, 7, 5, 3, 1] and _fits(Z[1], 8, X[1]) and _fits(X[1], SWEEP_RM, Z[1])
    assert _check_dot(f"dot sweep nproc {nproc} roomy x.y", X, Z) + _check_dot(f"dot sweep nproc {nproc} roomy y.x", Z, X) == 2


def test_dot_refuses_mismatching_trains():
    a = _up("C")[0]
    with pytest.raises(E.TTXError, match="dimensions not match"):
        a.dot(_up("F97")[0])
    with pytest.raises(E.TTXError, match="sizes not match"):
        a.dot(E.TTCross.from_cores(R.rand_train(1, [2, 4], [1, 2, 1])))


# ---- quad -------------------------------------------------------------------------------------------------------------
QUAD = ["A", "A'", "B", "B'", "C", "C'", "E64", "E64'", "F97", "F98", "F128", "L", "L'", "Z71", "Z72"]
QUAD_NONNEG = ["A", "A'", "E64", "E64'", "F98", "L"]


@pytest.mark.parametrize("name,nonneg", [(nm, False) for nm in QUAD] + [(nm, True) for nm in QUAD_NONNEG],
                         ids=[nm + "_mixed" for nm in QUAD] + [nm + "_nonneg" for nm in QUAD_NONNEG])
def test_quad_with_weights_and_without(name, nonneg):
    tt, cores, _ = _up(name, nonneg)
    w = Q.weights(name, 0, nonneg)
    sfx = " nonneg" if nonneg else ""
    Q.check(f"quad {name}{sfx} w", tt.quad(w), Q.quad(cores, w), Q.quad_bound(cores, w))
    plain = tt.quad()
    Q.check(f"quad {name}{sfx} plain", plain, Q.quad(cores), Q.quad_bound(cores))
    ones = tt.quad([np.ones(k) for k in Q.modes(cores)])
    assert np.float64(plain).tobytes() == np.float64(ones).tobytes()     # y + 1.0 * a and y + a round alike
    if nonneg:
        assert Q.quad_bound(cores, w) < 1e-11 * Q.quad(cores, w)


def test_quad_of_a_three_group_sweep_result_with_other_weights():
    """ends in k_quad_tree; weights that are not the run's own quadrature"""
    tt, cores, _ = _sweep(3)
    rng = np.random.default_rng(9)
    w = [rng.standard_normal(k) for k in Q.modes(cores)]
    Q.check("quad sweep nproc 3 w", tt.quad(w), Q.quad(cores, w), Q.quad_bound(cores, w))
    Q.check("quad sweep nproc 3 plain", tt.quad(), Q.quad(cores), Q.quad_bound(cores))
    assert tt.quad() == tt.quad([np.ones(k) for k in Q.modes(cores)])


# ---- zquad ------------------------------------------------------------------------------------------------------------
def _ztrain(name):
    return _sweep(3)[:2] if name == "sweep3" else _up(name)[:2]


def _zw(name, cores, nf):
    if name == "sweep3":
        rng = np.random.default_rng(33 + nf)
        sn = sum(Q.modes(cores))
        return np.exp(1j * rng.uniform(0.0, 2.0 * np.pi, (nf, sn))) * 2.0 ** rng.uniform(-3.0, 3.0, (nf, sn))
    return Q.zweights(name, nf)


@pytest.mark.parametrize("nf", [1, 33])
@pytest.mark.parametrize("name", ["A", "B", "C", "L", "Z71", "sweep3"])
def test_zquad_against_the_reference(name, nf):
    tt, cores = _ztrain(name)
    W = _zw(name, cores, nf)
    got = tt.zquad(W)
    assert got.shape == (nf,)
    Q.check(f"zquad {name} nf {nf}", got, Q.zquad(cores, W), Q.zquad_bound(cores, W))
    # conj W gives the conjugate: negating the imaginary weights negates yi = yi + wi v, bi ai keeps its value and br ai + bi ar
    # changes sign term by term (the build is compiled without contraction), so every rounding commutes with the negation
    gc = tt.zquad(np.conj(W))
    assert np.array_equal(gc.real, got.real) and np.array_equal(gc.imag, -got.imag)
    # an entry does not depend on its batch
    for k in sorted({0, nf // 4, nf - 1}):
        assert tt.zquad(W[k:k + 1]).tobytes() == got[k:k + 1].tobytes(), k


@pytest.mark.parametrize("name", ["A", "B", "C", "L", "Z71", "sweep3"])
def test_zquad_with_real_weights_is_quad(name):
    tt, cores = _ztrain(name)
    W = _zw(name, cores, 5).real * 2.0
    got = tt.zquad(W)
    assert np.all(got.imag == 0.0) and not np.any(np.signbit(got.imag))
    ws = [Q.split(cores, W[f]) for f in range(5)]
    Q.check(f"zquad {name} real weights", got.real, np.array([Q.quad(cores, w) for w in ws]), np.array([Q.quad_bound(cores, w) for w in ws]))


def test_zquad_lds_ceiling():
    tt, cores, _ = _up("Z72")
    before = np.float64(tt.quad(Q.weights("Z72"))).tobytes(), _state(tt)
    with pytest.raises(E.TTXError, match="maxrank <= 71"):
        tt.zquad(Q.zweights("Z72", 1))
    assert (np.float64(tt.quad(Q.weights("Z72"))).tobytes(), _state(tt)) == before
    t71, c71, _ = _up("Z71")
    W = Q.zweights("Z71", 2, seed=1)
    Q.check("zquad Z71 accepted", t71.zquad(W), Q.zquad(c71, W), Q.zquad_bound(c71, W))


def test_zquad_argument_errors():
    tt, cores, _ = _up("C")
    with pytest.raises(E.TTXError, match="bad argument"):
        tt.zquad(np.zeros((0, 5), dtype=np.complex128))
    with pytest.raises(ValueError, match="sum"):
        tt.zquad(np.ones((1, 4), dtype=np.complex128))
    with pytest.raises(ValueError, match="sum"):
        tt.zquad(np.ones(6, dtype=np.complex128))
    Q.check("zquad C after the refusals", tt.zquad(np.ones(5)), Q.zquad(cores, np.ones(5)), Q.zquad_bound(cores, np.ones(5)))


# ---- the single element -------------------------------------------------------------------------------------------------
def _edge_indices(n, seed):
    """for every mode the tuples with that mode at 1 and at n_k (the others random), all ones, all last"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(len(n)):
        for v in (1, n[k]):
            ind = [int(rng.integers(1, nk + 1)) for nk in n]
            ind[k] = v
            out.append(ind)
    return out + [[1] * len(n), list(n)]


@pytest.mark.parametrize("name", ["A", "B", "E64", "F128"])
def test_tijk_at_the_first_and_last_index_of_every_mode(name):
    tt, cores, _ = _up(name)
    n = Q.modes(cores)
    inds = _edge_indices(n, len(name))
    got = np.array([tt.tijk(i) for i in inds])
    bound = np.array([Q.element_bound(cores, i) for i in inds])
    Q.check(f"tijk {name}", got, np.array([Q.element(cores, i) for i in inds]), bound)
    Q.check(f"tijk {name} against tijk_batch exact", got, tt.tijk_batch(np.array(inds, dtype=np.int32), "exact"), bound)
    for k in range(len(n)):
        for v in (0, n[k] + 1):
            ind = list(inds[2 * k])
            ind[k] = v
            assert tt.tijk(ind) == -3.0, ind
    assert tt.tijk(inds[0]) == got[0]
