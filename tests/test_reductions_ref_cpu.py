"""The checker of the device reductions (tests/reduce_ref.py) pinned on the CPU: against mpmath at 50 digits on small trains,
and against itself with one deliberate defect at a time -- every seeded defect must fall outside the derived bound 2 N u B at
the shapes tests/test_gpu_reductions.py runs, or that bound would let the same defect of a kernel pass."""
import numpy as np
import pytest

import reduce_ref as Q
import tt_ref as R

mp = R.mp
needs_mp = pytest.mark.skipif(mp is None, reason="mpmath is not installed")

# r <= 8, d <= 6, mixed sign, unequal modes, a rank-1 bond, a mode of size 1
SMALL = {
    "d6": ([3, 1, 4, 2, 5, 3], [1, 3, 8, 1, 4, 6, 1], [1, 2, 5, 3, 1, 7, 1]),
    "d4": ([2, 7, 3, 5], [1, 2, 8, 5, 1], [1, 2, 3, 8, 1]),
    "d2": ([5, 3], [1, 3, 1], [1, 5, 1]),
}


def _small(name):
    n, rx, ry = SMALL[name]
    seed = sum(map(ord, name))
    rng = np.random.default_rng(seed)
    w = [rng.standard_normal(k) for k in n]
    W = rng.standard_normal((3, sum(n))) + 1j * rng.standard_normal((3, sum(n)))
    return R.rand_train(seed, n, rx), R.rand_train(seed + 1, n, ry), w, W


# ---- the same quantities at 50 digits ---------------------------------------------------------------------------------
def _mp(a):
    if np.iscomplexobj(a):
        return np.vectorize(lambda z: mp.mpc(float(z.real), float(z.imag)), otypes=[object])(a)
    return R._to_mp(np.asarray(a, dtype=np.float64))


def _one():
    return np.array([[mp.mpf(1)]], dtype=object)


def _mode_sum(c, q):
    return sum((c[:, j, :] * q[j] for j in range(1, c.shape[1])), c[:, 0, :] * q[0])


def mp_dot(x, y):
    phi = _one()
    for cx, cy in zip(x, y):
        cx, cy = _mp(cx), _mp(cy)
        (rx0, n, rx1), (ry0, _, ry1) = cx.shape, cy.shape
        t = phi @ cy.reshape(ry0, n * ry1)
        phi = cx.reshape(rx0 * n, rx1).T @ t.reshape(rx0 * n, ry1)
    return phi[0, 0]


def mp_quad(cores, w):
    v = _one()
    for c, q in zip(cores, w):
        v = v @ _mode_sum(_mp(c), _mp(q))
    return v[0, 0]


def mp_element(cores, ind):
    v = _one()
    for c, j in zip(cores, ind):
        v = v @ _mp(c)[:, j - 1, :]
    return v[0, 0]


def _within(got, want_mp, n, b):
    """|got - truth| <= N u B (one side of the bound)"""
    return abs(mp.mpmathify(got) - want_mp) <= n * Q.U * b


@needs_mp
@pytest.mark.parametrize("name", list(SMALL))
def test_reference_is_within_n_u_b_of_50_digits(name):
    mp.dps = R.MP_DPS
    x, y, w, W = _small(name)
    for a, b in ((x, y), (y, x), (x, x)):
        assert _within(Q.dot(a, b), mp_dot(a, b), Q.n_dot(a, b), Q.dot_abs(a, b))
    for c in (x, y):
        assert _within(Q.quad(c, w), mp_quad(c, w), Q.n_quad(c), Q.quad_abs(c, w))
        assert _within(Q.quad(c), mp_quad(c, [np.ones(k) for k in Q.modes(c)]), Q.n_quad(c), Q.quad_abs(c))
        got, ab = Q.zquad(c, W), Q.zquad_abs(c, W)
        for f in range(W.shape[0]):
            want = mp_quad(c, Q.split(c, W[f]))
            assert abs(got[f].real - want.real) <= Q.n_zquad(c) * Q.U * ab[f]          # per component: N u B
            assert abs(got[f].imag - want.imag) <= Q.n_zquad(c) * Q.U * ab[f]
            assert abs(mp.mpc(got[f].real, got[f].imag) - want) <= 0.5 * Q.zquad_bound(c, W)[f]
        n = Q.modes(c)
        for ind in R.probe_indices(n, 12, 5) + [[1] * len(n), n]:
            assert _within(Q.element(c, ind), mp_element(c, ind), Q.n_ijk(c), Q.element_abs(c, ind))


@needs_mp
def test_bound_partner_is_the_sum_of_absolute_values():
    """B of a non-negative train with non-negative weights is the value itself; B of a mixed-sign one is at least |value|"""
    mp.dps = R.MP_DPS
    x, y, w, W = _small("d6")
    ax, ay, aw = [np.abs(c) for c in x], [np.abs(c) for c in y], [np.abs(q) for q in w]
    assert Q.dot_abs(x, y) == Q.dot(ax, ay) and Q.quad_abs(x, w) == Q.quad(ax, aw)
    assert Q.dot_abs(x, y) >= abs(Q.dot(x, y)) and Q.quad_abs(x, w) >= abs(Q.quad(x, w))
    assert np.all(Q.zquad_abs(x, W) >= np.abs(Q.zquad(x, W)) / np.sqrt(2.0))
    assert Q.element_abs(x, [1] * 6) == abs(Q.element(ax, [1] * 6))


def test_operation_counts():
    x, y = [np.zeros((1, 3, 2)), np.zeros((2, 5, 4)), np.zeros((4, 2, 1))], [np.zeros((1, 3, 3)), np.zeros((3, 5, 2)), np.zeros((2, 2, 1))]
    assert Q.n_dot(x, y) == (1 + 1 * 3) + (3 + 2 * 5) + (2 + 4 * 2)
    assert Q.n_dot(y, x) == (1 + 1 * 3) + (2 + 3 * 5) + (4 + 2 * 2)
    assert Q.n_quad(x) == (3 + 1) + (5 + 2) + (2 + 4)
    assert Q.n_zquad(x) == Q.n_quad(x) + 2 * 3
    assert Q.n_ijk(x) == 1 + 2 + 4 + 1


def test_check_wants_equality_where_the_bound_is_zero():
    Q.check("equal", 0.0, 0.0, 0.0)
    Q.check("inside", 1.0 + 2.0 ** -52, 1.0, 2.0 ** -52)
    with pytest.raises(AssertionError):
        Q.check("outside", 1.0 + 2.0 ** -51, 1.0, 2.0 ** -52)
    with pytest.raises(AssertionError):
        Q.check("bound 0", 1e-300, 0.0, 0.0)
    with pytest.raises(AssertionError):
        Q.check("nan", float("nan"), 0.0, 1.0)
    z = [np.zeros((1, 2, 2)), np.ones((2, 2, 1))]
    assert Q.quad_bound(z) == 0.0 and Q.dot_bound(z, z) == 0.0


# ---- seeded defects -----------------------------------------------------------------------------------------------------
def _rejected(tag, got, want, bound):
    with pytest.raises(AssertionError):
        Q.check("seeded: " + tag, got, want, bound)


def _drop_bond(cores, bond):
    """the last rank index of bond `bond` (1..d-1) dropped"""
    out = [c.copy() for c in cores]
    out[bond - 1] = out[bond - 1][:, :, :-1]
    out[bond] = out[bond][:-1]
    return out


def _drop_weight(w, k):
    out = [np.array(q, dtype=np.float64) for q in w]
    out[k][-1] = 0.0
    return out


def _drop_tail(cores, k, rows):
    """the last K % 4 terms of the inner product over (rank index, mode index) of core k dropped; rows: that product runs over
    the left rank only (K = r_(k-1), the product of phi with y's core / of a slice with the vector)"""
    out = [c.copy() for c in cores]
    c = out[k]
    if rows:
        m = c.shape[0] % 4
        assert m
        c[c.shape[0] - m:] = 0.0
    else:
        u = c.reshape(c.shape[0] * c.shape[1], c.shape[2], order="F").copy()
        m = u.shape[0] % 4
        assert m
        u[u.shape[0] - m:] = 0.0
        out[k] = u.reshape(c.shape, order="F")
    return out


def _wrong_ld(cy, ld):
    """core of y read with leading dimension ld instead of its own: element (b, j, c) taken from b + ld (j + n c)"""
    r0, n, r1 = cy.shape
    flat = cy.ravel(order="F")
    b, j, c = np.meshgrid(np.arange(r0), np.arange(n), np.arange(r1), indexing="ij")
    return flat[(b + ld * (j + n * c)) % flat.size]


PAIRS = [("A", "A'"), ("B", "B'"), ("C", "C'"), ("E64", "E64'")]


def _bonds(cores):
    """the bonds of rank above 1"""
    return [b for b in range(1, len(cores)) if cores[b].shape[0] > 1]


@pytest.mark.parametrize("nx,ny", PAIRS + [(b, a) for a, b in PAIRS])
def test_seeded_defects_of_dot_are_rejected(nx, ny):
    x, y = Q.train(nx), Q.train(ny)
    want, bound = Q.dot(x, y), Q.dot_bound(x, y)
    Q.check(f"dot {nx} {ny}", want, want, bound)
    for b in _bonds(x):
        _rejected(f"bond {b} of x", Q.dot(_drop_bond(x, b), y), want, bound)
    for b in _bonds(y):
        _rejected(f"bond {b} of y", Q.dot(x, _drop_bond(y, b)), want, bound)
    seen = 0
    for k in range(len(x)):
        if y[k].shape[0] % 4:                                    # first product of core k: K = ry0
            _rejected(f"tail of K = ry0, core {k + 1}", Q.dot(x, _drop_tail(y, k, True)), want, bound)
            seen += 1
        if (x[k].shape[0] * x[k].shape[1]) % 4:                  # second: K = rx0 n
            _rejected(f"tail of K = rx0 n, core {k + 1}", Q.dot(_drop_tail(x, k, False), y), want, bound)
            seen += 1
        if x[k].shape[0] != y[k].shape[0] and y[k].shape[1] * y[k].shape[2] > 1:     # y's core read with x's leading dimension
            bad = [c.copy() for c in y]                          # (a core of one column is read the same with any)
            bad[k] = _wrong_ld(y[k], x[k].shape[0])
            _rejected(f"leading dimension of x for y, core {k + 1}", Q.dot(x, bad), want, bound)
            seen += 1
    assert seen >= 3


@pytest.mark.parametrize("name,nonneg", [(nm, False) for nm in ("A", "A'", "B", "B'", "C", "C'", "E64", "E64'", "F97", "F98", "F128", "Z71")] +
                         [(nm, True) for nm in ("A", "A'", "E64", "E64'", "F98")])       # the non-negative twins of the device tests
def test_seeded_defects_of_quad_and_zquad_are_rejected(name, nonneg):
    c, w = Q.train(name, nonneg), Q.weights(name, 0, nonneg)
    n = Q.modes(c)
    want, bound = Q.quad(c, w), Q.quad_bound(c, w)
    for k in range(len(c)):
        _rejected(f"quad {name}: last weight of mode {k + 1}", Q.quad(c, _drop_weight(w, k)), want, bound)
    for b in _bonds(c):
        _rejected(f"quad {name}: bond {b}", Q.quad(_drop_bond(c, b), w), want, bound)
    if nonneg:
        return
    W = Q.zweights(name, 2)
    zwant, zbound = Q.zquad(c, W), Q.zquad_bound(c, W)
    off = np.concatenate([[0], np.cumsum(n)])
    for k in range(len(c)):
        bad = W.copy()
        bad[:, off[k + 1] - 1] = 0.0
        _rejected(f"zquad {name}: last weight of mode {k + 1}", Q.zquad(c, bad), zwant, zbound)
        bad = W.copy()
        blk = W[:, off[k]:off[k + 1]]
        bad[:, off[k]:off[k + 1]] = blk.imag + 1j * blk.real
        _rejected(f"zquad {name}: re and im of mode {k + 1} swapped", Q.zquad(c, bad), zwant, zbound)
        if k >= 1 and off[k] != k * n[0] and k * n[0] + n[k] <= off[-1]:      # offset of mode k formed as k n_1
            bad = W.copy()
            bad[:, off[k]:off[k + 1]] = W[:, k * n[0]:k * n[0] + n[k]]
            _rejected(f"zquad {name}: offset of mode {k + 1} from n_1", Q.zquad(c, bad), zwant, zbound)
        if k >= 2 and off[k] != n[0]:                                            # ... or as n_1 itself
            bad = W.copy()
            bad[:, off[k]:off[k + 1]] = W[:, n[0]:n[0] + n[k]]
            _rejected(f"zquad {name}: offset of mode {k + 1} is n_1", Q.zquad(c, bad), zwant, zbound)
    for b in _bonds(c):
        _rejected(f"zquad {name}: bond {b}", Q.zquad(_drop_bond(c, b), W), zwant, zbound)


def test_seeded_defects_on_the_long_chain_need_the_non_negative_twin():
    """d = 300, rank 2: on the mixed-sign train B exceeds |value| by many orders (the bound only guards against a blow-up);
    on its non-negative twin B is the value and a dropped weight or rank index is far outside the bound"""
    c, y, w = Q.train("L", True), Q.train("L'", True), Q.weights("L", 0, True)
    want, bound = Q.quad(c, w), Q.quad_bound(c, w)
    assert np.isfinite(want) and 0 < bound < 1e-11 * want
    for k in (0, 150, 299):
        _rejected(f"quad L: last weight of mode {k + 1}", Q.quad(c, _drop_weight(w, k)), want, bound)
    for b in (1, 150, 299):
        _rejected(f"quad L: bond {b}", Q.quad(_drop_bond(c, b), w), want, bound)
    want, bound = Q.dot(c, y), Q.dot_bound(c, y)
    assert np.isfinite(want) and 0 < bound < 1e-11 * want
    for b in (1, 150, 299):
        _rejected(f"dot L: bond {b} of y", Q.dot(c, _drop_bond(y, b)), want, bound)
        _rejected(f"dot L: tail of K = ry0 at core {b + 1}", Q.dot(c, _drop_tail(y, b, True)), want, bound)
    for name in ("L", "L'"):                                  # the mixed-sign values and bounds stay inside the double range
        m = Q.train(name)
        assert np.isfinite(Q.quad_abs(m, Q.weights("L"))) and np.isfinite(Q.dot_abs(m, m)) and Q.quad(m, Q.weights("L")) != 0.0


@pytest.mark.parametrize("name", ["A", "B", "E64", "F128"])
def test_seeded_defects_of_the_element_are_rejected(name):
    c = Q.train(name)
    n = Q.modes(c)
    inds = R.probe_indices(n, 6, 3) + [[1] * len(n), n]
    want = np.array([Q.element(c, i) for i in inds])
    bound = np.array([Q.element_bound(c, i) for i in inds])
    for b in _bonds(c):
        _rejected(f"tijk {name}: bond {b}", np.array([Q.element(_drop_bond(c, b), i) for i in inds]), want, bound)
    seen = 0
    for k in range(1, len(c)):                                   # the step through core k has K = r_k, the rows of core k + 1
        if c[k].shape[0] % 4:
            _rejected(f"tijk {name}: tail of K = r_{k}", np.array([Q.element(_drop_tail(c, k, True), i) for i in inds]), want, bound)
            seen += 1
    assert seen
    # the slice taken with the wrong leading dimension (r0 instead of r0 n): index j read as j r0 / (r0 n) of the way
    for k in range(len(c)):
        if n[k] > 1 and c[k].shape[0] > 1:
            bad = [a.copy() for a in c]
            bad[k] = _wrong_ld(c[k], 1)
            _rejected(f"tijk {name}: leading dimension, core {k + 1}", np.array([Q.element(bad, i) for i in inds]), want, bound)
