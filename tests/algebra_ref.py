"""Reference for ttx_lincomb / ttx_hadamard, numpy float64 only (test side).  Cores have shape (r_(k-1), n_k, r_k).

lincomb_cores and hadamard_cores restate the layout of include/ttx.h.  Every element of a new core is a copy, a zero or one
rounded product, so the device's cores are compared with these BIT FOR BIT.

Bounds for comparisons of elements and sums (derived, not measured; u = 2^-53, gamma_N written as N u as in reduce_ref.py).
An element of a train read through a chain of matrix-vector steps obeys |computed - true| <= (sum_(k=0..d) r_k) u |train|(i)
(reduce_ref.n_ijk) when the cores are exact; a core whose entries carry one rounding each adds 1 per such core.
  lincomb   the chain over the NEW cores, whose first core carries the multiply by coef: N' = n_ijk(new) + 1.  The other side,
            sum_t c_t v_t with v_t the element of x_t by its own chain, carries n_ijk(x_t) <= n_ijk(new), one multiply and m - 1
            additions: at most n_ijk(new) + m.  Both are below
                N_lincomb = n_ijk(new) + m + 1,        B = sum_t |c_t| |x_t|(i) = the element of the train of |new cores|,
            and two values that are each within N u B of the truth differ by at most 2 N u B.
  hadamard  the chain over the new cores, every core carrying one multiply: n_ijk(new) + d.  The other side, the product of the
            two elements: n_ijk(x) + n_ijk(y) + 1 <= n_ijk(new) + (d + 1) + 1, because r_x + r_y <= r_x r_y + 1 on each of the
            d + 1 bonds.  Both are below
                N_hadamard = n_ijk(new) + d + 2,       B = |x|(i) |y|(i) = the element of the train of |new cores|.
  quad      the same with reduce_ref.n_quad (sum_k n_k + r_(k-1)) in the place of n_ijk:
                N_quad_lincomb = n_quad(new) + m + 1,  B = quad of the |new cores| against |w|.
Values are equal where B = 0."""
import numpy as np

import tt_ref as R

U = 2.0 ** -53


def _f64(cores):
    return [np.asarray(c, dtype=np.float64) for c in cores]


def ranks(cores):
    return [cores[0].shape[0]] + [c.shape[2] for c in cores]


def lincomb_ranks(trains):
    """r'(0) = r'(d) = 1, r'(k) = sum_t r_t(k) on interior bonds"""
    d = len(trains[0])
    return [1] + [sum(ranks(x)[k] for x in trains) for k in range(1, d)] + [1]


def hadamard_ranks(x, y):
    return [a * b for a, b in zip(ranks(x), ranks(y))]


def lincomb_cores(coefs, trains):
    """sum_t coefs[t] trains[t]: first cores side by side, each times its coefficient; interior cores block diagonal in term order
    with explicit zeros; last cores stacked"""
    trains = [_f64(x) for x in trains]
    d, rr = len(trains[0]), lincomb_ranks(trains)
    out = []
    for k in range(d):
        n = trains[0][k].shape[1]
        z = np.zeros((rr[k], n, rr[k + 1]))
        ro = co = 0
        for c, x in zip(coefs, trains):
            g = x[k]
            z[ro:ro + g.shape[0], :, co:co + g.shape[2]] = np.float64(c) * g if k == 0 else g
            if k > 0:
                ro += g.shape[0]
            if k < d - 1:
                co += g.shape[2]
        out.append(z)
    return out


def hadamard_cores(x, y):
    """Z[ib rx0 + ia, j, kb rx1 + ka] = X[ia, j, ka] Y[ib, j, kb]"""
    out = []
    for a, b in zip(_f64(x), _f64(y)):
        out.append(np.einsum("ajc,bjd->bajdc", a, b).reshape(b.shape[0] * a.shape[0], a.shape[1], b.shape[2] * a.shape[2]))
    return out


def lincomb_abs(coefs, trains):
    """the |.|-train of the bound: the same assembly on |coef| and |cores|"""
    return lincomb_cores([abs(float(c)) for c in coefs], [[np.abs(g) for g in _f64(x)] for x in trains])


def hadamard_abs(x, y):
    return hadamard_cores([np.abs(g) for g in _f64(x)], [np.abs(g) for g in _f64(y)])


def n_ijk(cores):
    return sum(ranks(cores))


def n_quad(cores):
    return sum(c.shape[1] + c.shape[0] for c in cores)


def n_lincomb(new, m):
    return n_ijk(new) + m + 1


def n_hadamard(new):
    return n_ijk(new) + len(new) + 2


def n_quad_lincomb(new, m):
    return n_quad(new) + m + 1


def elements(cores, ind):
    return np.array([R.element(cores, [int(j) for j in row]) for row in ind])


def dense(cores):
    """the full tensor of a small train (plain float64)"""
    t = _f64(cores)[0]
    for c in _f64(cores)[1:]:
        t = np.tensordot(t, c, axes=([t.ndim - 1], [0]))
    return t.reshape(t.shape[1:-1])


def check(tag, got, want, bound):
    """|got - want| <= bound everywhere, equal where the bound is 0; prints max |diff| / bound"""
    got, want, bound = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    diff = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf))
    print(tag, "values", got.size, "max |diff| / bound", float(ratio.max()))
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(bound)), tag
    assert np.all(diff <= bound), (tag, float(ratio.max()))
    assert np.array_equal(got[bound == 0], want[bound == 0]), tag
