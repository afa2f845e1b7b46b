"""Reference and derived bounds for the full reductions of a resident train: ttx_dot, ttx_quad, ttx_zquad, ttx_ijk (test side).

Plain numpy float64 / complex128, no device, no ctypes, nothing from oracle/.  Cores U_k have shape (r_(k-1), n_k, r_k).  Every
quantity comes with a bound partner B -- the same quantity on |cores| and |w| (complex weights: |Re w| + |Im w|) -- and an
operation count N, and the tolerance of a comparison is 2 N u B with u = 2^-53, exact equality where B = 0.

Derivation of N (derived, not measured).  A length-K inner product, in any order of the additions and with or without fused
multiply-add, obeys |computed - true| <= gamma_K sum |a||b|, gamma_K = K u / (1 - K u); a chain of inner products whose operands
are themselves computed accumulates gamma_(sum K) on the same chain of absolute values (componentwise bound of a product of
matrices).  gamma_N is N u to first order and N u < 1e-11 for every train used here, so N u is written for it.  The inner-product
lengths of the kernels, which the functions below repeat in the same grouping:
  dot      per core k: phi (rx_(k-1) x ry_(k-1)) times y's core, K = ry_(k-1), then x's core transposed times that, K = rx_(k-1) n_k:
           N_dot = sum_k (ry_(k-1) + rx_(k-1) n_k)
  quad     per core k: the weighted sum over the mode, K = n_k, then the chain step, K = r_(k-1):
           N_quad = sum_k (n_k + r_(k-1))            (any parenthesisation of the chain -- k_quad_tree -- has the same sum)
  element  one matrix-vector step per bond, K = r_k; counted over k = 0..d so that it covers the right-to-left order of ttx_ijk
           and the left-to-right order of the reference alike:  N_ijk = sum_(k=0..d) r_k
  zquad    the build forms the real and the imaginary sum separately, each an inner product of length n_k.  A chain step forms,
           per term, two products, one add or subtract of them and one accumulation, c = c + (br ar - bi ai): the term carries
           gamma_2 on |br ar| + |bi ai|, the accumulation over r_(k-1) terms another gamma_(r_(k-1)).  With s(z) = |Re z| + |Im z|,
           s(ab) <= s(a) s(b) and s(a + b) <= s(a) + s(b), so EACH COMPONENT of the result is within N_zquad u B of the truth,
           N_zquad = sum_k (n_k + r_(k-1) + 2),  B = quad(|cores|, |Re w| + |Im w|).
           The modulus of a complex number is at most sqrt(2) times its larger component: the bound on the modulus is
           sqrt(2) N_zquad u B per side, 2 sqrt(2) N_zquad u B between device and reference (zquad_bound).
Both sides, device and reference, are within N u B of the truth, hence |got - want| <= 2 N u B.

The trains of the device tests are listed here (SHAPES) so that tests/test_reductions_ref_cpu.py seeds its defects at the very
shapes tests/test_gpu_reductions.py runs."""
import math

import numpy as np

import tt_ref as R

U = 2.0 ** -53

# name -> (n, r); a primed name shares its modes with the unprimed one
SHAPES = {
    "A": ([3, 5, 2, 7, 4, 6], [1, 3, 17, 15, 16, 5, 1]),
    "A'": ([3, 5, 2, 7, 4, 6], [1, 2, 5, 33, 63, 7, 1]),
    "B": ([4, 1, 6, 1, 5, 3], [1, 3, 5, 1, 4, 2, 1]),            # modes of size 1, a rank-1 interior bond
    "B'": ([4, 1, 6, 1, 5, 3], [1, 6, 2, 7, 1, 3, 1]),
    "C": ([2, 3], [1, 2, 1]),                                     # d = 2
    "C'": ([2, 3], [1, 3, 1]),
    "E64": ([3] * 5, [1, 3, 64, 65, 3, 1]),
    "E64'": ([3] * 5, [1, 3, 63, 66, 3, 1]),
    "F97": ([2, 2, 2], [1, 2, 97, 1]),                            # quad: the last maxrank whose chain runs in LDS
    "F98": ([2, 2, 2], [1, 2, 98, 1]),                            # quad: the first that runs in global scratch
    "F128": ([2, 2, 2], [1, 2, 128, 1]),
    "L": ([2] * 300, [1] + [2] * 299 + [1]),
    "L'": ([2] * 300, [1] + [2] * 299 + [1]),
    "Z71": ([2, 3, 2], [1, 71, 71, 1]),                           # zquad: the largest maxrank the chain's LDS takes
    "Z72": ([2, 3, 2], [1, 72, 72, 1]),
}


def train(name, nonneg=False):
    """the train of SHAPES[name] (tt_ref.rand_train, mixed sign); nonneg: its non-negative twin, |cores|"""
    n, r = SHAPES[name]
    cores = R.rand_train(1000 + sum(map(ord, name)), n, r)
    return [np.abs(c) for c in cores] if nonneg else cores


def weights(name, seed=0, nonneg=False):
    """per-mode weight vectors for SHAPES[name], mixed sign and mixed magnitude"""
    rng = np.random.default_rng(2000 + sum(map(ord, name)) + seed)
    w = [rng.standard_normal(int(k)) * 2.0 ** rng.integers(-3, 4, int(k)) for k in SHAPES[name][0]]
    return [np.abs(q) for q in w] if nonneg else w


def zweights(name, nf, seed=0):
    """(nf, sum n) complex weights exp(i theta) rho, theta uniform, rho of mixed magnitude"""
    rng = np.random.default_rng(3000 + sum(map(ord, name)) + seed)
    sn = int(sum(SHAPES[name][0]))
    return np.exp(1j * rng.uniform(0.0, 2.0 * math.pi, (nf, sn))) * 2.0 ** rng.uniform(-3.0, 3.0, (nf, sn))


def ranks(cores):
    return [cores[0].shape[0]] + [c.shape[2] for c in cores]


def modes(cores):
    return [c.shape[1] for c in cores]


def _f64(cores):
    return [np.asarray(c, dtype=np.float64) for c in cores]


def _abs(cores):
    return [np.abs(c) for c in _f64(cores)]


def _ones(cores):
    return [np.ones(c.shape[1]) for c in cores]


def split(cores, flat):
    """a concatenated weight block (..., sum n) as per-mode pieces"""
    return np.split(np.asarray(flat), np.cumsum(modes(cores))[:-1], axis=-1)


# ---- dot ------------------------------------------------------------------------------------------------------------
def dot(x, y):
    """<x, y> by the interface recurrence of dtt_dot: phi <- U_x^T (phi U_y) core by core"""
    phi = np.ones((1, 1))
    for cx, cy in zip(_f64(x), _f64(y)):
        t = np.einsum("ab,bjc->ajc", phi, cy)                  # K = ry0
        phi = np.einsum("ajd,ajc->dc", cx, t)                  # K = rx0 n
    return float(phi[0, 0])


def dot_abs(x, y):
    return dot(_abs(x), _abs(y))


def n_dot(x, y):
    return sum(cy.shape[0] + cx.shape[0] * cx.shape[1] for cx, cy in zip(x, y))


def dot_bound(x, y):
    return 2.0 * n_dot(x, y) * U * dot_abs(x, y)


# ---- quad -----------------------------------------------------------------------------------------------------------
def quad(cores, w=None):
    """sum_i A(i) prod_k w_k(i_k); w None: weights of ones"""
    cores = _f64(cores)
    v = np.ones((1, 1))
    for c, q in zip(cores, _ones(cores) if w is None else w):
        v = v @ np.einsum("ajb,j->ab", c, np.asarray(q, dtype=np.float64).ravel())
    return float(v[0, 0])


def quad_abs(cores, w=None):
    return quad(_abs(cores), None if w is None else [np.abs(np.asarray(q, dtype=np.float64)) for q in w])


def n_quad(cores):
    return sum(c.shape[1] + c.shape[0] for c in cores)


def quad_bound(cores, w=None):
    return 2.0 * n_quad(cores) * U * quad_abs(cores, w)


# ---- zquad ----------------------------------------------------------------------------------------------------------
def zquad(cores, W):
    """complex128 chain; W (nf, sum n) -> nf values"""
    cores = _f64(cores)
    W = np.atleast_2d(np.asarray(W, dtype=np.complex128))
    out = np.zeros(W.shape[0], dtype=np.complex128)
    for f in range(W.shape[0]):
        v = np.ones((1, 1), dtype=np.complex128)
        for c, q in zip(cores, split(cores, W[f])):
            v = v @ np.einsum("ajb,j->ab", c.astype(np.complex128), q)
        out[f] = v[0, 0]
    return out


def zquad_abs(cores, W):
    """B per weight set: quad on |cores| and |Re w| + |Im w|"""
    W = np.atleast_2d(np.asarray(W, dtype=np.complex128))
    s = np.abs(W.real) + np.abs(W.imag)
    return np.array([quad(_abs(cores), split(cores, s[f])) for f in range(W.shape[0])])


def n_zquad(cores):
    return sum(c.shape[1] + c.shape[0] + 2 for c in cores)


def zquad_bound(cores, W):
    """on the modulus |got - want|: sqrt(2) takes the bound of a component to the modulus"""
    return 2.0 * math.sqrt(2.0) * n_zquad(cores) * U * zquad_abs(cores, W)


# ---- element --------------------------------------------------------------------------------------------------------
def element(cores, ind):
    """A(ind), ind 1-based"""
    return R.element(_f64(cores), [int(j) for j in ind])


def element_abs(cores, ind):
    return R.element(_abs(cores), [int(j) for j in ind])


def n_ijk(cores):
    return sum(ranks(cores))


def element_bound(cores, ind):
    return 2.0 * n_ijk(cores) * U * element_abs(cores, ind)


# ---- the comparison -------------------------------------------------------------------------------------------------
def check(tag, got, want, bound):
    """|got - want| <= bound everywhere (the modulus, for complex values), equal where the bound is 0; prints max |diff| / bound"""
    got, want, bound = np.atleast_1d(got), np.atleast_1d(want), np.atleast_1d(np.asarray(bound, dtype=np.float64))
    diff = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, diff / bound, np.where(diff == 0, 0.0, np.inf))
    print(tag, "max |diff| / bound", float(ratio.max()))
    assert np.all(np.isfinite(got)), tag
    assert np.all(np.isfinite(bound)), tag
    assert np.all(diff <= bound), (tag, float(ratio.max()))
    assert np.array_equal(got[bound == 0], want[bound == 0]), tag
    return float(ratio.max())
