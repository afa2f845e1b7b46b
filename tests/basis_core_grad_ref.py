"""Reference for ttx_basis_core_grad_batch / ttx_basis_core_grad_tab and ttx_cores_axpy, numpy float64 only (test side).

core_grad_chain restates the definition of include/ttx.h.  phis[m] is the table of mode m + 1, shape (npts, n_m); c the weights,
shape (npts,).  Backward, from the last mode to the first, from X_d = (1): t_j(a) = sum_k U(a, j, k) X_i(k), from 0.0 over ascending
k; X_(i-1)(a) = sum_j phi_j t_j(a), from 0.0 over ascending j; val = X_0(1) -- the operation sequence of basis_ref.chain, every X_i
kept.  Forward, from the first mode to the last, from L_1 = (1): s_j(k) = sum_a L_i(a) U(a, j, k), from 0.0 over ascending a;
L_(i+1)(k) = sum_j phi_j s_j(k), from 0.0 over ascending j -- the forward step of basis_grad_ref.grad_chain; L_(d+1) is not formed.
Gradient: G_i(a, j, k) = G0_i(a, j, k) + sum_p ((c[p] * L_i(p, a)) * (phi_(i, j)(p) * X_i(p, k))), a plain loop over ascending p that
adds one term per element and step onto G0 (0.0, or g0).  numpy's elementwise * and + round once each, so this is the operation
sequence of TTX_EVAL_EXACT.  abs_core_grad is the same on |U|, |phi|, |c| (and |g0|): B_i, the sum of the absolute values of all
terms of G_i.

Bound.  G_i(a, j, k) is the sum over the points and over all index tuples of the other modes of the terms
c_p [prod_(m < i) phi U] phi_(i, j) [prod_(m > i) phi U].  Follow one term.  Through the forward step of a core m < i it is multiplied
twice and joins a sum of n_m r_(m-1) terms: at most n_m r_(m-1) + 1 roundings in any order, i.e. with the first-order constant
rounded up by one u, a factor within (n_m r_(m-1) + 2) u (basis_grad_ref's count of a forward step).  Through the backward step of a
core m > i it is multiplied twice and joins a sum of n_m r_m terms: (n_m r_m + 2) u (basis_ref's count).  Core i itself is not
passed.  The three multiplies of the gradient's term add 3 roundings.  The sum over the points, whatever its tree -- the plain
loop, the four-point groups of an MFMA, segments whose partial blocks are added afterwards, chunks, a second call that accumulates
-- has P + 1 leaves with G0, so a leaf passes at most P additions: P roundings.  3 + P, rounded up by one u for the higher-order
terms: P + 4.  Errors of incoming states pass linearly through later steps and meet the same factors, so
    |computed G_i - true| <= N_i u B_i,   N_i = sum_(m < i) (n_m r_(m-1) + 2) + sum_(m > i) (n_m r_m + 2) + P + 4,
and two evaluations in different summation orders (exact against MFMA) differ by at most 2 N_i u B_i.  For cores, tables and
weights without negative entries B_i is G_i itself: the bound is 2 N_i u relative, and a dropped tile, point group or partial block
shows.

Linearity.  f is linear in core i, so for any block E of its shape sum_p c_p f_(U_i <- E)(x_p) = <G_i, E>.  identity_allowance
bounds the difference of the two computed sides: the left side is P values of basis_ref.chain (N u B each, N = basis_ref.count)
weighted and summed (P + 1 more roundings, rounded up: P + 2), the right side a dot product of size_i terms (size_i + 1) of a G_i
that carries N_i u B_i; both sums of absolute values equal A = <B_i, |E|> up to rounding, and each side is given twice its
first-order bound, as everywhere in these references:  2 (N + P + 2) u A_left + 2 (N_i + size_i + 1) u A_right."""
import numpy as np

import basis_ref as B
from basis_ref import U  # noqa: F401


def states(cores, phis):
    """X[i] (npts, r_i), i = 0 .. d (X[d] = (1), X[0][:, 0] = val) and L[i] (npts, r_i), i = 0 .. d-1 (L[0] = (1))"""
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    phis = [np.asarray(p, dtype=np.float64) for p in phis]
    d = len(cores)
    assert len(phis) == d
    npts = phis[0].shape[0]
    X = [None] * (d + 1)
    X[d] = np.ones((npts, 1))
    L = [None] * d
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(d - 1, -1, -1):
            c, ph = cores[i], phis[i]
            r0, n, r1 = c.shape
            assert ph.shape == (npts, n) and X[i + 1].shape == (npts, r1)
            z = np.zeros((npts, r0))
            for j in range(n):
                t = np.zeros((npts, r0))
                for k in range(r1):
                    t = t + c[None, :, j, k] * X[i + 1][:, k, None]
                z = z + ph[:, j, None] * t
            X[i] = z
        assert X[0].shape == (npts, 1)
        L[0] = np.ones((npts, 1))
        for i in range(d - 1):
            c, ph = cores[i], phis[i]
            r0, n, r1 = c.shape
            ln = np.zeros((npts, r1))
            for j in range(n):
                s = np.zeros((npts, r1))
                for a in range(r0):
                    s = s + L[i][:, a, None] * c[None, a, j, :]
                ln = ln + ph[:, j, None] * s
            L[i + 1] = ln
    return X, L


def core_grad_chain(cores, phis, c, g0=None):
    """(val, [G_1 .. G_d]): the definition, the points added one by one in ascending order onto g0 (a list of blocks) or 0.0"""
    cores = [np.asarray(u, dtype=np.float64) for u in cores]
    phis = [np.asarray(p, dtype=np.float64) for p in phis]
    c = np.asarray(c, dtype=np.float64)
    d, npts = len(cores), phis[0].shape[0]
    assert c.shape == (npts,)
    X, L = states(cores, phis)
    G = [np.zeros(u.shape) if g0 is None else np.array(g0[i], dtype=np.float64) for i, u in enumerate(cores)]
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(d):
            assert G[i].shape == cores[i].shape
            g = G[i]
            cl = c[:, None] * L[i]                                      # (c[p] * L_i(p, a))
            for p in range(npts):
                g = g + cl[p][:, None, None] * (phis[i][p][None, :, None] * X[i + 1][p][None, None, :])
            G[i] = g
    return X[0][:, 0].copy(), G


def abs_core_grad(cores, phis, c, g0=None):
    """B_i for every core"""
    return core_grad_chain([np.abs(np.asarray(u, dtype=np.float64)) for u in cores], [np.abs(np.asarray(p, dtype=np.float64)) for p in phis],
                           np.abs(np.asarray(c, dtype=np.float64)), None if g0 is None else [np.abs(np.asarray(g, dtype=np.float64)) for g in g0])[1]


def count(cores, i, npts):
    """N_i of the bound (i 0-based): sum_(m < i) (n_m r_(m-1) + 2) + sum_(m > i) (n_m r_m + 2) + P + 4"""
    return (sum(u.shape[1] * u.shape[0] + 2 for u in cores[:i]) + sum(u.shape[1] * u.shape[2] + 2 for u in cores[i + 1:]) + npts + 4)


def bound(cores, phis, c, g0=None):
    """2 N_i u B_i for every core: what two evaluations of G_i in different summation orders may differ by"""
    npts = np.asarray(phis[0]).shape[0]
    return [2.0 * count(cores, i, npts) * U * b for i, b in enumerate(abs_core_grad(cores, phis, c, g0))]


def replaced(cores, i, E):
    return [np.asarray(E, dtype=np.float64) if k == i else u for k, u in enumerate(cores)]


def identity_sides(cores, phis, c, i, E, G_i, chain=B.chain):
    """(sum_p c_p f_(U_i <- E)(x_p), <G_i, E>), both summed plainly in float64; chain: what evaluates the train"""
    left = float(np.sum(np.asarray(c, dtype=np.float64) * chain(replaced(cores, i, E), phis)))
    right = float(np.sum(np.asarray(G_i, dtype=np.float64) * np.asarray(E, dtype=np.float64)))
    return left, right


def identity_allowance(cores, phis, c, i, E, B_i):
    npts = np.asarray(phis[0]).shape[0]
    rep = replaced(cores, i, E)
    a_left = float(np.sum(np.abs(c) * B.abs_chain(rep, phis)))
    a_right = float(np.sum(B_i * np.abs(E)))
    return 2.0 * (B.count(rep) + npts + 2) * U * a_left + 2.0 * (count(cores, i, npts) + np.size(E) + 1) * U * a_right


def dense_longdouble(cores, phis, c):
    """every G_i of the definition by einsum in long double: the states by one contraction per core, then one over the points"""
    ld = np.longdouble
    cores = [np.asarray(u, dtype=np.float64).astype(ld) for u in cores]
    phis = [np.asarray(p, dtype=np.float64).astype(ld) for p in phis]
    c = np.asarray(c, dtype=np.float64).astype(ld)
    d, npts = len(cores), phis[0].shape[0]
    X = [None] * (d + 1)
    X[d] = np.ones((npts, 1), dtype=ld)
    for i in range(d - 1, -1, -1):
        X[i] = np.einsum("ajk,pj,pk->pa", cores[i], phis[i], X[i + 1])
    L = [np.ones((npts, 1), dtype=ld)]
    for i in range(d - 1):
        L.append(np.einsum("pa,ajk,pj->pk", L[i], cores[i], phis[i]))
    return [np.einsum("p,pa,pj,pk->ajk", c, L[i], phis[i], X[i + 1]) for i in range(d)]


# ---- the block-coordinate least-squares fit of the tests: loss = 1/2 sum_p (f(x_p) - y_p)^2, one core at a time, exact line search
FIT_N, FIT_R, FIT_NPTS, FIT_SWEEPS = [5, 6, 4], [1, 3, 2, 1], 200, 3


def hat_table(nodes, x):
    return B.linear_table(nodes, x)


def fit_problem():
    """the pinned inputs: the start train, hat-function tables at 200 points, targets from a second seeded train"""
    rng = np.random.default_rng(20240521)
    start = [rng.standard_normal((FIT_R[k], FIT_N[k], FIT_R[k + 1])) for k in range(3)]
    truth = [rng.standard_normal((FIT_R[k], FIT_N[k], FIT_R[k + 1])) for k in range(3)]
    x = rng.uniform(0.0, 1.0, (FIT_NPTS, 3))
    phis = [hat_table(np.linspace(0.0, 1.0, nk), x[:, k]) for k, nk in enumerate(FIT_N)]
    y = B.chain(truth, phis)
    return start, phis, y


def fit_step(G_i, f_dir):
    """the exact step along -G_i: with f_dir[p] = f_(U_i <- G_i)(x_p), alpha = <G_i, G_i> / sum_p f_dir[p]^2; U_i <- U_i + (-alpha) G_i.
    <G_i, G_i> is summed over the block in its packed (column-major) order, whatever the memory layout of the array that holds it:
    numpy's sum follows the layout, and the same block comes C-ordered from numpy and F-ordered from the engine"""
    g = np.ravel(np.asarray(G_i, dtype=np.float64), order="F").copy()
    alpha = float(np.sum(g * g)) / float(np.sum(f_dir * f_dir))
    return -alpha


def fit_loss(val, y):
    res = val - y
    return 0.5 * float(np.sum(res * res))


def fit_numpy(chain=B.chain):
    """the whole fit in numpy: the losses before every step and after the last, and the final cores"""
    cores, phis, y = fit_problem()
    cores = [u.copy() for u in cores]
    losses = []
    for _ in range(FIT_SWEEPS):
        for i in range(len(cores)):
            val, G = core_grad_chain(cores, phis, B.chain(cores, phis) - y)
            losses.append(fit_loss(val, y))
            f_dir = chain(replaced(cores, i, G[i]), phis)
            cores[i] = cores[i] + fit_step(G[i], f_dir) * G[i]
    losses.append(fit_loss(B.chain(cores, phis), y))
    return losses, cores
