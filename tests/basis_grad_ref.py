"""Reference for ttx_basis_grad_batch / ttx_basis_grad_tab, numpy float64 only (test side).

grad_chain restates the definition of include/ttx.h.  phis[m] and dphis[m] are the table and the derivative table of mode m + 1,
shape (npts, n_m).  Backward, from the last mode to the first: x = (1); t_j(a) = sum_k U(a, j, k) x(k), from 0.0 over ascending k;
z(a) = sum_j phi_j t_j(a) and e(a) = sum_j dphi_j t_j(a), from 0.0 over ascending j; D_i = e; x = z; val = z(1) after mode 1 -- the
operation sequence of basis_ref.chain.  Forward, from the first mode to the last: l = (1); grad_i = sum_a l(a) D_i(a), from 0.0 over
ascending a; s_j(k) = sum_a l(a) U(a, j, k), from 0.0 over ascending a; l(k) = sum_j phi_j s_j(k), from 0.0 over ascending j; the
last l is not formed.  numpy's elementwise * and + round once each, so this is the operation sequence of TTX_EVAL_EXACT.
abs_grad_chain is the same on |U|, |phi|, |dphi|: B_m, the sum of the absolute values of all terms of grad_m.

Bound.  grad_m is the sum, over all index tuples, of the terms  [prod_(i<m) phi U]  dphi_m U_m  [prod_(i>m) phi U]: the chain of
basis_ref with mode m's table replaced, split at the bond left of core m into l (modes before m) and D_m (modes from m on) and
joined by the dot product l . D_m over r_(m-1) <= rmax terms.  Follow one term.  Through a backward step of core i >= m it is
multiplied twice and joins a sum of n_i r_i terms: at most n_i r_i + 1 roundings in any order (basis_ref's count, r_i the right
rank), i.e. with the first-order constant rounded up by one u, a factor within (n_i r_i + 2) u.  Through a forward step of core
i < m it is multiplied twice and joins a sum of n_i r_(i-1) terms: (n_i r_(i-1) + 2) u.  Every core is passed by exactly one of the
two, so the steps give at most sum_i (n_i max(r_(i-1), r_i) + 2) whatever m is.  The dot product adds one multiplication and at
most rmax - 1 additions: rmax roundings, rounded up by one: rmax + 1.  Errors of incoming states pass linearly through later steps
and meet the same factors, so
    |computed grad_m - true| <= N_g u B_m,   N_g = sum_i (n_i max(r_(i-1), r_i) + 2) + rmax + 1,
and two evaluations in different summation orders (exact against MFMA, the two-pass form against the substituted chain, whose own
count sum_i (n_i r_i + 2) is not larger) differ by at most 2 N_g u B_m.  For cores and tables without negative entries B_m is
grad_m itself: the bound is 2 N_g u relative, and a dropped tile or term shows.

dcos_table and dlinear_table restate the two built-in derivative tables; dcos_table takes the sine as an argument, so that it can be
evaluated with the library's own ttx_sin (bit for bit) or with another one."""
import numpy as np

from basis_ref import PI, TRIG_MAX, U  # noqa: F401


def grad_chain(cores, phis, dphis):
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    phis = [np.asarray(p, dtype=np.float64) for p in phis]
    dphis = [np.asarray(p, dtype=np.float64) for p in dphis]
    d = len(cores)
    assert len(phis) == d and len(dphis) == d
    npts = phis[0].shape[0]
    x = np.ones((npts, 1))
    D = [None] * d
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(d - 1, -1, -1):
            c, ph, dh = cores[i], phis[i], dphis[i]
            r0, n, r1 = c.shape
            assert ph.shape == (npts, n) and dh.shape == (npts, n) and x.shape == (npts, r1)
            z, e = np.zeros((npts, r0)), np.zeros((npts, r0))
            for j in range(n):
                t = np.zeros((npts, r0))
                for k in range(r1):
                    t = t + c[None, :, j, k] * x[:, k, None]
                z = z + ph[:, j, None] * t
                e = e + dh[:, j, None] * t
            D[i] = e
            x = z
        assert x.shape == (npts, 1)
        val = x[:, 0].copy()
        grad = np.zeros((npts, d))
        l = np.ones((npts, 1))
        for i in range(d):
            c, ph = cores[i], phis[i]
            r0, n, r1 = c.shape
            g = np.zeros(npts)
            for a in range(r0):
                g = g + l[:, a] * D[i][:, a]
            grad[:, i] = g
            if i == d - 1:
                break
            ln = np.zeros((npts, r1))
            for j in range(n):
                s = np.zeros((npts, r1))
                for a in range(r0):
                    s = s + l[:, a, None] * c[None, a, j, :]
                ln = ln + ph[:, j, None] * s
            l = ln
    return val, grad


def abs_grad_chain(cores, phis, dphis):
    """B_m for every m, shape (npts, d)"""
    return grad_chain([np.abs(np.asarray(c, dtype=np.float64)) for c in cores], [np.abs(np.asarray(p, dtype=np.float64)) for p in phis],
                      [np.abs(np.asarray(p, dtype=np.float64)) for p in dphis])[1]


def count(cores):
    """N_g of the bound: sum_i (n_i max(r_(i-1), r_i) + 2) + rmax + 1"""
    rmax = max(max(c.shape[0], c.shape[2]) for c in cores)
    return sum(c.shape[1] * max(c.shape[0], c.shape[2]) + 2 for c in cores) + rmax + 1


def bound(cores, phis, dphis):
    """2 N_g u B_m: what two evaluations of grad_m in different summation orders may differ by, shape (npts, d)"""
    return 2.0 * count(cores) * U * abs_grad_chain(cores, phis, dphis)


def substituted(phis, dphis, m):
    """the tables of the independent route to grad_m: mode m's table replaced by its derivative table"""
    return [dphis[k] if k == m else phis[k] for k in range(len(phis))]


def dcos_table(a, b, n, x, sin=np.sin):
    """dphi[p, j] = -((j w) sin(arg)), arg = (double)j * ((x - a) * w), w = PI / (b - a); 0.0 at j = 0; NaN where |arg| > 2^19 or
    not finite (j = 0 included)"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    w = PI / (np.float64(b) - np.float64(a))
    j = np.arange(n, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        y = (x - np.float64(a)) * w
        arg = j[None, :] * y[:, None]
        ok = np.abs(arg) <= TRIG_MAX           # False for NaN
        dphi = np.full(arg.shape, np.nan)
        if ok.any():
            jw = np.broadcast_to((j * w)[None, :], arg.shape)
            dphi[ok] = -(jw[ok] * sin(np.ascontiguousarray(arg[ok])))
    dphi[:, 0] = np.where(ok[:, 0], 0.0, np.nan)
    return dphi


def dlinear_table(nodes, x):
    """the derivative of the branch linear_table takes: the right-hand derivative at an interior node, 0 on and outside the ends"""
    t = np.asarray(nodes, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = t.size
    dphi = np.zeros((x.size, n))
    for p, v in enumerate(x):
        if np.isnan(v):
            dphi[p, :] = np.nan
        elif n == 1 or v <= t[0] or v >= t[n - 1]:
            pass
        else:
            i = int(np.searchsorted(t, v, side="right")) - 1        # the last node with t_i <= v
            s = 1.0 / (t[i + 1] - t[i])
            dphi[p, i + 1] = s
            dphi[p, i] = -s
    return dphi
