"""Reference for ttx_basis_batch / ttx_basis_tab, numpy float64 only (test side).

chain restates the definition of include/ttx.h.  phis[m] is the table of mode m + 1, shape (npts, n_m).  From the last mode to the
first: x = (1); t_j(a) = sum_k U(a, j, k) x(k), from 0.0 over ascending k; z(a) = sum_j phi_j t_j(a), from 0.0 over ascending j;
x = z; the value is z(1) after mode 1.  numpy's elementwise * and + round once each, so this is the operation sequence of
TTX_EVAL_EXACT.  abs_chain is the same on |U| and |phi|: B, the sum of the absolute values of all terms of the value.

Bound.  One step forms, per row a, the sum of the n_i r_i triple products phi_j U(a, j, k) x(k) (r_i the right rank of core i).
In any order, fused or not, a product meets at most 2 roundings of its two multiplications and at most n_i r_i - 1 roundings of the
additions on its path to the result: at most n_i r_i + 1 roundings, each a factor (1 + delta), |delta| <= u = 2^-53, so the step
stays within ((1 + u)^(n_i r_i + 1) - 1) S <= (n_i r_i + 2) u S of the true value of its inputs, S the same sum on absolute values
(first-order constant rounded up by one u, which covers the higher-order terms for n_i r_i u << 1).  The errors of the incoming x
pass through the next steps linearly and meet the same factors, so over the chain the factors multiply:
|computed - true| <= N u B with N = count(cores) = sum_i (n_i r_i + 2).  Two evaluations in different orders differ by at most
2 N u B.  For a train and tables without negative entries B is the value itself: the bound is 2 N u relative, and a dropped tile
or term shows.

cos_table and linear_table restate the two built-in kinds (include/ttx.h); cos_table takes the cosine as an argument, so that it
can be evaluated with the library's own ttx_cos (bit for bit) or with another one."""
import numpy as np

U = 2.0 ** -53
PI = 3.14159265358979323846        # TTX_COSCOEFF_PI
TRIG_MAX = 2.0 ** 19               # TTX_TRIG_MAX


def chain(cores, phis):
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    phis = [np.asarray(p, dtype=np.float64) for p in phis]
    assert len(cores) == len(phis)
    npts = phis[0].shape[0]
    x = np.ones((npts, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for c, ph in zip(cores[::-1], phis[::-1]):
            r0, n, r1 = c.shape
            assert ph.shape == (npts, n) and x.shape == (npts, r1)
            z = np.zeros((npts, r0))
            for j in range(n):
                t = np.zeros((npts, r0))
                for k in range(r1):
                    t = t + c[None, :, j, k] * x[:, k, None]
                z = z + ph[:, j, None] * t
            x = z
    assert x.shape == (npts, 1)
    return x[:, 0].copy()


def abs_chain(cores, phis):
    return chain([np.abs(np.asarray(c, dtype=np.float64)) for c in cores], [np.abs(np.asarray(p, dtype=np.float64)) for p in phis])


def count(cores):
    """N of the bound: sum_i (n_i r_i + 2), r_i the right rank of core i"""
    return sum(c.shape[1] * c.shape[2] + 2 for c in cores)


def bound(cores, phis):
    """2 N u B: what two evaluations of the chain in different summation orders may differ by"""
    return 2.0 * count(cores) * U * abs_chain(cores, phis)


def cos_table(a, b, n, x, halve_first=False, cos=np.cos):
    """phi[p, j] = c_j cos(arg), arg = (double)j * ((x - a) * w), w = PI / (b - a); NaN where |arg| > 2^19 or not finite"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    w = PI / (np.float64(b) - np.float64(a))
    with np.errstate(invalid="ignore", over="ignore"):
        y = (x - np.float64(a)) * w
        arg = np.arange(n, dtype=np.float64)[None, :] * y[:, None]
        ok = np.abs(arg) <= TRIG_MAX           # False for NaN
        phi = np.full(arg.shape, np.nan)
        if ok.any():
            phi[ok] = cos(np.ascontiguousarray(arg[ok]))
    if halve_first:
        phi[:, 0] = phi[:, 0] * 0.5
    return phi


def linear_table(nodes, x):
    """hat functions on strictly ascending nodes, the rows of include/ttx.h"""
    t = np.asarray(nodes, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    n = t.size
    phi = np.zeros((x.size, n))
    for p, v in enumerate(x):
        if np.isnan(v):
            phi[p, :] = np.nan
        elif n == 1 or v <= t[0]:
            phi[p, 0] = 1.0
        elif v >= t[n - 1]:
            phi[p, n - 1] = 1.0
        else:
            i = int(np.searchsorted(t, v, side="right")) - 1        # the last node with t_i <= v
            lam = (v - t[i]) / (t[i + 1] - t[i])
            phi[p, i + 1] = lam
            phi[p, i] = 1.0 - lam
    return phi


def unit_tables(n, ind):
    """unit-vector tables of the 1-based index rows ind (npts, d)"""
    ind = np.asarray(ind)
    return [np.eye(int(nk))[ind[:, k] - 1] for k, nk in enumerate(n)]


def hstack(phis):
    return np.ascontiguousarray(np.hstack(phis))
