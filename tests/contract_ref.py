"""Reference for ttx_contract / ttx_marginals, numpy float64 only (test side).

contract_cores restates the definition of include/ttx.h: kept modes k_1 < ... < k_m; M_k = sum_i w_k(i) G_k(:, i, :) for a
contracted mode; new core j = P_j G_(k_j) with P_j the ordered product of the M_k between k_(j-1) and k_j; the M_k after k_m
go into the last new core from the right.  abs_bound is the same contraction on |cores| and |w|: with
N = sum_(k=0..d) (r_k + 1) + sum_(contracted k) (n_k + 1) every order of the sums and products obeys
|computed - true| <= N 2^-53 B elementwise (componentwise bound of a product of matrices whose entries are sums)."""
import numpy as np

import tt_ref as R

U = 2.0 ** -53


def _weights(cores, w):
    if w is None:
        return [np.ones(c.shape[1]) for c in cores]
    return [np.asarray(q, dtype=np.float64).ravel() for q in w]


def contract_cores(cores, keep, w=None):
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    keep = [int(k) for k in keep]
    w = _weights(cores, w)
    out, p = [], None
    for c, kp, q in zip(cores, keep, w):
        if kp:
            out.append(c.copy() if p is None else np.einsum("ab,bjc->ajc", p, c))
            p = None
        else:
            m = np.einsum("ajb,j->ab", c, q)
            p = m if p is None else p @ m
    if p is not None:                       # the run after the last kept mode
        out[-1] = np.einsum("ajb,bc->ajc", out[-1], p)
    return out


def abs_bound(cores, keep, w=None):
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    return contract_cores([np.abs(c) for c in cores], keep, [np.abs(q) for q in _weights(cores, w)])


def ranks(cores):
    return [cores[0].shape[0]] + [c.shape[2] for c in cores]


def stated_ranks(cores, keep):
    """r'(0) = 1, r'(j) = r(k_j) for j < m, r'(m) = 1"""
    r = ranks(cores)
    kept = [k for k, kp in enumerate(keep) if kp]
    return [1] + [r[k + 1] for k in kept[:-1]] + [1]


def count(cores, keep):
    """N of the bound"""
    return sum(rk + 1 for rk in ranks(cores)) + sum(c.shape[1] + 1 for c, kp in zip(cores, keep) if not kp)


def elements(cores, ind):
    return np.array([R.element(cores, row) for row in ind])


def marginals(cores, w=None):
    """block k (i) = the train summed over every other mode against its weights"""
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    w = _weights(cores, w)
    ms = [np.einsum("ajb,j->ab", c, q) for c, q in zip(cores, w)]
    d = len(cores)
    left, right = [np.ones((1, 1))], [np.ones((1, 1))]
    for k in range(d - 1):
        left.append(left[-1] @ ms[k])
    for k in range(d - 1, 0, -1):
        right.append(ms[k] @ right[-1])
    right = right[::-1]                     # right[k] = M_(k+1) ... M_(d-1) (0-based), right[d-1] = [1]
    return [np.einsum("a,ajb,b->j", left[k][0], cores[k], right[k][:, 0]) for k in range(d)]


def marginals_abs(cores, w=None):
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    return marginals([np.abs(c) for c in cores], [np.abs(q) for q in _weights(cores, w)])
