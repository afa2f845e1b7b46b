"""Reference for ttx_mode_apply, numpy float64 only (test side).

apply_cores restates the definition of include/ttx.h: an applied mode k gets G'_k(a, j, b) = sum_i A_k[j, i] G_k(a, i, b), the sum
over ascending i from 0.0 with a separate multiply and add (the operation sequence of TTX_EVAL_EXACT: numpy's elementwise * and +
round once each); an untouched core is a copy.  abs_cores is the same on |A| and |G|: S(a, j, b) = sum_i |A_k[j, i]| |G_k(a, i, b)|.
Core-level bound: any order of the n_k products and sums of one element, fused or not, stays within (n_k + 1) u S of the true
value (u = 2^-53: at most n_k + 1 roundings on every path from a product to the result, first-order constants rounded up), so two
such evaluations differ by at most 2 (n_k + 1) u S, and are equal where S = 0.
Element-level bound: an element of the new train is a product of d matrices whose entries are, for an applied mode, sums of n_k
products; count gives N = sum_(k=0..d) (r_k + 1) + sum_(applied k) (n_k + 1), the counting of contract_ref.count, and
|computed - true| <= N u B with B the element of the train of abs_cores."""
import numpy as np

U = 2.0 ** -53


def _mats(cores, mats):
    if isinstance(mats, dict):
        mats = [mats.get(k) for k in range(1, len(cores) + 1)]
    assert len(mats) == len(cores)
    return [None if a is None else np.asarray(a, dtype=np.float64) for a in mats]


def apply_cores(cores, mats):
    out = []
    for g, a in zip(cores, _mats(cores, mats)):
        g = np.asarray(g, dtype=np.float64)
        if a is None:
            out.append(g.copy())
            continue
        assert a.ndim == 2 and a.shape[1] == g.shape[1]
        acc = np.zeros((g.shape[0], a.shape[0], g.shape[2]))
        for i in range(g.shape[1]):
            acc = acc + a[None, :, i, None] * g[:, None, i, :]
        out.append(acc)
    return out


def abs_cores(cores, mats):
    return apply_cores([np.abs(np.asarray(g, dtype=np.float64)) for g in cores], [None if a is None else np.abs(a) for a in _mats(cores, mats)])


def count(cores, mats):
    """N of the element-level bound"""
    r = [cores[0].shape[0]] + [c.shape[2] for c in cores]
    return sum(rk + 1 for rk in r) + sum(c.shape[1] + 1 for c, a in zip(cores, _mats(cores, mats)) if a is not None)
