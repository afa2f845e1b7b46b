"""Reference for ttx_topk (include/ttx.h), numpy float64 only (test side).

search(cores, K, which, fixed) restates the header's definition: the prefix Gram matrices P_k, the search from the last mode to the
first over the sheet of (candidate, index) pairs with the score sqrt(max(0, y^T P_(k-1) y)), the K largest kept in ascending flat
position with ties to the smaller position, bound_k = the largest score not kept, the rows by back-tracking and the final order
by `which` with ties to the lexicographically smaller row.  The x of a kept pair is summed over ascending b from 0.0 with a
separate multiply and add, the chain's own order, so val carries the bits of tijk_batch(ind, "exact").

The allowances (nothing here is measured on the code under test).  A squared score is a triple sum: s^2 = y^T P y with
y = G_k .. G_d along the suffix and P = P_(k-1) built from the cores 1 .. k-1.  One term of the expanded sum is a product of
core entries and reaches the result through
  * the suffix chain, twice (y enters on both sides): per bond j > k one multiply and r_j additions: 2 sum_j (r_j + 1);
  * the Gram chain: per step j < k the product W = P G (r_(j-1) additions and a multiply) and G^T W summed over the n_j indices
    and r_(j-1) rows (n_j r_(j-1) additions and a multiply): sum_j (n_j r_(j-1) + r_(j-1) + 2);
  * z = P y and y . z: 2 (r_(k-1) + 1).
N(cores) takes the sums over all bonds and the largest rank, so it covers every mode.  For every order of the sums (plain loops,
the matrix cores, numpy's einsum) |computed s^2 - true s^2| <= g B2 with g = 1.01 N 2^-53 and B2 the same expression on |cores|
(the N u B form of reduce_ref.py and sample_ref.py); device against reference is E = 2 g B2 on s^2.  The root: for a, b >= 0,
|sqrt(a) - sqrt(b)| <= min(sqrt|a - b|, |a - b| / sqrt(b)), and each root rounds once: with s the reference's score
    tol(s) = min(sqrt(E), E / s) + 2^-52 (s + sqrt(E)).
max(0, .) does not widen this (it moves a negative computed value towards the true one).  The bound is a maximum over the pairs not
kept, and |max a - max b| <= max |a - b| over the same pairs, so its allowance is the largest tol among the pairs not kept of all
modes.  A mode of a case is DECIDED when the gap between the K-th and the (K+1)-th largest reference score exceeds twice the
largest tol of the two: then every summation order keeps the same pairs."""
import numpy as np

U = 2.0 ** -53


def ranks(cores):
    return [cores[0].shape[0]] + [c.shape[2] for c in cores]


def count(cores):
    """N of the allowance"""
    r = ranks(cores)
    return (2 * sum(rk + 1 for rk in r) + sum(c.shape[1] * c.shape[0] + c.shape[0] + 2 for c in cores) + 2 * (max(r) + 1))


def dense(cores):
    """the full tensor of a small train"""
    t = np.asarray(cores[0], dtype=np.float64)
    for c in cores[1:]:
        t = np.tensordot(t, c, axes=([t.ndim - 1], [0]))
    return t[0, ..., 0]


def _index_sets(cores, fixed):
    d = len(cores)
    fixed = [0] * d if fixed is None else [int(f) for f in fixed]
    return [np.arange(c.shape[1]) if not f else np.array([f - 1]) for c, f in zip(cores, fixed)]


def grams(cores, I):
    """P_0 .. P_(d-1)"""
    P = [np.ones((1, 1))]
    for c, idx in zip(cores[:-1], I):
        g = c[:, idx, :]
        P.append(np.tensordot(g, np.tensordot(P[-1], g, axes=(1, 0)), axes=([0, 1], [0, 1])))
    return P


def _sheet(c, idx, X):
    """Y[cand, i, a] = sum_b G(a, i, b) X[cand, b], ascending b from 0.0, separate multiply and add"""
    g = c[:, idx, :]
    Y = np.zeros((X.shape[0], len(idx), c.shape[0]))
    for b in range(c.shape[2]):
        Y = Y + g[:, :, b].T[None, :, :] * X[:, b][:, None, None]
    return Y


def search(cores, K, which="abs", fixed=None):
    """dict(ind (nfound, d) int32 1-based, val, bound, nfound, certified, gap: per mode (1-based key) the gap at the cut divided by
    twice the allowance there (inf where everything was kept), tol_bound: the allowance of bound, nan: a score was NaN)"""
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    d = len(cores)
    I = _index_sets(cores, fixed)
    P = grams(cores, I)
    acores = [np.abs(c) for c in cores]
    PB = grams(acores, I)
    g = 1.01 * count(cores) * U
    X, XB = np.ones((1, 1)), np.ones((1, 1))
    recs, gaps = [None] * d, {}
    bound, tol_bound, any_nan = 0.0, 0.0, False
    with np.errstate(all="ignore"):
        for k in range(d - 1, -1, -1):
            nI = len(I[k])
            Y, YB = _sheet(cores[k], I[k], X), _sheet(acores[k], I[k], XB)
            if k == 0:
                s = np.abs(Y[:, :, 0]).ravel()
            else:
                s2 = (Y * (Y @ P[k].T)).sum(axis=2).ravel()
                s = np.where(np.isnan(s2), np.nan, np.sqrt(np.maximum(s2, 0.0)))
            E = 2.0 * g * (YB * (YB @ PB[k].T)).sum(axis=2).ravel()
            tol = np.minimum(np.sqrt(E), np.where(s > 0, E / np.where(s > 0, s, 1.0), np.inf)) + 2.0 * U * (s + np.sqrt(E))
            any_nan = any_nan or bool(np.isnan(s).any())
            rank = np.where(np.isnan(s), -1.0, s)
            order = np.argsort(-rank, kind="stable")                            # ties to the smaller flat position
            kept, drop = np.sort(order[:K]), order[K:]
            if drop.size:
                bound = max(bound, float(rank[drop[0]]))
                tol_bound = max(tol_bound, float(np.nanmax(tol[drop])))
                lo, hi = order[K - 1], order[K]
                gaps[k + 1] = float((rank[lo] - rank[hi]) / (2.0 * max(tol[lo], tol[hi])))
            else:
                gaps[k + 1] = np.inf
            recs[k] = kept
            cand, ii = kept // nI, kept % nI
            X, XB = Y[cand, ii, :], YB[cand, ii, :]
    nf = X.shape[0]
    ind = np.zeros((nf, d), dtype=np.int32)
    slot = np.arange(nf)
    for k in range(d):
        p = recs[k][slot]
        ind[:, k] = I[k][p % len(I[k])] + 1
        slot = p // len(I[k])
    val = X[:, 0].copy()
    o = order_rows(ind, val, which)
    ind, val = ind[o], val[o]
    b = np.nan if any_nan else bound
    return dict(ind=ind, val=val, bound=b, nfound=nf, certified=certified(val, b), gap=gaps, tol_bound=tol_bound, nan=any_nan)


def order_rows(ind, val, which):
    """the permutation that orders the rows by `which`, NaN last, ties by the lexicographically smaller row"""
    key = {"abs": -np.abs(val), "max": -val, "min": val}[which]
    rows = [(np.isnan(key[j]), 0.0 if np.isnan(key[j]) else key[j] + 0.0, tuple(ind[j])) for j in range(len(val))]
    return np.array(sorted(range(len(val)), key=lambda j: rows[j]), dtype=np.int64)


def certified(val, bound):
    av = np.abs(val)
    if av.size > 1 and bound <= av.min():                                       # a single row: the two coincide, "max" is reported
        return "all"
    if av.size and bound <= av.max():
        return "max"
    return None


def dense_topk(T, K, which="abs", fixed=None):
    """(ind 1-based, val) of the K first elements of the dense tensor (at the fixed indices) in the order of `which`"""
    d = T.ndim
    fixed = [0] * d if fixed is None else [int(f) for f in fixed]
    sl = tuple(slice(None) if not f else slice(f - 1, f) for f in fixed)
    sub = T[sl]
    idx = np.stack(np.unravel_index(np.arange(sub.size), sub.shape), axis=1)
    idx = idx + np.array([f - 1 if f else 0 for f in fixed])[None, :] + 1
    val = sub.ravel()
    o = order_rows(idx, val, which)[:K]
    return idx[o].astype(np.int32), val[o]


# ---- the cases of tests/test_gpu_topk.py, shared with the CPU test that checks their conditions on the reference alone ------------
SHAPES = {
    "tiny": ((3, 2, 4), (1, 2, 3, 1)),
    "d4": ((6, 7, 5, 8), (1, 4, 5, 3, 1)),
    "d4_pos": ((6, 7, 5, 8), (1, 4, 5, 3, 1)),
    "d6": ((5,) * 6, (1, 3, 4, 4, 4, 3, 1)),
    "d3_wide": ((70, 9, 66), (1, 9, 70, 1)),
    "d3_r128": ((20, 130, 20), (1, 128, 128, 1)),
    "rank1": ((9,) * 5, (1,) * 6),
    "peaked": ((9,) * 5, (1, 3, 3, 3, 3, 1)),
    "d3_r17_33": ((4, 3, 4), (1, 17, 33, 1)),                   # left ranks in 17..32 and 33..64: the score kernel's tiers 2 and 4
    "d3_r112_113": ((3, 3, 3), (1, 112, 113, 1)),               # either side of the score kernel's 64 KB of LDS
}
SEEDS = {name: 100 + j for j, name in enumerate(SHAPES)}
KS = (1, 4, 5, 16, 17, 64, 100, 256)
# the (case, K) pairs of the GPU tests: every case at every K
GPU_KS = {name: KS for name in SHAPES}
_cache = {}


def case(name):
    """the cores of a case: seeded and mode-dependent, so that no two modes share a factor"""
    if name in _cache:
        return _cache[name]
    n, r = SHAPES[name]
    d = len(n)
    rng = np.random.default_rng(SEEDS[name])
    if name == "peaked":
        cores = []
        for k in range(d):
            x = np.arange(n[k])
            c1, c2 = 1.3 + 0.9 * k, 6.6 - 0.7 * k
            w1, w2 = 0.4 + 0.03 * k, 0.45 - 0.02 * k
            f = [np.exp(-0.5 * ((x - c1) / w1) ** 2), 0.6 * np.exp(-0.5 * ((x - c2) / w2) ** 2)]
            g = 0.05 * rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1]))
            for a in range(r[k]):
                for b in range(r[k + 1]):
                    if a == b or r[k] == 1 or r[k + 1] == 1:
                        j = (a if r[k] > 1 else b) % 3
                        if j < 2:
                            g[a, :, b] += f[j]
            cores.append(g)
    elif name == "d4_pos":
        cores = [rng.uniform(0.1, 1.0, (r[k], n[k], r[k + 1])) for k in range(d)]
    else:
        cores = [rng.standard_normal((r[k], n[k], r[k + 1])) for k in range(d)]
    _cache[name] = cores
    return cores


def cases():
    return list(SHAPES)


_dense, _search = {}, {}


def dense_of(name):
    if name not in _dense:
        _dense[name] = dense(case(name))
        _dense[name].setflags(write=False)
    return _dense[name]


def search_of(name, K, which="abs"):
    """the reference's search of a case, computed once"""
    key = (name, K, which)
    if key not in _search:
        _search[key] = search(case(name), K, which)
    return _search[key]
