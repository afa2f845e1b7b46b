"""Integer trains on which ttx_topk and ttx_sample have ONE answer (test side, numpy only).

The cores hold small integers, so every product and sum of either call is an exact double far below 2^53 and no summation order
-- plain loops, the matrix cores, numpy, the marginals kernels -- can change a bit: the definitions of include/ttx.h apply with no
allowance, and tests/topk_ref.py's search and tests/sample_ref.py's draw are the expectation as they stand.  Exact ties come from
periodic modes, G_k(:, i, :) = B_k(:, i mod q, :) (times (-1)^(i div q) for top-K: a sign flips y, not the score), so that the cut of
every selection falls inside a group of bit-identical scores, and a uniform u = j q / n_k lands exactly on an edge of the CDF.

tie_train / edge_train / edge_u build the inputs; cut_trace walks a top-K search by the definition's own words (the keys above T,
then the first `need` keys equal to T) and reports where the cut fell; exact_check redoes the arithmetic the decisions rest on in
exact Python numbers (object dtype) and asserts that the float64 values are those numbers, below 2^40.
The cases of tests/test_gpu_exact_decisions.py are listed at the end; tests/test_exact_decisions_cpu.py asserts on the references
alone that they reach what they are meant to reach."""
import functools
from fractions import Fraction

import numpy as np

import sample_ref as S
import topk_ref as R

LIMIT = 2 ** 40
CHUNK = 4096                                                                    # TTX_TK_CHUNK: positions per workgroup of the compaction kernels


# ---- generators ------------------------------------------------------------------------------------------------------------------
def _periodic(base, n, q, flip):
    i = np.arange(n)
    g = base[:, i % q, :]
    if flip:
        g = g * np.where((i // q) % 2 == 0, 1, -1)[None, :, None]
    return g.astype(np.float64)


def tie_train(seed, n, r, q, lo, hi):
    """cores G_k(:, i, :) = (-1)^(i div q) B_k(:, i mod q, :), the base slices integer-valued, uniform in lo..hi, none all zero"""
    rng = np.random.default_rng(seed)
    cores = []
    for k, nk in enumerate(n):
        assert nk % q == 0
        base = rng.integers(lo, hi + 1, (r[k], q, r[k + 1]))
        for s in range(q):
            while not base[:, s, :].any():
                base[:, s, :] = rng.integers(lo, hi + 1, (r[k], r[k + 1]))
        cores.append(_periodic(base, nk, q, True))
    return cores


def edge_train(seed, n, r, q, zero_slots):
    """non-negative cores G_k(:, i, :) = B_k(:, i mod q, :) with integers in 0..2 and no sign flips (they would cancel the mode sums
    M_k); the base slices of zero_slots are all zero, the others have a positive first row and first column, so that p > 0 there"""
    rng = np.random.default_rng(seed)
    cores = []
    for k, nk in enumerate(n):
        assert nk % q == 0
        base = rng.integers(0, 3, (r[k], q, r[k + 1]))
        base[0, :, :] = rng.integers(1, 3, (q, r[k + 1]))
        base[:, :, 0] = rng.integers(1, 3, (r[k], q))
        base[:, list(zero_slots), :] = 0
        cores.append(_periodic(base, nk, q, False))
    return cores


def edge_u(seed, n, q, npts):
    """u[:, k] = j / (n_k / q), j uniform in 0 .. n_k / q: with n_k / q a power of two u_k c_k(n_k) is exactly c_k(q j - 1)"""
    rng = np.random.default_rng(seed)
    u = np.empty((npts, len(n)))
    for k, nk in enumerate(n):
        reps = nk // q
        assert reps * q == nk and reps & (reps - 1) == 0
        u[:, k] = rng.integers(0, reps + 1, npts) / reps
    return u


def edge_closed_form(n, q, zero_slots, u):
    """the 1-based indices the definition gives on an edge_train: q j + (first non-zero slot) for u_k = j / reps < 1, the last index
    with a non-zero slot for u_k = 1"""
    live = [s for s in range(q) if s not in set(zero_slots)]
    ind = np.empty(u.shape, dtype=np.int32)
    for k, nk in enumerate(n):
        reps = nk // q
        j = np.rint(u[:, k] * reps).astype(np.int64)
        assert np.array_equal(j / reps, u[:, k])
        ind[:, k] = np.where(j < reps, q * j + live[0], nk - q + live[-1]) + 1
    return ind


# ---- exact numbers ---------------------------------------------------------------------------------------------------------------
def _obj(a):
    """the doubles of a as exact Python numbers: int where integral, else Fraction"""
    a = np.asarray(a, dtype=np.float64)
    assert np.all(np.isfinite(a))
    out = np.empty(a.size, dtype=object)
    for j, v in enumerate(a.ravel().tolist()):
        out[j] = int(v) if v == int(v) else Fraction(v)
    return out.reshape(a.shape)


def _same(f, x, what):
    """the float64 array f holds exactly the numbers of the object array x, all below 2^40 in magnitude"""
    f, x = np.asarray(f, dtype=np.float64), np.asarray(x, dtype=object)
    assert f.shape == x.shape, (what, f.shape, x.shape)
    big = max([abs(v) for v in x.ravel().tolist()], default=0)
    assert big < LIMIT, (what, big)
    assert np.all(_obj(f) == x), what


def _classes(rows):
    """(representatives, inverse) of the distinct rows of a 2-d float array"""
    rep, inv = np.unique(rows, axis=0, return_inverse=True)
    return rep, np.asarray(inv).ravel()


def _slices(c, idx):
    """the slices G(:, i, :) for i in idx as rows of length r0 r1"""
    return np.moveaxis(c[:, idx, :], 1, 0).reshape(len(idx), -1)


def _grams_exact(cores, I):
    """P_0 .. P_(d-1) in exact numbers, each distinct slice (up to its sign, which g^T P g does not see) taken once"""
    P = [np.array([[1]], dtype=object)]
    for c, idx in zip(cores[:-1], I):
        r0, _, r1 = c.shape
        rows = _slices(c, idx)
        lead = rows[np.arange(len(rows)), (rows != 0).argmax(axis=1)]
        rep, inv = _classes(rows * np.where(lead < 0, -1.0, 1.0)[:, None])
        cnt = np.bincount(inv, minlength=len(rep))
        acc = np.zeros((r1, r1), dtype=object)
        for row, m in zip(rep, cnt):
            g = _obj(row.reshape(r0, r1))
            acc = acc + int(m) * (g.T @ (P[-1] @ g))
        P.append(acc)
    return P


def cut_trace(cores, K, fixed=None, check=False):
    """The search of include/ttx.h told by thresholds: per mode T = the K-th largest score, the pairs above T and then the first
    need = K - #(above) pairs equal to T, in ascending flat position.  Returns (ind, modes): the kept index rows (1-based, in the
    candidate order of mode 1) and per mode with a real selection (1-based key) dict(M, T, need, equal = positions of the scores
    equal to T).  check: every y and every s^2 of the walk is compared with exact numbers (distinct states x distinct slices)."""
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    d = len(cores)
    I = R._index_sets(cores, fixed)
    P = R.grams(cores, I)
    if check:
        PX = _grams_exact(cores, I)
        for k in range(d):
            _same(P[k], PX[k], f"P_{k}")
    X = np.ones((1, 1))
    recs, modes = [None] * d, {}
    for k in range(d - 1, -1, -1):
        nI = len(I[k])
        Y = R._sheet(cores[k], I[k], X)
        s2 = Y[:, :, 0] ** 2 if k == 0 else (Y * (Y @ P[k].T)).sum(axis=2)
        if check:
            r0, _, r1 = cores[k].shape
            xr, xi = _classes(X)
            gr, gi = _classes(_slices(cores[k], I[k]))
            yx = np.empty((len(xr), len(gr), r0), dtype=object)
            sx = np.empty((len(xr), len(gr)), dtype=object)
            for a, xv in enumerate(xr):
                for b, gv in enumerate(gr):
                    y = _obj(gv.reshape(r0, r1)) @ _obj(xv)
                    yx[a, b] = y
                    sx[a, b] = y[0] * y[0] if k == 0 else y @ (PX[k] @ y)
            big = max(max(abs(v) for v in yx.ravel().tolist()), max(abs(v) for v in sx.ravel().tolist()))
            assert big < LIMIT, (k, big)
            assert np.array_equal(Y, yx.astype(np.float64)[xi][:, gi]), f"y of mode {k + 1}"
            assert np.array_equal(s2, sx.astype(np.float64)[xi][:, gi]), f"s^2 of mode {k + 1}"
        s = np.abs(Y[:, :, 0]).ravel() if k == 0 else np.sqrt(np.maximum(s2.ravel(), 0.0))
        M = s.size
        if M <= K:
            kept = np.arange(M)
        else:
            T = np.partition(s, M - K)[M - K]
            above, equal = np.flatnonzero(s > T), np.flatnonzero(s == T)
            need = K - above.size
            kept = np.sort(np.concatenate([above, equal[:need]]))
            modes[k + 1] = dict(M=M, T=float(T), need=int(need), equal=equal)
        recs[k] = kept
        X = Y[kept // nI, kept % nI, :]
    nf = X.shape[0]
    ind = np.zeros((nf, d), dtype=np.int32)
    slot = np.arange(nf)
    for k in range(d):
        p = recs[k][slot]
        ind[:, k] = I[k][p % len(I[k])] + 1
        slot = p // len(I[k])
    return ind, modes


def sample_walk(cores, u, w=None, check=False):
    """draw's walk once more with its intermediate numbers: (ind, modes), per mode (1-based key) dict(p, c, t) of every sample.
    check: the prefix vectors, the head tables and every p (distinct states) are compared with exact numbers."""
    cores, w, fixed = S._prep(cores, w, None)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    d, npts = len(cores), u.shape[0]
    H = S.heads(cores, w, fixed)
    if check:
        lv, lx = np.ones(1), np.array([1], dtype=object)
        for k, (c, q) in enumerate(zip(cores, w)):
            r0, n, r1 = c.shape
            hx = np.empty((n, r1), dtype=object)
            rep, inv = _classes(_slices(c, np.arange(n)))
            hrep = [lx @ _obj(row.reshape(r0, r1)) for row in rep]
            qx = _obj(q)
            for i in range(n):
                hx[i] = qx[i] * hrep[inv[i]]
            mx = np.zeros((r0, r1), dtype=object)                               # M_k, once per distinct (slice, weight)
            wrep, winv = _classes(np.column_stack([inv.astype(np.float64), q]))
            for (cls, wt), m in zip(wrep, np.bincount(winv, minlength=len(wrep))):
                mx = mx + int(m) * _obj(wt).item() * _obj(rep[int(cls)].reshape(r0, r1))
            _same(H[k], hx, f"H_{k + 1}")
            m = np.zeros((r0, r1))                                              # the floats of sample_ref.heads, in its order
            for i in range(n):
                m = m + q[i] * c[:, i, :]
            nl = np.zeros(r1)
            for a in range(r0):
                nl = nl + lv[a] * m[a]
            lv, lx = nl, lx @ mx
            _same(lv, lx, f"l_{k + 1}")
    ind = np.zeros((npts, d), dtype=np.int32)
    x = np.ones((npts, 1))
    modes = {}
    for k in range(d - 1, -1, -1):
        p = S._p_rows(H[k], x)
        c = np.cumsum(p, axis=1)
        t = u[:, k] * c[:, -1]
        if check:
            xr, xi = _classes(x)
            hx = _obj(H[k])
            px = np.empty((len(xr), hx.shape[0]), dtype=object)
            for a, xv in enumerate(xr):
                px[a] = np.abs(hx @ _obj(xv))
            _same(p[np.unique(xi, return_index=True)[1]], px, f"p_{k + 1}")
            assert np.array_equal(p, px.astype(np.float64)[xi])
            cx = np.cumsum(px, axis=1)
            _same(c[np.unique(xi, return_index=True)[1]], cx, f"c_{k + 1}")
        i0 = S._choose(p, c, t, u[:, k])
        assert np.all(i0 >= 0)
        modes[k + 1] = dict(p=p, c=c, t=t)
        ind[:, k] = i0 + 1
        x = S._step(cores[k], i0, x)
    return ind, modes


def exact_check(cores, K=None, fixed=None, u=None, w=None):
    """The quantities the decisions rest on, recomputed in exact Python numbers and compared with the float64 of the references:
    with K (one or several) every Gram matrix entry, every y and every s^2 of the top-K walk; with u every prefix vector, head
    table, p and running sum of the samples' walk.  Each must be the exact number, of magnitude below 2^40."""
    assert (K is None) != (u is None)
    if K is not None:
        for kk in np.atleast_1d(K):
            cut_trace(cores, int(kk), fixed, check=True)
    else:
        sample_walk(cores, u, w, check=True)
    return True


# ---- the cases of tests/test_gpu_exact_decisions.py --------------------------------------------------------------------------------
TOPK = {
    "ties_d4": dict(n=(12,) * 4, r=(1, 3, 3, 3, 1), q=4, lo=-2, hi=2, seed=1, K=(5, 17, 100)),
    "ties_chunks": dict(n=(64,) * 3, r=(1, 2, 2, 1), q=8, lo=-2, hi=2, seed=1, K=(256, 1000, 4096)),
    # seed 4037: the first of 1 .. 4037 at which the two largest of the 25 distinct scores of mode 2 are equal (each 64 times on the sheet),
    # so that K = 64 cuts inside a tie group there as well
    "ties_r65": dict(n=(40,) * 3, r=(1, 65, 65, 1), q=5, lo=-1, hi=1, seed=4037, K=(64, 300)),
    "full_sheet": dict(n=(4096, 4096), r=(1, 2, 1), q=16, lo=-2, hi=2, seed=1, K=(4096,)),
}
WHICH_CASES = (("ties_d4", 100), ("ties_chunks", 256))
FIXED_CASE = ("ties_d4", 17, (0, 3, 0, 0))
SAMPLE = {
    "edge_small": dict(n=(64, 128, 32), r=(1, 3, 2, 1), q=8, zero=(0, 3, 7), seed=1),
    "edge_long": dict(n=(16, 2048, 8), r=(1, 2, 3, 1), q=8, zero=(0, 7), seed=1),
    "edge_r65": dict(n=(16, 16, 16), r=(1, 65, 65, 1), q=4, zero=(0,), seed=1),
}
NPTS = 600
WEIGHTED = "edge_small"


@functools.lru_cache(maxsize=None)
def topk_case(name):
    c = TOPK[name]
    cores = tie_train(c["seed"], c["n"], c["r"], c["q"], c["lo"], c["hi"])
    for g in cores:
        g.setflags(write=False)
    return cores


@functools.lru_cache(maxsize=None)
def refusal_train():
    """n = (3, 4097), integers in -2..2: K = 4096 asks for a sheet of 2^24 + 4096 pairs, K = 4095 fits"""
    rng = np.random.default_rng(7)
    cores = [rng.integers(-2, 3, (1, 3, 2)).astype(np.float64), rng.integers(-2, 3, (2, 4097, 1)).astype(np.float64)]
    cores[0][0, :, 0] = (1.0, -2.0, 1.0)                                        # no slice is all zero
    for g in cores:
        g.setflags(write=False)
    return cores


@functools.lru_cache(maxsize=None)
def topk_search(name, K, which="abs", fixed=None):
    """the reference's search of a case, computed once and shared"""
    res = R.search(topk_case(name), K, which, None if fixed is None else list(fixed))
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def sample_case(name):
    """(cores, u) of a sampling case: u on the edges"""
    c = SAMPLE[name]
    cores = edge_train(c["seed"], c["n"], c["r"], c["q"], c["zero"])
    u = edge_u(c["seed"] + 1000, c["n"], c["q"], NPTS)
    for a in cores + [u]:
        a.setflags(write=False)
    return cores, u


def below(u):
    """every non-zero entry one ulp towards 0"""
    return np.where(u > 0.0, np.nextafter(u, -1.0), u)


@functools.lru_cache(maxsize=None)
def weights(name):
    """power-of-two weights with zeros, w in {0, 0.5, 1, 2}, not periodic"""
    rng = np.random.default_rng(SAMPLE[name]["seed"] + 2000)
    w = [rng.choice([0.0, 0.5, 1.0, 2.0], nk) for nk in SAMPLE[name]["n"]]
    for a in w:
        a.setflags(write=False)
    return tuple(w)
