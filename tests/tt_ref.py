"""Independent reference for the tt_lib utilities (dtt_ort / dtt_svd / dtt_norm / dtt_lognrm), test side only.

Nothing here comes from oracle/: the contractions are numpy float64 that carry a running binary exponent (so no train
whose norm is representable anywhere in [2^-2^62, 2^2^62] over- or underflows), and the rounding of lib/tt.f90 (ort, then
right-to-left svd with the chop of lib/mat.f90, rank floored at 1) is restated in two precisions:
  * "mp":  mpmath at 50 digits for small trains (r <= 16); the factorisations come from the Gram matrix of each unfolding
           (eigsy), which at 50 digits still resolves singular values down to ~1e-20 of the largest;
  * "f64": numpy / LAPACK (np.linalg.qr / svd, which scale internally), each unfolding prescaled by a power of two.
Every chop decision reports its margin |tail - tol^2 |s|^2| / (tol^2 |s|^2); a test asserts a rank only where the margin
is wide enough for the device's rounding not to flip it.  The builders use powers of two for every scale, so a gauged
or scaled train is exactly the same tensor (times 2^e)."""
import math

import numpy as np

try:
    from mpmath import mp
except ImportError:      # mpmath ships with torch; without it only the f64 reference is available
    mp = None

MP_DPS = 50


# ---- scaled float64 contractions ----------------------------------------------------------------------------------
def _renorm(x, e):
    """x * 2^e -> (x', e') with max |x'| in [0.5, 1) (x unchanged if zero or not finite)"""
    m = np.max(np.abs(x)) if np.size(x) else 0.0
    if m == 0.0 or not np.isfinite(m):
        return x, e
    k = math.frexp(m)[1]
    return np.ldexp(x, -k), e + k


def _cores_scaled(cores):
    out, e = [], 0
    for c in cores:
        c2, k = _renorm(np.asarray(c, dtype=np.float64), 0)
        out.append(c2)
        e += k
    return out, e


def norm_log2(cores):
    """log2 of the Frobenius norm (-inf for a zero train)"""
    cs, e = _cores_scaled(cores)
    g = np.ones((1, 1))
    for c in cs:
        g = np.einsum("ab,ajc,bjd->cd", g, c, c)
        g, e2 = _renorm(g, 0)
        e += e2 / 2.0                      # g is the Gram matrix: its exponent counts twice
    s = float(g[0, 0])
    return -math.inf if s == 0.0 else 0.5 * math.log2(s) + e


def log10_norm(cores):
    return norm_log2(cores) * math.log10(2.0)


def norm(cores):
    """the norm as a double (0 / inf outside the double range, as dtt_norm)"""
    l2 = norm_log2(cores)
    if l2 == -math.inf:
        return 0.0
    if l2 > 1024:
        return math.inf
    return math.ldexp(2.0 ** (l2 - math.floor(l2)), int(math.floor(l2)))


def _chain(cores, mats):
    """v = prod_k mats[k](core_k) with a running exponent; returns (mantissa, exponent)"""
    cs, e = _cores_scaled(cores)
    v = np.ones((1, 1))
    for c, f in zip(cs, mats):
        v = v @ f(c)
        v, e2 = _renorm(v, 0)
        e += e2
    return float(v[0, 0]), e


def quad(cores, w):
    """sum_i A(i) prod_k w_k(i_k) (dtt_quad with rank-1 weights)"""
    m, e = _chain(cores, [lambda c, q=q: np.einsum("ijk,j->ik", c, np.asarray(q, dtype=np.float64)) for q in w])
    return math.ldexp(m, e)


def element(cores, ind):
    """A(ind), ind 1-based (dtt_ijk)"""
    m, e = _chain(cores, [lambda c, j=j: c[:, j - 1, :] for j in ind])
    return math.ldexp(m, e)


def scaled_dense(cores):
    """dense tensor of a small train as (T, e): A = T * 2^e"""
    cs, e = _cores_scaled(cores)
    t = cs[0]
    for c in cs[1:]:
        t = np.tensordot(t, c, axes=([t.ndim - 1], [0]))
        t, e2 = _renorm(t, 0)
        e += e2
    return t.reshape(t.shape[1:-1]), e


# ---- chop (lib/mat.f90:433-458), the rank floored at 1 ------------------------------------------------------------
def chop(s2, tol, rmax):
    """s2: squared singular values, descending.  Returns (rank, squared tail, margin of the closest decision)."""
    n = len(s2)
    r, er2 = n, 0 * s2[0]
    if 0 < rmax < r:
        er2 = sum(s2[rmax:], 0 * s2[0])
        r = rmax
    margin = math.inf
    if tol is not None:
        bound = tol * tol * sum(s2, 0 * s2[0])
        er = er2 + s2[r - 1]
        while r > 1:
            if bound > 0:
                margin = min(margin, float(abs(er - bound) / bound))
            if not er < bound:
                break
            er2 = er
            r -= 1
            er = er + s2[r - 1]
    return r, er2, margin


# ---- factorisations ------------------------------------------------------------------------------------------------
def _to_mp(a):
    return np.vectorize(lambda x: mp.mpf(float(x)), otypes=[object])(a)


def _mp_eig_desc(g):
    """eigen-decomposition of a symmetric object matrix, descending; negative rounding noise clipped to 0"""
    E, Q = mp.eigsy(mp.matrix(g.tolist()))
    n = g.shape[0]
    lam = [E[i] for i in range(n)]
    order = sorted(range(n), key=lambda i: -lam[i])
    lam = [max(lam[i], mp.mpf(0)) for i in order]
    q = np.empty((n, n), dtype=object)
    for c, i in enumerate(order):
        for rr in range(n):
            q[rr, c] = Q[rr, i]
    return lam, q


def _left_factor(a, prec):
    """a (m x n) = Q B, Q with orthonormal columns (min(m, n) of them) -- the left-orthogonalisation step of dtt_ort"""
    m, n = a.shape
    k = min(m, n)
    if prec == "f64":
        q, b = np.linalg.qr(a)
        return q[:, :k], b[:k, :]
    lam, v = _mp_eig_desc(a.T @ a)                        # a = (a v s^-1) (s v^T)
    lam = lam[:k]
    cut = lam[0] * mp.mpf(10) ** (-2 * MP_DPS + 10) if lam and lam[0] > 0 else mp.mpf(0)
    q = a @ v[:, :k]
    for c in range(k):
        s = mp.sqrt(lam[c])
        for rr in range(m):
            q[rr, c] = q[rr, c] / s if lam[c] > cut else mp.mpf(0)
    b = np.empty((k, n), dtype=object)
    for c in range(k):
        s = mp.sqrt(lam[c])
        for j in range(n):
            b[c, j] = s * v[j, c]
    return q, b


def _svd(a, prec):
    """a (m x n) = U diag(s) Vt with min(m, n) singular values, descending; returns (U, s^2 list, s list, Vt)"""
    m, n = a.shape
    k = min(m, n)
    if prec == "f64":
        u, s, vt = np.linalg.svd(a, full_matrices=False)
        return u, [float(x) ** 2 for x in s], [float(x) for x in s], vt
    lam, u = _mp_eig_desc(a @ a.T)
    lam = lam[:k]
    u = u[:, :k]
    s = [mp.sqrt(x) for x in lam]
    cut = lam[0] * mp.mpf(10) ** (-2 * MP_DPS + 10) if lam and lam[0] > 0 else mp.mpf(0)
    ut_a = u.T @ a
    vt = np.empty((k, n), dtype=object)
    for c in range(k):
        for j in range(n):
            vt[c, j] = ut_a[c, j] / s[c] if lam[c] > cut else mp.mpf(0)
    return u, lam, s, vt


def _prescale(a, prec):
    """a -> (a 2^-e, e), max |a 2^-e| in [0.5, 1)"""
    if prec == "mp":
        m = max((abs(x) for x in a.flat), default=mp.mpf(0))
        if m == 0:
            return a, 0
        e = int(mp.floor(mp.log(m, 2))) + 1
        return a * mp.ldexp(mp.mpf(1), -e), e
    return _renorm(a, 0)


# ---- dtt_svd (lib/tt.f90:307-368) -----------------------------------------------------------------------------------
def tt_svd_ref(cores, tol, rmax=0, prec="mp"):
    """ort + right-to-left truncated svd.  tol None: no tolerance (rmax only).  Returns a dict:
    ranks (r0..rd), spectra (per bond k = 1..d-1: singular values divided by their 2-norm, as floats), err (relative
    Frobenius error of the rounded train, = sqrt(sum of the chopped tails) / |A|), margin (per bond), log2norm (of A)."""
    if prec == "mp" and mp is None:
        raise RuntimeError("mpmath is not available")
    d = len(cores)
    r = [cores[0].shape[0]] + [c.shape[2] for c in cores]
    n = [c.shape[1] for c in cores]
    if prec == "mp":
        mp.dps = MP_DPS
        cs = [_to_mp(c) for c in cores]
    else:
        cs = [np.asarray(c, dtype=np.float64).copy() for c in cores]
    ex = 0                                                          # the train is cs * 2^ex
    for k in range(d):
        cs[k], e = _prescale(cs[k], prec)
        ex += e

    def unf(k, rows):
        return cs[k].reshape((rows, -1), order="F")

    # ort, left to right
    for k in range(d - 1):
        a = unf(k, r[k] * n[k])
        q, b = _left_factor(a, prec)
        mn = q.shape[1]
        cs[k] = q.reshape((r[k], n[k], mn), order="F")
        nxt = b @ unf(k + 1, r[k + 1])
        r[k + 1] = mn
        cs[k + 1], e = _prescale(nxt.reshape((mn, n[k + 1], r[k + 2]), order="F"), prec)
        ex += e
    spectra, margins, tails = [None] * (d - 1), [math.inf] * (d - 1), []
    total = None
    for k in range(d - 1, 0, -1):
        a = unf(k, r[k])
        u, s2, s, vt = _svd(a, prec)
        if total is None:
            total = (sum(s2, 0 * s2[0]), ex)                       # |A|^2 = total[0] * 4^ex
        rr, tail, mg = chop(s2, tol, rmax)
        nrm = math.sqrt(float(sum(s2, 0 * s2[0]))) if float(sum(s2, 0 * s2[0])) > 0 else 1.0
        spectra[k - 1] = [float(x) / nrm for x in s]
        margins[k - 1] = mg
        tails.append((tail, ex))
        cs[k] = vt[:rr].reshape((rr, n[k], r[k + 1]), order="F")
        us = u[:, :rr] * np.array(s[:rr], dtype=object if prec == "mp" else np.float64)[None, :]
        prv = unf(k - 1, r[k - 1] * n[k - 1]) @ us
        r[k] = rr
        cs[k - 1], e = _prescale(prv.reshape((r[k - 1], n[k - 1], rr), order="F"), prec)
        ex += e
    if total is None or float(total[0]) == 0.0:
        err = 0.0
    else:
        err2 = sum(float(t / total[0]) * 4.0 ** (e - total[1]) for t, e in tails)
        err = math.sqrt(err2)
    return dict(ranks=r, spectra=spectra, err=err, margin=margins, log2norm=norm_log2(cores))


def ort_ranks(cores):
    """the ranks dtt_ort leaves: r_k = min(r_(k-1) n_k, r_k) left to right"""
    r = [cores[0].shape[0]] + [c.shape[2] for c in cores]
    for k in range(len(cores) - 1):
        r[k + 1] = min(r[k] * cores[k].shape[1], r[k + 1])
    return r


# ---- train builders (every scale a power of two) -------------------------------------------------------------------
def rand_train(seed, n, r):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((r[k], n[k], r[k + 1])) for k in range(len(n))]


def gauge(cores, bond, e):
    """core bond-1 times 2^e, core bond times 2^-e (bond = 1..d-1): the same tensor"""
    out = [c.copy() for c in cores]
    out[bond - 1] = np.ldexp(out[bond - 1], e)
    out[bond] = np.ldexp(out[bond], -e)
    return out


def scale(cores, e):
    """the tensor times 2^e, spread evenly over the cores"""
    d = len(cores)
    es = [e // d] * d
    es[0] += e - sum(es)
    return [np.ldexp(c, k) for c, k in zip(cores, es)]


def rank_deficient(seed, n, rdecl=12, rtrue=3):
    """declared bond ranks rdecl, true ranks rtrue: every bond index repeated rdecl/rtrue times, the copies of a
    right-hand index divided by that count (a power of two) -- exactly the rank-rtrue train"""
    rep = rdecl // rtrue
    assert rep * rtrue == rdecl and rep & (rep - 1) == 0
    d = len(n)
    base = rand_train(seed, n, [1] + [rtrue] * (d - 1) + [1])
    out = []
    for k, c in enumerate(base):
        ri = np.arange(1 if k == 0 else rdecl) % c.shape[0]
        ro = np.arange(1 if k == d - 1 else rdecl) % c.shape[2]
        x = c[ri][:, :, ro]
        if k > 0:
            x = x / rep
        out.append(x)
    return out


def _orth(rng, m, k):
    q, _ = np.linalg.qr(rng.standard_normal((m, k)))
    return q[:, :k]


def flat(seed, n, r):
    """every unfolding has r equal singular values: cores whose mode slices are orthogonal / sqrt(n) (left and right
    orthonormal at once), the first with orthonormal columns, the last with orthonormal rows (needs n >= r at the ends)"""
    rng = np.random.default_rng(seed)
    d = len(n)
    out = [_orth(rng, n[0], r).reshape((1, n[0], r))]
    for k in range(1, d - 1):
        out.append(np.stack([_orth(rng, r, r) for _ in range(n[k])], axis=1) / math.sqrt(n[k]))
    out.append(_orth(rng, n[-1], r).T.reshape((r, n[-1], 1)))
    return out


def graded(seed, n, r, bond=1, step=2):
    """a flat train with diag(10^-step*i), i = 0..r-1, at `bond`: that bond's spectrum is graded"""
    out = flat(seed, n, r)
    s = 10.0 ** (-step * np.arange(r))
    out[bond] = out[bond] * s[:, None, None]
    return out


def zero_train(n, r):
    return [np.zeros((r[k], n[k], r[k + 1])) for k in range(len(n))]


def one_zero_core(seed, n, r, k):
    out = rand_train(seed, n, r)
    out[k] = np.zeros_like(out[k])
    return out


# ---- comparisons ---------------------------------------------------------------------------------------------------
def probe_indices(n, count=64, seed=0):
    rng = np.random.default_rng(seed)
    return [[int(rng.integers(1, nk + 1)) for nk in n] for _ in range(count)]


def rel_dist(cores, ref, shift=0):
    """|A(cores) 2^-shift - A(ref)| / |A(ref)|: dense for d <= 6, otherwise over 64 probe elements (relative to their norm)"""
    n = [c.shape[1] for c in ref]
    if len(ref) <= 6:
        t1, e1 = scaled_dense(cores)
        t0, e0 = scaled_dense(ref)
        den = np.linalg.norm(t0)
        return np.linalg.norm(np.ldexp(t1, e1 - shift - e0) - t0) / den if den > 0 else np.linalg.norm(t1)
    a = np.array([element(cores, i) for i in probe_indices(n)])
    b = np.array([element(ref, i) for i in probe_indices(n)])
    return np.linalg.norm(np.ldexp(a, -shift) - b) / np.linalg.norm(b)


def orthonormality(cores):
    """max |U^T U - I| over the left unfoldings of cores 1..d-1, each divided by its own norm / sqrt(columns)
    (dtt_ort leaves orthonormal unfoldings times the equalised scale |A|^(1/d))"""
    worst = 0.0
    for c in cores[:-1]:
        u = c.reshape(-1, c.shape[2], order="F")
        u, _ = _renorm(u, 0)
        u = u / (np.linalg.norm(u) / math.sqrt(u.shape[1]))
        worst = max(worst, float(np.abs(u.T @ u - np.eye(u.shape[1])).max()))
    return worst
