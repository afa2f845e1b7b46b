"""Reference for ttx_sample_real (include/ttx.h), numpy float64 only (test side).

draw(cores, nodes, u, cond) restates the definition with plain sequential sums: effective weights (trapezoid weights of a drawn
mode, the hat row of a held one), prefix vectors, head tables with weights of 1.0, modes drawn from the last to the first:
p = |H_k x|, cell masses A(j) = (0.5 (p(j) + p(j+1))) h_j, C their sequential running sum, T = u C(n-2), the smallest cell with
A > 0 and T < C (else the largest with A > 0 and lambda = 1), the root of p(j) l + D l^2 / 2 = s' in the form without cancellation,
x = t_j + lambda h_j clamped into the cell, the hat row of the rounded x, the two-term chain step.

verify(cores, nodes, u, cond, x_dev, cell_dev) walks every sample along the DEVICE's x, so that a difference at one mode cannot
cascade into the modes after it.  There is no "undecided" allowance: the conditional CDF is continuous, so the check is made in
its domain.  For every drawn mode, with j = cell_dev - 1:
    x_dev lies in [t_j, t_(j+1)],   A_ref(j) > 0,   |CDF_ref(x_dev) - min(u_k, 1) C_ref(n-2)| <= tol_k,
    CDF_ref(x) = C_ref(j-1) + h_j (p(j) l + D l^2 / 2),  l = (x - t_j) / h_j  (on a node the two cells that contain x agree).

The bound tol_k = 6 N u Bc + 16 u pmax h_j + u pmax max|t_k|, with pmax = max(p(j), p(j+1)) and u = 2^-53.

  * N.  One term of the double sum C(j) is a product l-chain . G_k . x-chain . h and reaches the result through the roundings
    sample_ref.py counts for ttx_sample, N0 = 2 sum_(k=0..d) (r_k + 2) + max n_k + 4 (prefix chain, state chain, the running sum
    in any association order, four single operations), and through
      - two more per bond of the state chain, 2 d in all: the chain step is z = (0.0 + phi_i tau_i) + phi_(i+1) tau_(i+1), one
        multiply by a hat value and one addition on top of tau's own.  The hat values themselves are no rounding DIFFERENCE:
        device and reference form them from the same x_dev by the same IEEE operations (ttx_basis_host's rule), as they form the
        trapezoid weights and h_j from the same nodes;
      - three for the cell mass: p(j) + p(j+1), the difference h_j, the product (the factor 0.5 is exact).
    N = N0 + 2 d + 3.  As in sample_ref.py, |computed - true| <= N u B for every order of the sums, B being the same quantity on
    |cores|, the effective weights (they are >= 0) and |state|; Bc is B for the total C(n-2).
  * 6 N u Bc.  Device against reference is 2 N u Bc on each number compared.  Three enter: the target T; the running sum C(j-1)
    together with the p(j), p(j+1) of the part inside the cell (their coefficients l - l^2/2 and l^2/2 times h_j are at most the
    cell's own weights, so both are covered by the bound on C(j)); and, where the device's s = T - C(j-1) left [0, A(j)] and
    was clipped, the distance between two of the device's own partial sums that stand for the same true number (C(j-1) and the C of
    the last cell with A > 0 before it differ by zeros added in another association order).
  * 16 u pmax h_j: the inversion, a fixed number of operations.  s = T - C(j-1), s' = s / h_j, D, p(j)^2, 2 D s', their sum,
    the square root, den, 2 s' / den, h_j, lambda h_j on the device: eleven, square root and division taken as within 1 ulp = 2 u,
    not as correctly rounded: 13 u; the reference's own l = (x - t_j) / h_j and the three operations of its quadratic: at most 16 u.
    Each is a relative error of a quantity bounded by pmax (s', D, den, sqrt(disc)) or pmax^2 (the terms of disc), and none is
    magnified on the way to the mass: with rho = p(j) + D l the density at the root, d(mass) = rho dl, dl = l d(den) / den,
    rho d(sqrt(disc)) <= d(disc) / 1 and den >= max(p(j), rho), so an error eps pmax^2 of disc moves the mass per unit length by
    at most eps pmax, also where disc cancels to 0 at the right end of a cell that falls to p(j+1) = 0.
  * u pmax max|t_k|: the rounding of x = t_j + lambda h_j itself, at most u |x|, times the density, which is at most pmax.
No constant comes from a run of the device code.

logq.  Along the device's x the log term is log((phi_i p(i) + phi_(i+1) p(i+1)) / C(n-2)): numerator and denominator carry 2 (N + 3)
u each relative to their B (the two multiplies and the addition on top of N), and the allowance 8 u (1 + |log term|) of
test_gpu_sample.py covers the division, both logs and the addition into the running sum:
    |logq_dev - logq_ref| <= sum over drawn modes of (4 (N + 3) u Bratio_k + 8 u (1 + |log term|)),
Bratio_k = max(Bnum / num, Bc / C(n-2)), which is 1 for a train without sign changes.  There exp(logq) = val / Z with Z = the
quad of the train with the effective weights; val and Z carry N u each against their true values:
    |exp(logq) Z - val| <= val (logq bound + 4 N u)."""
import numpy as np

import sample_ref as S

U = S.U
CASES, NPTS, SIGNED = S.CASES, S.NPTS, S.SIGNED


def case(name, signed=False):
    """(cores, u, nodes) of a test case: the cores and uniforms of sample_ref.case, unchanged, and seeded non-equidistant nodes"""
    cores, u, _ = S.case(name, signed)
    rng = np.random.default_rng(sum(map(ord, name)) + 77)
    nodes = [np.cumsum(rng.uniform(0.2, 1.0, c.shape[1])) - rng.uniform(0.0, 3.0) for c in cores]
    return cores, u, nodes


def trapezoid(t):
    t = np.asarray(t, dtype=np.float64)
    if t.size == 1:
        return np.ones(1)
    om = np.empty(t.size)
    om[0], om[-1] = 0.5 * (t[1] - t[0]), 0.5 * (t[-1] - t[-2])
    om[1:-1] = 0.5 * (t[2:] - t[:-2])
    return om


def hat(t, x):
    """TTX_BASIS_LINEAR's rule at the coordinates x (no NaN): (i, phi_i, phi_(i+1)) with i in 0 .. max(n - 2, 0); a mode of one node: (0, 1, 0)"""
    t, x = np.asarray(t, dtype=np.float64), np.asarray(x, dtype=np.float64)
    n = t.size
    if n == 1:
        return np.zeros(x.shape, int), np.ones(x.shape), np.zeros(x.shape)
    i = np.clip(np.searchsorted(t, x, side="right") - 1, 0, n - 2)
    lam = (x - t[i]) / (t[i + 1] - t[i])
    lo, hi = x <= t[0], x >= t[-1]
    f1 = np.where(lo, 0.0, np.where(hi, 1.0, lam))
    f0 = np.where(lo, 1.0, np.where(hi, 0.0, 1.0 - lam))
    return i, f0, f1


def hat_row(t, x):
    """the dense row phi(0 .. n-1) at one coordinate"""
    i, f0, f1 = hat(t, np.array([x]))
    row = np.zeros(np.size(t))
    row[i[0]] = f0[0]
    if np.size(t) > 1:
        row[i[0] + 1] = f1[0]
    return row


def _prep(cores, nodes, cond):
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    d = len(cores)
    nodes = [np.asarray(t, dtype=np.float64) for t in nodes]
    cond = np.full(d, np.nan) if cond is None else np.asarray(cond, dtype=np.float64)
    held = [bool(np.isfinite(cond[k]) or nodes[k].size == 1) for k in range(d)]
    xh = [float(cond[k]) if np.isfinite(cond[k]) else float(nodes[k][0]) for k in range(d)]
    eff = [hat_row(nodes[k], xh[k]) if held[k] else trapezoid(nodes[k]) for k in range(d)]
    return cores, nodes, held, xh, eff


def heads(cores, eff, held):
    """H_k(i, b) = sum_a l_(k-1)(a) G_k(a, i, b) as (n_k, r_k) arrays (None for a held mode), every sum sequential from 0.0"""
    lv, out = np.ones(1), []
    for c, e, f in zip(cores, eff, held):
        r0, n, r1 = c.shape
        if f:
            out.append(None)
        else:
            s = np.zeros((n, r1))
            for a in range(r0):
                s = s + lv[a] * c[a]
            out.append(s)
        m = np.zeros((r0, r1))
        for i in range(n):
            m = m + e[i] * c[:, i, :]
        nl = np.zeros(r1)
        for a in range(r0):
            nl = nl + lv[a] * m[a]
        lv = nl
    return out


def quad(cores, eff):
    """Z: the full sum of the train with the effective weights"""
    lv = np.ones(1)
    for c, e in zip(cores, eff):
        lv = lv @ np.tensordot(e, c, axes=([0], [1]))
    return float(lv[0])


def _masses(p, t):
    h = np.diff(t)
    return (0.5 * (p[:, :-1] + p[:, 1:])) * h[None, :]


def invert(p0, p1, sp):
    """lambda of the definition, elementwise: after the exact scaling that takes max(p0, p1) into [0.5, 1)"""
    m = np.maximum(p0, p1)
    e = np.frexp(np.where(np.isfinite(m) & (m > 0.0), m, 1.0))[1]
    p0, p1, sp = np.ldexp(p0, -e), np.ldexp(p1, -e), np.ldexp(sp, -e)
    D = p1 - p0
    disc = np.maximum(p0 * p0 + (2.0 * D) * sp, 0.0)
    den = p0 + np.sqrt(disc)
    with np.errstate(all="ignore"):
        lam = np.where(den > 0.0, (2.0 * sp) / np.where(den > 0.0, den, 1.0), 0.0)
    return np.clip(lam, 0.0, 1.0)


def _chain(c, i, f0, f1, x):
    """z = (0.0 + phi_i tau_i) + phi_(i+1) tau_(i+1); a mode of one node has the first term only"""
    z = 0.0 + f0[:, None] * S._step(c, i, x)
    if c.shape[1] > 1:
        z = z + f1[:, None] * S._step(c, i + 1, x)
    return z


def draw(cores, nodes, u, cond=None):
    """(x [npts][d], cell [npts][d] int32, logq, val, failed mask) by the definition"""
    cores, nodes, held, xh, eff = _prep(cores, nodes, cond)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    npts, d = u.shape
    H = heads(cores, eff, held)
    xs, cell, logq = np.zeros((npts, d)), np.zeros((npts, d), dtype=np.int32), np.zeros(npts)
    drawn = ~np.array(held)
    with np.errstate(invalid="ignore"):
        failed = ~np.all((u >= 0.0) | ~drawn[None, :], axis=1)
    st = np.ones((npts, 1))
    rows = np.arange(npts)
    with np.errstate(all="ignore"):
        for k in range(d - 1, -1, -1):
            t = nodes[k]
            if held[k]:
                xk = np.full(npts, xh[k])
            else:
                p = S._p_rows(H[k], st)
                A = _masses(p, t)
                C = np.cumsum(A, axis=1)
                tot = C[:, -1]
                T = u[:, k] * tot
                j = S._choose(A, C, T, u[:, k])
                failed |= ~(tot > 0.0) | np.isinf(tot) | (j < 0)
                j = np.where(failed, 0, j)
                hit = (A > 0) & (T[:, None] < C) & (u[:, k:k + 1] < 1.0)
                inside = hit[rows, j]                                   # else: the largest cell with A > 0, lambda = 1
                h = t[j + 1] - t[j]
                cprev = np.where(j > 0, C[rows, np.maximum(j - 1, 0)], 0.0)
                s = np.minimum(np.maximum(T - cprev, 0.0), A[rows, j])
                lam = np.where(inside, invert(p[rows, j], p[rows, j + 1], s / h), 1.0)
                xk = np.minimum(np.maximum(t[j] + lam * h, t[j]), t[j + 1])
                xk = np.where(failed, t[0], xk)
                cell[:, k] = j + 1
            i, f0, f1 = hat(t, xk)
            if not held[k]:
                logq = logq + np.log((f0 * p[rows, i] + f1 * p[rows, i + 1]) / tot)
            xs[:, k] = xk
            st = _chain(cores[k], i, f0, f1, st)
    xs[failed] = np.nan
    cell[failed] = 0
    return xs, cell, np.where(failed, np.nan, logq), np.where(failed, 0.0, st[:, 0]), failed


def count(cores):
    """N of the bound (module docstring)"""
    return S.count(cores) + 2 * len(cores) + 3


def verify(cores, nodes, u, cond, x_dev, cell_dev):
    """Walk the samples along x_dev (module docstring).  Raises AssertionError on a sample the definition does not allow; returns
    dict(logq, val = the reference's along the device's x, logq_bound = the bound on |logq_dev - logq|, N, worst = the largest
    |CDF_ref(x_dev) - T| / tol met, Z = the quad with the effective weights; and per sample and mode, zero for a held mode: tol,
    total = C_ref(n-2), pend = (p(n-2), p(n-1)), the reference's conditional at the two nodes of the last cell)."""
    cores, nodes, held, xh, eff = _prep(cores, nodes, cond)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    x_dev, cell_dev = np.asarray(x_dev, dtype=np.float64), np.asarray(cell_dev)
    npts, d = u.shape
    N = count(cores)
    H = heads(cores, eff, held)
    HB = heads([np.abs(c) for c in cores], eff, held)
    ref_failed = draw(cores, nodes, u, cond)[4]
    dev_failed = np.isnan(x_dev[:, 0])
    assert np.array_equal(dev_failed, ref_failed), ("failed samples differ", np.flatnonzero(dev_failed != ref_failed)[:10])
    assert np.all(np.isnan(x_dev[dev_failed])) and np.all(cell_dev[dev_failed] == 0)
    ok = ~dev_failed
    assert np.all(np.isfinite(x_dev[ok]))
    xw = np.where(ok[:, None], x_dev, np.array([t[0] for t in nodes])[None, :])
    st, stb = np.ones((npts, 1)), np.ones((npts, 1))
    logq, lqb = np.zeros(npts), np.zeros(npts)
    tols, totals, pend = np.zeros((npts, d)), np.zeros((npts, d)), np.zeros((npts, d, 2))
    rows = np.arange(npts)
    worst = 0.0
    for k in range(d - 1, -1, -1):
        t = nodes[k]
        xk = xw[:, k]
        i, f0, f1 = hat(t, xk)
        if held[k]:
            assert np.all(x_dev[ok, k] == xh[k]), f"mode {k + 1} is held at {xh[k]}"
            assert np.all(cell_dev[:, k] == 0), f"mode {k + 1} is held: cell 0"
        else:
            with np.errstate(all="ignore"):
                p = S._p_rows(H[k], st)
                A = _masses(p, t)
                C = np.cumsum(A, axis=1)
                tot = C[:, -1]
                Bc = np.cumsum(_masses(S._p_rows(HB[k], stb), t), axis=1)[:, -1]
            j = np.where(ok, cell_dev[:, k] - 1, 0)
            assert np.all((j >= 0) & (j <= t.size - 2)), f"mode {k + 1}: a cell outside 1 .. n - 1"
            assert np.all((t[j] <= xk) & (xk <= t[j + 1]) | ~ok), f"mode {k + 1}: x outside its cell"
            assert np.all((A[rows, j] > 0) | ~ok), f"mode {k + 1}: a cell without mass was drawn"
            h = t[j + 1] - t[j]
            p0, p1 = p[rows, j], p[rows, j + 1]
            lam = (xk - t[j]) / h
            cdf = np.where(j > 0, C[rows, np.maximum(j - 1, 0)], 0.0) + h * (p0 * lam + (p1 - p0) * (0.5 * (lam * lam)))
            target = np.minimum(u[:, k], 1.0) * tot
            pmax = np.maximum(p0, p1)
            tol = 6.0 * N * U * Bc + 16.0 * U * pmax * h + U * pmax * np.abs(t).max()
            tols[:, k], totals[:, k], pend[:, k, :] = tol, tot, p[:, -2:]
            with np.errstate(all="ignore"):
                bad = ok & ~(np.abs(cdf - target) <= tol)
                worst = max(worst, float(np.max(np.where(ok, np.abs(cdf - target) / tol, 0.0))))
            assert not bad.any(), (f"mode {k + 1}: {int(bad.sum())} samples off", [(int(s), float(xk[s]), int(j[s]), float(cdf[s]), float(target[s]), float(tol[s])) for s in np.flatnonzero(bad)[:5]])
            with np.errstate(all="ignore"):
                num = f0 * p[rows, i] + f1 * p[rows, i + 1]
                pb = S._p_rows(HB[k], stb)
                numb = f0 * pb[rows, i] + f1 * pb[rows, i + 1]
                term = np.where(ok, np.log(num / tot), 0.0)
                ratio = np.where(ok, np.maximum(numb / num, Bc / tot), 1.0)
            logq = logq + term
            lqb = lqb + 4.0 * (N + 3) * U * ratio + 8.0 * U * (1.0 + np.abs(term))
        st = _chain(cores[k], i, f0, f1, st)
        stb = _chain(np.abs(cores[k]), i, f0, f1, stb)
    return dict(logq=np.where(ok, logq, np.nan), val=np.where(ok, st[:, 0], 0.0), logq_bound=lqb, N=N, worst=worst, Z=quad(cores, eff), tol=tols, total=totals,
                pend=pend)


def dense_interpolant(cores, nodes, x):
    """the multilinear interpolant of a small train's dense tensor at the points x (npts, d)"""
    t = S.dense(cores)
    out = np.zeros(x.shape[0])
    for s in range(x.shape[0]):
        v = t
        for k in range(len(cores)):
            v = np.tensordot(hat_row(nodes[k], x[s, k]), v, axes=([0], [0]))
        out[s] = v
    return out
