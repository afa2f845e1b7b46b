"""Reference for ttx_sample_sq_real (include/ttx.h), numpy only (test side): real-valued samples from the square of the interpolant.

tables(cores, nodes, cond, gamma) restates the head pass twice, independently:
  * the FACTOR route in float64, as the definition states it: H_k = F_(k-1) G_k, F_k = the R factor (numpy's Householder QR) of the
    rows dg(i) H_k(a, i, :) + sp(i) H_k(a, i+1, :) with (dg, sp) the bidiagonal Cholesky factor of the mass matrix (mass_cholesky
    below, bit for bit the engine's host code) or, for a held mode, the hat row; scaled by the power of two that takes its largest
    entry into [0.5, 1);
  * the GRAM route in numpy.longdouble with the mass matrices M_k THEMSELVES, not their factors: P_k = sum_(i,i') M_k(i, i')
    G_k(:, i, :)^T P_(k-1) G_k(:, i', :) (for a held mode M = phi phi^T), s(i) = y_i^T P y_i, c(j) = y_j^T P y_(j+1), y_i = G_k(:, i, :) x,
    brought into the factor route's units by the exact factor 2^(-2 s_(k-1)).
draw(..) restates the definition by either route.  verify(cores, nodes, u, cond, gamma, x_dev, cell_dev) walks every sample along
the DEVICE's x in the domain of the conditional CDF, sample_real_ref.verify's scheme: the CDF is continuous, so there is no undecided
allowance.  For every drawn mode, with j = cell_dev - 1, l = (x - t_j) / h_j:
    x_dev in [t_j, t_(j+1)],  A_ref(j) > 0,  |C_ref(j-1) + h_j Q_ref(l) - min(u_k, 1) C_ref(n-2)| <= tol_k.

The allowance tol_k = 6 N u Bc + 4 N u F2 Yc + 64 u qmax h_j + u qmax max|t_k|, u = 2^-53, has sample_sq_ref's two terms and the
cubic inversion's operation count.

1. Rounding of the rows and the sums.  The state x is the device's own (the chain step is restated operation for operation along the
   device's x, as in sample_real_ref).  Given H and x, sample_sq_ref's count gives |ds(i)| <= (2 r_k + l_(k-1) + 3) u sb(i), sb(i) =
   sum_a (sum_b |H| |x|)^2; the same count holds for c(j) with sqrt(sb(j) sb(j+1)) in place of sb (Cauchy-Schwarz), and the clamp
   into [-lim, lim] moves c by no more than lim's own error, two roots and a product on top of s.  The cell mass adds the three
   additions of g, two sums, the division, h_j and the product: eight instead of sample_real_ref's three; the chain carries two
   more per bond, as there.  N = sample_ref.count + 2 d + 8 exceeds the count of any one number.  Device against reference is
   2 N u B on each number compared, and three enter as in sample_real_ref (the target, the running sum with the part inside the
   cell, and the clipped s): 6 N u Bc with Bc = sum_j (((sb(j) + g) + (sqrt(sb(j) sb(j+1)) + g) + (sb(j+1) + g)) / 3) h_j.
2. The factor pass, sample_sq_ref's argument unchanged: device and numpy hold two computed factors of the same P_(k-1), F^T F =
   2^(-2 s) (P + dP), ||dP||_2 <= eps ||P||_2, eps = 4 N u (first order, the figure sample_sq_ref takes; the rows here carry one
   multiply-add more than sqrt(e) H, which N's eight spare roundings cover).  A quadratic form y^T P y' moves by at most eps
   ||P||_2 ||y|| ||y'||, the total by eps F2 Yc, Yc = sum_j ((yy(j) + sqrt(yy(j) yy(j+1)) + yy(j+1)) / 3) h_j, yy(i) = ||y_i||^2.
3. The cubic inversion, a fixed number of operations.  sqr_invert leaves |Q(lambda) - s'| <= 32 u qmax (derived in
   tests/sample_sq_real_main.cpp, which checks it on the host), qmax = max(q0, |qm|, q1); s = T - C(j-1) and s' = s / h_j are two
   roundings of numbers below qmax h_j, lambda h_j one more: 4 u; the reference's own l = (x - t_j) / h_j and its Horner evaluation
   of the cubic in float64 are the same operations as the device's f: 28 u.  Together 64 u qmax h_j in units of mass.  The rounding
   of x = t_j + lambda h_j itself is at most u |x| times the density, which is at most qmax.

logq.  Along the device's x a log term is log(dens / C(n-2)), dens = f0^2 s(i) + 2 f0 f1 c(i) + f1^2 s(i+1) + g.  Numerator and
denominator differ from the reference's by at most 2 (N + 8) u Bnum + 4 N u F2 Ynum (eight more for the products and sums of
dens; Bnum, Ynum: dens on sb and yy) and 2 N u Bc + 4 N u F2 Yc; 8 u (1 + |term|) covers the division, the logs and the sum:
    |logq_dev - logq_ref| <= sum over drawn modes of (tol_num / dens + tol_tot / C(n-2) + 8 u (1 + |term|)).
The last log term's numerator is val^2 + gamma itself (F_0 = [1]), so the identity exp(logq) (Z + gamma V) = val^2 + gamma holds
within (val^2 + gamma) (logq bound + 4 N u) for Z from the dense tensor.  No constant comes from a run of the device code."""
import numpy as np

import sample_real_ref as R
import sample_ref as S

U = S.U
LD = np.longdouble
case = R.case
hat = R.hat


def mass_cholesky(t):
    """(dg, sp) of the definition, one operation at a time"""
    t = np.asarray(t, dtype=np.float64)
    n = t.size
    if n == 1:
        return np.ones(1), np.zeros(1)
    dg, sp = np.zeros(n), np.zeros(n)
    dg[0] = np.sqrt((t[1] - t[0]) / 3.0)
    for i in range(n - 1):
        h = t[i + 1] - t[i]
        sp[i] = (h / 6.0) / dg[i]
        diag = (h + (t[i + 2] - t[i + 1])) / 3.0 if i + 1 < n - 1 else h / 3.0
        dg[i + 1] = np.sqrt(diag - sp[i] * sp[i])
    return dg, sp


def mass_matrix(t):
    """M_k in long double, dense"""
    t = np.asarray(t, dtype=LD)
    n = t.size
    M = np.zeros((n, n), dtype=LD)
    h = np.diff(t)
    for i in range(n - 1):
        M[i, i] += h[i] / LD(3); M[i + 1, i + 1] += h[i] / LD(3)
        M[i, i + 1] += h[i] / LD(6); M[i + 1, i] += h[i] / LD(6)
    return M


def _prep(cores, nodes, cond):
    cores, nodes, held, xh, eff = R._prep(cores, nodes, cond)
    return cores, nodes, held, xh, eff             # eff: the hat row of a held mode (the trapezoid weights of a drawn one are not used)


def tables(cores, nodes, cond=None, gamma=0.0, gram=True):
    """dict: H[k] (l_k, n_k, r_(k+1)) float64, F2[k] = ||F_k||_2^2, cum[k] = s_k, g[k] the defensive term of 0-based mode k in the
    factor's units, and for the Gram route P[k] (long double, unscaled) and gW[k] = gamma prod_(j<k) L_j"""
    cores, nodes, held, xh, eff = _prep(cores, nodes, cond)
    d = len(cores)
    F, cum, gw = np.ones((1, 1)), 0, float(gamma)
    P = np.ones((1, 1), dtype=LD)
    out = dict(H=[], F2=[], cum=[], g=[], P=[], gW=[], l=[])
    for k, (c, t) in enumerate(zip(cores, nodes)):
        r0, n, r1 = c.shape
        H = np.einsum("xa,aib->xib", F, c)
        out["H"].append(H); out["F2"].append(float(np.linalg.norm(F, 2)) ** 2); out["cum"].append(cum); out["l"].append(F.shape[0])
        with np.errstate(all="ignore"):
            out["g"].append(float(np.ldexp(LD(gw), int(np.clip(-2 * cum, -100000, 100000)))))
        out["P"].append(P); out["gW"].append(LD(gw))
        if k == d - 1:
            break
        if held[k]:
            i, f0, f1 = hat(t, np.array([xh[k]]))
            dg, sp = np.zeros(n), np.zeros(n)
            dg[i[0]], sp[i[0]] = f0[0], f1[0]
        else:
            dg, sp = mass_cholesky(t)
        A = dg[None, :, None] * H
        A[:, :-1, :] = A[:, :-1, :] + sp[None, :-1, None] * H[:, 1:, :]
        A = A.reshape(F.shape[0] * n, r1)
        Rf = np.linalg.qr(A, mode="r") if A.shape[0] > r1 else A
        m = np.abs(Rf).max()
        ex = int(np.frexp(m)[1]) if (m > 0.0 and np.isfinite(m)) else 0
        F = np.ldexp(Rf, -ex)
        cum += ex
        gw = gw * (1.0 if held[k] else float(t[-1] - t[0]))
        if gram:
            cl = c.astype(LD)
            M = np.outer(eff[k], eff[k]).astype(LD) if held[k] else mass_matrix(t)
            P = np.einsum("ij,aib,ac,cjd->bd", M, cl, P, cl, optimize=True)
    return out


def _rows_factor(T, k, x):
    """(s [npts][n], c [npts][n-1]) of the definition in float64"""
    m = np.einsum("aib,sb->sai", T["H"][k], x)
    return (m * m).sum(1), (m[:, :, :-1] * m[:, :, 1:]).sum(1)


def _rows_gram(T, cores, k, x):
    """the same from P_(k-1) in long double, in the factor route's units"""
    y = np.einsum("aib,sb->sai", cores[k].astype(LD), x.astype(LD))
    Py = np.einsum("ab,sbi->sai", T["P"][k], y)
    sc = -2 * T["cum"][k]
    return np.ldexp((y * Py).sum(1), sc), np.ldexp((y[:, :, :-1] * Py[:, :, 1:]).sum(1), sc)


def _clamp(s, c):
    with np.errstate(all="ignore"):
        lim = np.sqrt(s[:, :-1]) * np.sqrt(s[:, 1:])
        c = np.where(c > lim, lim, c)
        return np.where(c < -lim, -lim, c)


def _masses(s, c, g, t):
    """(A, q0, qm, q1) per cell; c already clamped"""
    h = np.diff(t).astype(s.dtype)
    q0, qm, q1 = s[:, :-1] + g, c + g, s[:, 1:] + g
    return (((q0 + qm) + q1) / 3.0) * h[None, :], q0, qm, q1


def cubic(q0, qm, q1, l):
    """Q(l) in the device's Horner form"""
    d1, d2 = qm - q0, (q0 - 2.0 * qm) + q1
    return l * (q0 + l * (d1 + l * (d2 / 3.0)))


def invert(q0, qm, q1, sp):
    """sqr_invert of the definition, elementwise (float64)"""
    q0, qm, q1, sp = (np.array(v, dtype=np.float64) for v in np.broadcast_arrays(q0, qm, q1, sp))
    with np.errstate(all="ignore"):
        nan = np.isnan(q0) | np.isnan(qm) | np.isnan(q1) | np.isnan(sp)
        m = np.maximum(np.maximum(q0, q1), np.abs(qm))
        dead = nan | ~(m > 0.0) | ~(m <= 1.7976931348623157e308)
        e = np.frexp(np.where(dead, 1.0, m))[1]
        q0, qm, q1, sp = (np.ldexp(np.where(dead, 1.0, v), -e) for v in (q0, qm, q1, sp))
        zero = dead | ~(sp > 0.0)
        one = ~zero & (sp >= ((q0 + qm) + q1) / 3.0)
        d1, d2 = qm - q0, (q0 - 2.0 * qm) + q1
        d3 = d2 / 3.0
        lo, hi, l = np.zeros(q0.shape), np.ones(q0.shape), np.full(q0.shape, 0.5)
        live = ~(zero | one)
        for _ in range(64):
            if not live.any():
                break
            f = l * (q0 + l * (d1 + l * d3)) - sp
            up = live & (f > 0.0)
            hi = np.where(up, l, hi)
            lo = np.where(live & ~up, l, lo)
            live = live & (f != 0.0)
            ql = q0 + l * (2.0 * d1 + l * d2)
            ln = l - f / ql
            ln = np.where(~(ql > 0.0) | ~((ln > lo) & (ln < hi)), 0.5 * (lo + hi), ln)
            live = live & (ln != l)
            l = np.where(live, ln, l)
    return np.where(zero, 0.0, np.where(one, 1.0, l))


def draw(cores, nodes, u, cond=None, gamma=0.0, route="factor"):
    """(x [npts][d], cell [npts][d] int32, logq, val, failed mask) by the definition; route "factor" (float64) or "gram" (rows in long double)"""
    cores, nodes, held, xh, eff = _prep(cores, nodes, cond)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    npts, d = u.shape
    T = tables(cores, nodes, cond, gamma, gram=route == "gram")
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
                s, c = _rows_factor(T, k, st) if route == "factor" else tuple(v.astype(np.float64) for v in _rows_gram(T, cores, k, st))
                c = _clamp(s, c)
                g = T["g"][k]
                A, q0, qm, q1 = _masses(s, c, g, t)
                C = np.cumsum(A, axis=1)
                tot = C[:, -1]
                Tg = u[:, k] * tot
                j = S._choose(A, C, Tg, u[:, k])
                failed |= ~(tot > 0.0) | np.isinf(tot) | (j < 0)
                j = np.where(failed, 0, j)
                hit = (A > 0) & (Tg[:, None] < C) & (u[:, k:k + 1] < 1.0)
                inside = hit[rows, j]
                h = t[j + 1] - t[j]
                cprev = np.where(j > 0, C[rows, np.maximum(j - 1, 0)], 0.0)
                sm = np.minimum(np.maximum(Tg - cprev, 0.0), A[rows, j])
                lam = np.where(inside, invert(q0[rows, j], qm[rows, j], q1[rows, j], sm / h), 1.0)
                xk = np.minimum(np.maximum(t[j] + lam * h, t[j]), t[j + 1])
                xk = np.where(failed, t[0], xk)
                cell[:, k] = j + 1
            i, f0, f1 = hat(t, xk)
            if not held[k]:
                dens = (((f0 * f0) * s[rows, i] + ((2.0 * f0) * f1) * c[rows, i]) + (f1 * f1) * s[rows, i + 1]) + g
                logq = logq + np.log(np.maximum(dens, 0.0) / tot)
            xs[:, k] = xk
            st = R._chain(cores[k], i, f0, f1, st)
    xs[failed] = np.nan
    cell[failed] = 0
    return xs, cell, np.where(failed, np.nan, logq), np.where(failed, 0.0, st[:, 0]), failed


def count(cores):
    """N of the bound (module docstring)"""
    return S.count(cores) + 2 * len(cores) + 8


def verify(cores, nodes, u, cond, gamma, x_dev, cell_dev, routes=False):
    """Walk the samples along x_dev (module docstring).  Raises AssertionError on a sample the definition does not allow; returns
    dict(logq, val = the reference's along the device's x, logq_bound, N, worst = the largest |CDF_ref(x_dev) - T| / tol met, and with
    routes=True gap = the largest difference of the two routes' running sums C over all modes, samples and cells as a fraction of
    the mode's allowance)."""
    cores, nodes, held, xh, eff = _prep(cores, nodes, cond)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    x_dev, cell_dev = np.asarray(x_dev, dtype=np.float64), np.asarray(cell_dev)
    npts, d = u.shape
    N = count(cores)
    eps = 4.0 * N * U
    T = tables(cores, nodes, cond, gamma, gram=routes)
    ref_failed = draw(cores, nodes, u, cond, gamma)[4]
    dev_failed = np.isnan(x_dev[:, 0])
    assert np.array_equal(dev_failed, ref_failed), ("failed samples differ", np.flatnonzero(dev_failed != ref_failed)[:10])
    assert np.all(np.isnan(x_dev[dev_failed])) and np.all(cell_dev[dev_failed] == 0)
    ok = ~dev_failed
    assert np.all(np.isfinite(x_dev[ok]))
    xw = np.where(ok[:, None], x_dev, np.array([t[0] for t in nodes])[None, :])
    st = np.ones((npts, 1))
    logq, lqb = np.zeros(npts), np.zeros(npts)
    rows = np.arange(npts)
    worst, gap = 0.0, 0.0
    for k in range(d - 1, -1, -1):
        t = nodes[k]
        xk = xw[:, k]
        i, f0, f1 = hat(t, xk)
        if held[k]:
            assert np.all(x_dev[ok, k] == xh[k]), f"mode {k + 1} is held at {xh[k]}"
            assert np.all(cell_dev[:, k] == 0), f"mode {k + 1} is held: cell 0"
        else:
            g = T["g"][k]
            hh = np.diff(t)
            with np.errstate(all="ignore"):
                s, c = _rows_factor(T, k, st)
                c = _clamp(s, c)
                A, q0, qm, q1 = _masses(s, c, g, t)
                C = np.cumsum(A, axis=1)
                tot = C[:, -1]
                mb = np.einsum("aib,sb->sai", np.abs(T["H"][k]), np.abs(st))
                sb = (mb * mb).sum(1)
                cb = np.sqrt(sb[:, :-1] * sb[:, 1:])
                Bc = _masses(sb, cb, g, t)[0].sum(1)
                y = np.einsum("aib,sb->sai", cores[k], st)
                yy = (y * y).sum(1)
                yc = np.sqrt(yy[:, :-1] * yy[:, 1:])
                Yc = _masses(yy, yc, 0.0, t)[0].sum(1)
                tol_tot = 2.0 * N * U * Bc + eps * T["F2"][k] * Yc
            j = np.where(ok, cell_dev[:, k] - 1, 0)
            assert np.all((j >= 0) & (j <= t.size - 2)), f"mode {k + 1}: a cell outside 1 .. n - 1"
            assert np.all((t[j] <= xk) & (xk <= t[j + 1]) | ~ok), f"mode {k + 1}: x outside its cell"
            assert np.all((A[rows, j] > 0) | ~ok), f"mode {k + 1}: a cell without mass was drawn"
            h = hh[j]
            lam = (xk - t[j]) / h
            with np.errstate(all="ignore"):
                cdf = np.where(j > 0, C[rows, np.maximum(j - 1, 0)], 0.0) + h * cubic(q0[rows, j], qm[rows, j], q1[rows, j], lam)
                target = np.minimum(u[:, k], 1.0) * tot
                qmax = np.maximum(np.maximum(q0[rows, j], q1[rows, j]), np.abs(qm[rows, j]))
                tol = 6.0 * N * U * Bc + eps * T["F2"][k] * Yc + 64.0 * U * qmax * h + U * qmax * np.abs(t).max()
                bad = ok & ~(np.abs(cdf - target) <= tol)
                worst = max(worst, float(np.max(np.where(ok, np.abs(cdf - target) / tol, 0.0))))
                if routes:
                    sg, cg = _rows_gram(T, cores, k, st)
                    Cg = np.cumsum(_masses(sg, _clamp(sg, cg), LD(g), t)[0], axis=1)
                    dgp = (np.abs(C.astype(LD) - Cg).max(1) / tol.astype(LD))[ok & (tol > 0.0)]
                    if dgp.size:
                        gap = max(gap, float(dgp.max()))
            assert not bad.any(), (f"mode {k + 1}: {int(bad.sum())} samples off", [(int(q), float(xk[q]), int(j[q]), float(cdf[q]), float(target[q]), float(tol[q])) for q in np.flatnonzero(bad)[:5]])
            with np.errstate(all="ignore"):
                dens = (((f0 * f0) * s[rows, i] + ((2.0 * f0) * f1) * c[rows, i]) + (f1 * f1) * s[rows, i + 1]) + g
                densb = (((f0 * f0) * sb[rows, i] + ((2.0 * f0) * f1) * cb[rows, i]) + (f1 * f1) * sb[rows, i + 1]) + g
                densy = ((f0 * f0) * yy[rows, i] + ((2.0 * f0) * f1) * yc[rows, i]) + (f1 * f1) * yy[rows, i + 1]
                tol_num = 2.0 * (N + 8) * U * densb + eps * T["F2"][k] * densy
                term = np.where(ok, np.log(np.maximum(dens, 0.0) / tot), 0.0)
                lqb = lqb + np.where(ok, tol_num / dens + tol_tot / tot + 8.0 * U * (1.0 + np.abs(term)), 0.0)
            logq = logq + term
        st = R._chain(cores[k], i, f0, f1, st)
    return dict(logq=np.where(ok, logq, np.nan), val=np.where(ok, st[:, 0], 0.0), logq_bound=lqb, N=N, worst=worst, gap=gap)


def dense_Z(cores, nodes):
    """the integral of the squared interpolant over the whole box, from the dense tensor and the mass matrices, in long double"""
    t = S.dense(cores).astype(LD)
    v = t
    for k, tk in enumerate(nodes):
        v = np.moveaxis(np.tensordot(mass_matrix(tk), v, axes=([1], [k])), 0, k)
    return (t * v).sum()


def volume(nodes):
    return float(np.prod([LD(t[-1]) - LD(t[0]) for t in nodes]))


def dense_cell_masses(cores, nodes, gamma=0.0):
    """the probability of every cell of the box under (g^2 + gamma) / (Z + gamma V), long double: per mode the two nodes of a cell
    carry the local mass matrix h [[1/3, 1/6], [1/6, 1/3]]"""
    t = S.dense(cores).astype(LD)
    d = t.ndim
    # pair tensor: out[j_1 .. j_d] = sum over the corners e, e' in {0, 1}^d of prod_k m_k(e_k, e'_k) T[j + e] T[j + e']
    n = t.shape
    out = np.zeros([nk - 1 for nk in n], dtype=LD)
    corners = list(np.ndindex(*([2] * d)))
    sl = lambda e: tuple(slice(ek, n[k] - 1 + ek) for k, ek in enumerate(e))
    for e in corners:
        for f in corners:
            wgt = LD(1)
            for k in range(d):
                wgt = wgt * (LD(1) / 3 if e[k] == f[k] else LD(1) / 6)
            out = out + wgt * t[sl(e)] * t[sl(f)]
    for k, tk in enumerate(nodes):
        sh = [1] * d
        sh[k] = n[k] - 1
        out = out * np.diff(np.asarray(tk, dtype=LD)).reshape(sh)
    vol = np.ones([nk - 1 for nk in n], dtype=LD)
    for k, tk in enumerate(nodes):
        sh = [1] * d
        sh[k] = n[k] - 1
        vol = vol * np.diff(np.asarray(tk, dtype=LD)).reshape(sh)
    out = out + LD(gamma) * vol
    return out / out.sum()


def chi2(cell, rho):
    """the statistic of the 1-based cell rows (no failed ones) against the cell probabilities rho"""
    cnt = np.zeros(rho.shape)
    np.add.at(cnt, tuple((np.asarray(cell) - 1).T), 1.0)
    ex = np.asarray(rho, dtype=np.float64) * len(cell)
    return float(((cnt - ex) ** 2 / ex).sum())


CHI_NPTS, CHI_SEED, CHI_GAMMA = 20000, 20222, 0.25


def chi2_quantile(df, z=4.753424):
    """Wilson-Hilferty: the quantile of chi-square with df degrees of freedom at the normal deviate z (4.753424: 1 - 1e-6)"""
    return df * (1.0 - 2.0 / (9.0 * df) + z * np.sqrt(2.0 / (9.0 * df))) ** 3
