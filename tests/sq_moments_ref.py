"""Reference for ttx_sq_moments, numpy float64 only (test side): moments() restates the definition of include/ttx.h on top of
sq_norm_ref's chains, stencil, pow2 and dot_rule.  cores[k] is U_k (r0, n, r1); md, mo the rows of M_k; ad, ao those of the observable A_k
(ad None: no moments; ad[k] None: mode k not selected); a2d, a2o those of A2_k for the diagonal of c2.  numpy's elementwise * and + round
once each and every sum is a plain loop from 0.0 over ascending indices, so this is the operation sequence of TTX_EVAL_EXACT.

    left step with X from P:   W(a, i, b') = sum_a' P(a, a') V(a', i, b'), V the stencil of X;  p_i(b, b') = sum_a U(a, i, b) W(a, i, b');  sum_i p_i
    right step with X from P:  Y(a', i, b) = sum_b' P(b, b') V(a', i, b');                        p_i(a, a') = sum_b U(a, i, b) Y(a', i, b);  sum_i p_i
    RA_(l-1)  = right step with A_l from PR_l, not rescaled                            m1[l]    = ldexp(dot(PL_(l-1), RA_(l-1)) / z_mant, eL(l-1) + eR(l) - z_exp)
    C^(k)_k   = pow2(left step with A_k from PL_(k-1)),  e = eL(k-1) + ex            C^(k)_j  = pow2(left step with M_j from C^(k)_(j-1)),  e += ex
    c2[k][l]  = ldexp(dot(C^(k)_(l-1), RA_(l-1)) / z_mant, e^(k)_(l-1) + eR(l) - z_exp)  c2[k][k] = m1's formula with A2_k
    T = PL_(k-1) U_k,  D0(a, i, b) = sum_b' T(a, i, b') PR_k(b, b'),  B_k(i, i') = sum_b [sum_a U_k(a, i, b) D0(a, i', b)],  bd, bo = B_k's band over Z

Allowance, in the house form of sq_norm_ref: count the roundings on the longest path of a term, multiply by u and by the same contraction on
absolute values, and give an evaluation twice its first-order bound.  Every output is X = N / Z with N a chain through all d modes.  A term of
N passes a left step in every mode left of the closing bond (left_count(m) = n_m + 2 r_(m-1) + 7 roundings, the observable's stencil counts
as M's), a right step in every mode right of it (right_count(m)), and the closing product: a multiply and a sum of at most rmax^2 terms in
some tree (rmax^2 + 1); for the band the three sums of mode k instead (r0 + 1, r1 + 1, r0 + 1 + r1).  The powers of two are exact.  With
NZ = sum_m left_count(m), NR = sum_m right_count(m):   |computed N - N| <= C u Nabs,   C = NZ + NR + rmax^2 + 4 rmax + 8   (an upper bound of
every path above), Nabs the chain on |U|, |M|, |A|.  Z carries NZ u Zabs (sq_norm_ref); the quotient rounds once, ldexp is exact (the ratios
are O(1)).  To first order, with rho = Zabs / |Z| and Xabs = Nabs / Zabs:
    |computed X - X| <= u [ C Xabs rho + |X| (NZ rho + 1) ]
bound() returns twice that for every output: what the restatement may differ by from another evaluation of the same definition in any
order.  The restatement itself lies within half of it of a dense long-double contraction (test_sq_moments_cpu.py, factor 1 + 2^-10 for the
long double's own error).  MFMA mode evaluates the carried steps in another order (and may fuse a multiply into an add: fewer roundings): it
is such another evaluation, and C grows with every mode a carried matrix crosses, so the allowance compounds over the carried steps."""
import numpy as np

import sq_norm_ref as S

U = S.U


def _f(a):
    return np.asarray(a, dtype=np.float64)


def left_step(c, xd, xo, p):
    """sum_i p_i of one step of the left chain with the rows (xd, xo) from p (r0 x r0): r1 x r1, not rescaled"""
    r0, n, r1 = c.shape
    with np.errstate(invalid="ignore", over="ignore"):
        v = S.stencil(c, xd, xo)
        w = np.zeros((r0, n, r1))
        for q in range(r0):
            w = w + p[:, q, None, None] * v[None, q, :, :]
        out = np.zeros((r1, r1))
        for i in range(n):
            pi = np.zeros((r1, r1))
            for a in range(r0):
                pi = pi + c[a, i, :, None] * w[a, i, None, :]
            out = out + pi
    return out


def right_step(c, xd, xo, p):
    """sum_i p_i of one step of the right chain with the rows (xd, xo) from p (r1 x r1): r0 x r0, not rescaled"""
    r0, n, r1 = c.shape
    with np.errstate(invalid="ignore", over="ignore"):
        v = S.stencil(c, xd, xo)
        y = np.zeros((r0, n, r1))
        for q in range(r1):
            y = y + p[None, None, :, q] * v[:, :, q, None]
        out = np.zeros((r0, r0))
        for i in range(n):
            pi = np.zeros((r0, r0))
            for b in range(r1):
                pi = pi + c[:, i, b, None] * y[None, :, i, b]
            out = out + pi
    return out


def left_chain(cores, md, mo):
    """(PL[0 .. d], eL[0 .. d]): the left chain of sq_norm_ref.chains with every PL_k kept"""
    d = len(cores)
    mo = [None] * d if mo is None else list(mo)
    PL, eL = [np.ones((1, 1))], [0]
    for k in range(d):
        p, ex = S.pow2(left_step(cores[k], md[k], mo[k], PL[k]))
        PL.append(p)
        eL.append(eL[k] + ex)
    return PL, eL


def ratio(dot, z_mant, e):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return float(np.ldexp(np.float64(dot) / np.float64(z_mant), S._clamp(e)))


def band_of(c, pl, pr):
    """(B(i, i), B(i, i+1) with 0.0 at the end) of one mode, unscaled"""
    r0, n, r1 = c.shape
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.zeros((r0, n, r1))
        for q in range(r0):
            t = t + pl[:, q, None, None] * c[None, q, :, :]
        d0 = np.zeros((r0, n, r1))
        for q in range(r1):
            d0 = d0 + t[:, :, q, None] * pr[None, None, :, q]
        ind, ino = np.zeros((n, r1)), np.zeros((max(n - 1, 0), r1))
        for a in range(r0):
            ind = ind + c[a, :, :] * d0[a, :, :]
            ino = ino + c[a, :-1, :] * d0[a, 1:, :]
        bd, bo = np.zeros(n), np.zeros(n)
        for b in range(r1):
            bd = bd + ind[:, b]
            bo[:n - 1] = bo[:n - 1] + ino[:, b]
    return bd, bo


def moments(cores, md, mo=None, ad=None, ao=None, a2d=None, a2o=None, band=True, ch=None):
    """dict(z_mant, z_exp, bd, bo, m1, c2): the definition.  bd, bo lists per mode (None without band); m1 (d,), c2 (d, d)"""
    cores = [_f(c) for c in cores]
    d = len(cores)
    mo = [None] * d if mo is None else list(mo)
    ao = [None] * d if ao is None else list(ao)
    a2o = [None] * d if a2o is None else list(a2o)
    ch = S.chains(cores, md, mo) if ch is None else ch
    PL, eL = left_chain(cores, md, mo)
    PR, eR, zm, ze = ch["PR"], ch["eR"], ch["z_mant"], ch["z_exp"]
    assert eL == list(ch["eL"]) and (PL[d][0, 0] == zm or zm != zm)
    out = dict(z_mant=zm, z_exp=ze, bd=None, bo=None, m1=np.zeros(d), c2=np.zeros((d, d)))
    if band:
        out["bd"], out["bo"] = [], []
        for k in range(1, d + 1):
            bd, bo = band_of(cores[k - 1], PL[k - 1], PR[k])
            e = eL[k - 1] + eR[k] - ze
            out["bd"].append(np.array([ratio(v, zm, e) for v in bd]))
            out["bo"].append(np.array([ratio(v, zm, e) for v in bo[:-1]] + [0.0]))
    sel = [] if ad is None else [k for k in range(1, d + 1) if ad[k - 1] is not None]
    carried = []                                                                # [k, C, e] for every selected k so far
    for j in range(1, (sel[-1] if sel else 0) + 1):
        c = cores[j - 1]
        if j in sel:
            ra = right_step(c, ad[j - 1], ao[j - 1], PR[j])
            out["m1"][j - 1] = ratio(S.dot_rule(PL[j - 1].ravel(order="F"), ra.ravel(order="F")), zm, eL[j - 1] + eR[j] - ze)
            if a2d is not None and a2d[j - 1] is not None:
                ra2 = right_step(c, a2d[j - 1], a2o[j - 1], PR[j])
                out["c2"][j - 1, j - 1] = ratio(S.dot_rule(PL[j - 1].ravel(order="F"), ra2.ravel(order="F")), zm, eL[j - 1] + eR[j] - ze)
            for k, C, e in carried:
                v = ratio(S.dot_rule(C.ravel(order="F"), ra.ravel(order="F")), zm, e + eR[j] - ze)
                out["c2"][k - 1, j - 1] = out["c2"][j - 1, k - 1] = v
        if j == sel[-1]:
            break
        for m in carried:
            m[1], ex = S.pow2(left_step(c, md[j - 1], mo[j - 1], m[1]))
            m[2] += ex
        if j in sel:
            C, ex = S.pow2(left_step(c, ad[j - 1], ao[j - 1], PL[j - 1]))
            carried.append([j, C, eL[j - 1] + ex])
    return out


def steps_of(sel):
    """sum over the selected k below the largest of (l_max - k): the carried chain steps of a call (sel 1-based or 0-based alike)"""
    return sum(max(sel) - k for k in sel) if sel else 0


def _absrows(rows):
    return None if rows is None else [None if m is None else np.abs(_f(m)) for m in rows]


def bound(cores, md, mo=None, ad=None, ao=None, a2d=None, a2o=None, band=True, got=None):
    """dict(bd, bo, m1, c2) of 2 u [C Xabs rho + |X| (NZ rho + 1)], the shapes of moments(); got: the values X to use (default: moments())"""
    cores = [_f(c) for c in cores]
    got = moments(cores, md, mo, ad, ao, a2d, a2o, band) if got is None else got
    ca = [np.abs(c) for c in cores]
    ab = moments(ca, _absrows(md), _absrows(mo), _absrows(ad), _absrows(ao), _absrows(a2d), _absrows(a2o), band)
    nz, nr = sum(S.left_count(c) for c in cores), sum(S.right_count(c) for c in cores)
    rmax = max(max(c.shape[0], c.shape[2]) for c in cores)
    C = nz + nr + rmax * rmax + 4 * rmax + 8
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        rho = float(np.ldexp(np.float64(ab["z_mant"]) / abs(np.float64(got["z_mant"])), S._clamp(ab["z_exp"] - got["z_exp"])))

        def one(x, xabs):
            return 2.0 * U * (C * _f(xabs) * rho + np.abs(_f(x)) * (nz * rho + 1.0))
        out = dict(m1=one(got["m1"], ab["m1"]), c2=one(got["c2"], ab["c2"]), bd=None, bo=None, rho=rho, C=C)
        if band:
            out["bd"] = [one(x, a) for x, a in zip(got["bd"], ab["bd"])]
            out["bo"] = [one(x, a) for x, a in zip(got["bo"], ab["bo"])]
    return out


def band_trace(bd, bo, bbd, bbo, xd, xo):
    """(sum_i bd_i xd_i + 2 sum_i bo_i xo_i, its allowance) for one mode: the moment of the tridiagonal X from the band.  The allowance:
    the band's own bounds (bbd, bbo) times |X|, plus the short sum's rounding, (n + 2) u on the absolute terms, twice"""
    xd = _f(xd)
    xo_ = np.zeros(xd.size) if xo is None else np.concatenate([_f(xo)[:xd.size - 1], [0.0]])
    val = float(np.sum(bd * xd) + 2.0 * np.sum(bo * xo_))
    allow = float(np.sum(bbd * np.abs(xd)) + 2.0 * np.sum(bbo * np.abs(xo_))) + 4.0 * (xd.size + 2) * U * float(np.sum(np.abs(bd * xd)) + 2.0 * np.sum(np.abs(bo * xo_)))
    return val, allow


# ---- the dense long-double contraction ---------------------------------------------------------------------------------------------
def dense_tensor(cores):
    ld = np.longdouble
    t = np.ones((1,), dtype=ld).reshape(1, 1)
    for c in cores:
        t = np.tensordot(t, _f(c).astype(ld), axes=([t.ndim - 1], [0]))
    return t.reshape([c.shape[1] for c in cores])


def _apply(t, k, m):
    return np.moveaxis(np.tensordot(m, t, axes=([1], [k])), 0, k)


def dense_moments(cores, md, mo=None, ad=None, ao=None, a2d=None, a2o=None):
    """dict(Z, m1, c2, B): <T, (A_k x A_l) T>_M / Z and the reduced density matrices B_k / Z (full n x n), long double"""
    ld = np.longdouble
    d = len(cores)
    mo = [None] * d if mo is None else list(mo)
    ao = [None] * d if ao is None else list(ao)
    a2o = [None] * d if a2o is None else list(a2o)
    T = dense_tensor(cores)
    M = [S.tridiag_dense(md[k], mo[k]).astype(ld) for k in range(d)]

    def form(repl):
        t = T
        for k in range(d):
            if k in repl:
                if repl[k] is not None:
                    t = _apply(t, k, repl[k])
            else:
                t = _apply(t, k, M[k])
        return t
    Z = np.sum(T * form({}))
    m1, c2, B = np.zeros(d, dtype=ld), np.zeros((d, d), dtype=ld), []
    for k in range(d):
        others = [j for j in range(d) if j != k]
        B.append(np.tensordot(T, form({k: None}), axes=(others, others)) / Z)
    sel = [] if ad is None else [k for k in range(d) if ad[k] is not None]
    A = {k: S.tridiag_dense(ad[k], ao[k]).astype(ld) for k in sel}
    for x, k in enumerate(sel):
        m1[k] = np.sum(T * form({k: A[k]})) / Z
        if a2d is not None and a2d[k] is not None:
            c2[k, k] = np.sum(T * form({k: S.tridiag_dense(a2d[k], a2o[k]).astype(ld)})) / Z
        for l in sel[x + 1:]:
            c2[k, l] = c2[l, k] = np.sum(T * form({k: A[k], l: A[l]})) / Z
    return dict(Z=Z, m1=m1, c2=c2, B=B)


# ---- moment matrices of the hat functions, by quadrature -----------------------------------------------------------------------------
def moment_tridiag_gl(nodes, power):
    """(d, o) of int x^power phi_i phi_j by 3-point Gauss-Legendre per cell, in long double: exact for these integrands of degree <= 4
    up to the long double's rounding.  The closed forms round about six times relative to h max|t|^power / 3 (diagonal) or / 6
    (off-diagonal), the mass matrix's entries times max|t|^power: the test allows 32 u of that."""
    ld = np.longdouble
    t = _f(nodes).astype(ld)
    n = t.size
    gx = np.array([-np.sqrt(ld(0.6)), ld(0.0), np.sqrt(ld(0.6))])
    gw = np.array([5.0, 8.0, 5.0], dtype=ld) / ld(9.0)
    dg, of = np.zeros(n, dtype=ld), np.zeros(max(n - 1, 0), dtype=ld)
    for i in range(n - 1):
        a, b = t[i], t[i + 1]
        h = b - a
        x = 0.5 * (a + b) + 0.5 * h * gx
        w = 0.5 * h * gw
        p0, p1 = (b - x) / h, (x - a) / h
        dg[i] += np.sum(w * x ** power * p0 * p0)
        dg[i + 1] += np.sum(w * x ** power * p1 * p1)
        of[i] += np.sum(w * x ** power * p0 * p1)
    return dg, of


# ---- the statistics of the sampler test ----------------------------------------------------------------------------------------------
def sample_check(x, mean, cov, nse=5.0):
    """(mean ok, cov ok, worst mean ratio, worst cov ratio): the sample mean of N points against mean within nse standard errors
    sqrt(cov_kk / N) computed from the moments themselves; the sample covariance within nse standard errors from the sample's fourth
    moments, se(c_kl)^2 = (mean of (y_k y_l)^2 - c_kl^2) / N with y the centred sample."""
    x = _f(x)
    N = x.shape[0]
    sm = x.mean(axis=0)
    y = x - sm
    sc = (y.T @ y) / N
    se_m = np.sqrt(np.diag(cov) / N)
    m4 = np.einsum("pk,pl->kl", y * y, y * y) / N
    se_c = np.sqrt(np.maximum(m4 - sc * sc, 0.0) / N)
    rm, rc = np.abs(sm - mean) / se_m, np.abs(sc - cov) / se_c
    return bool(np.all(rm <= nse)), bool(np.all(rc <= nse)), float(rm.max()), float(rc.max())
