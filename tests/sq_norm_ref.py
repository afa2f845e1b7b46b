"""Reference for ttx_sq_lognorm_grad, ttx_sq_nll_batch and TTCross.fit_density, numpy float64 only (test side).

lognorm_grad restates the definition of include/ttx.h.  cores[k] is U_k of shape (r0, n, r1); md[k] the diagonal of the symmetric
tridiagonal M_k, mo[k] its off-diagonal (None: a diagonal matrix).  numpy's elementwise * and + round once each, every sum is a plain
loop from 0.0 over ascending indices, so this is the operation sequence of TTX_EVAL_EXACT:
    V(a, i, b)   = ((0.0 + mo(i-1) U(a, i-1, b)) + md(i) U(a, i, b)) + mo(i) U(a, i+1, b), a term that does not exist left out
    right, k = d .. 2:  Y(a', i, b) = sum_b' PR_k(b, b') V(a', i, b');   PR_(k-1)(a, a') = sum_i [sum_b U(a, i, b) Y(a', i, b)]
    left,  k = 1 .. d:  W_k(a, i, b') = sum_a' PL_(k-1)(a, a') V(a', i, b');   PL_k(b, b') = sum_i [sum_a U(a, i, b) W_k(a, i, b')]
    (the bracket is summed first, from 0.0, for every i; the brackets are then added over ascending i from 0.0)
    after every step: times 2^-ex, ex = frexp's exponent of the largest |entry| (0 where that is 0 or not finite), exponents summed
    z_mant = PL_d, z_exp = eL(d), den = z_mant + ldexp(gvol, -z_exp), logz = z_exp ln 2 + log(den)
    D_k(a, i, b) = sum_b' W_k(a, i, b') PR_k(b, b'),  s_k = ldexp((2 coef) / den, eL(k-1) + eR(k) - z_exp),  G_k = G0_k + s_k D_k

Allowances, in the house form: count the roundings on the longest path of a term, multiply by u and by the same contraction on absolute
values, and give an evaluation twice its first-order bound.

Chains.  A term of PL_k is a product of entries of U_1 .. U_k (twice each) and M_1 .. M_k.  Through step m it passes the stencil (one
multiply, at most three additions: 4), the product with PL_(m-1) (one multiply, a sum of r_(m-1) terms from 0.0: r_(m-1) + 1) and the
product with U_m (one multiply, a sum of r_(m-1) terms and then a sum of n_m terms: n_m + r_(m-1) + 1); the power of two is exact.  With
one u for the higher orders: left_count(m) = n_m + 2 r_(m-1) + 7, and in the same way right_count(m) = n_m + 2 r_m + 7.  So
    |computed Z - Z| <= NZ u Zabs,   NZ = sum_m left_count(m),   Zabs the chain on |U| and |M|.
Gradient.  W_k carries sum_(m < k) left_count(m) + 4 + (r_(k-1) + 1), PR_k carries sum_(m > k) right_count(m), D_k adds one multiply
and a sum of r_k terms (r_k + 1), s_k D_k one multiply.  s_k = (2 coef) / den: 2 coef and ldexp are exact, den is one addition of a
z_mant that carries NZ u Zabs, the quotient one rounding: to first order |delta s / s| <= (NZ Zabs + 2 (|Z| + gvol)) u / |Z + gvol|.  The
last addition onto G0 rounds once relative to |G_k| <= |G0| + |s| Dabs.  With one u for the higher orders:
    |computed G_k - G_k| <= u [ (NG_k + rel_s) |s_k| Dabs_k + |G0_k| ],
    NG_k = sum_(m < k) left_count(m) + sum_(m > k) right_count(m) + r_(k-1) + r_k + 10,   rel_s = (NZ Zabs + 2 (|Z| + gvol)) / |Z + gvol|
with Dabs_k the contraction on absolute values in the units of D_k.  bound() returns twice that: what the restatement may differ by from
another evaluation of the same definition in any order; the restatement itself sits within half of it of a dense long-double einsum
(checked in test_sq_norm_cpu.py with the factor 1 + 2^-10 for the long-double's own error).
MFMA.  The device's chains are the same kernels in both modes, so W_k, PR_k, s_k are the restatement's bits and only D_k's sum over b'
(r_k terms, one multiply each), the multiply by s_k and the addition onto G0 are evaluated in another order:
    |mfma G_k - restated G_k| <= 2 u [ (r_k + 4) |s_k| A_k + |G0_k| ],   A_k(a, i, b) = sum_b' |W_k(a, i, b')| |PR_k(b, b')|      (mfma_bound)
logz = z_exp ln 2 + log(den): the product is exact to u |z_exp ln 2| (one rounding, ln 2 to u / 2), log is given 2 u |log den| + 2 u (a libm
log is within 1 ulp, den's own rounding moves it by at most u), the sum rounds once: logz_allowance = 4 u (|z_exp| ln 2 + |log den| + 1)
for the same z_mant and z_exp; against a true log(Z + gvol) add rel_s u."""
import numpy as np

U = 2.0 ** -53
LN2 = 0.6931471805599453


def _f(a):
    return np.asarray(a, dtype=np.float64)


def stencil(c, md, mo):
    """V = U x_2 M, the terms i-1, i, i+1 from 0.0"""
    c, md = _f(c), _f(md)
    n = c.shape[1]
    assert md.shape == (n,)
    v = np.zeros(c.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        if mo is not None and n > 1:
            mo = _f(mo)[:n - 1]
            v[:, 1:, :] = v[:, 1:, :] + mo[None, :, None] * c[:, :-1, :]
        v = v + md[None, :, None] * c
        if mo is not None and n > 1:
            v[:, :-1, :] = v[:, :-1, :] + mo[None, :, None] * c[:, 1:, :]
    return v


def pow2(p):
    """(p 2^-ex, ex): k_sq_pow2's rule"""
    a = np.abs(p)
    ex = 0
    if np.all(a <= 1.7976931348623157e308):                                     # NaN and Inf compare false
        m = float(a.max())
        if m > 0.0:
            ex = int(np.frexp(m)[1])
    return np.ldexp(p, -ex), ex


def _clamp(e):
    return int(max(-100000, min(100000, int(e))))


def chains(cores, md, mo):
    """dict(W, PR, eL, eR, z_mant, z_exp): W[k], PR[k] (k = 1 .. d at index k; PR[d] = [1]) as the device holds them"""
    cores = [_f(c) for c in cores]
    d = len(cores)
    mo = [None] * d if mo is None else list(mo)
    PR, eR = [None] * (d + 1), [0] * (d + 1)
    PR[d] = np.ones((1, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(d, 1, -1):
            c = cores[k - 1]
            r0, n, r1 = c.shape
            v = stencil(c, md[k - 1], mo[k - 1])
            y = np.zeros((r0, n, r1))                                           # Y(a', i, b)
            for q in range(r1):
                y = y + PR[k][None, None, :, q] * v[:, :, q, None]
            p = np.zeros((r0, r0))                                              # PR_(k-1)(a, a')
            for i in range(n):
                pi = np.zeros((r0, r0))
                for b in range(r1):
                    pi = pi + c[:, i, b, None] * y[None, :, i, b]
                p = p + pi
            PR[k - 1], ex = pow2(p)
            eR[k - 1] = eR[k] + ex
        W, eL = [None] * (d + 1), [0] * (d + 1)
        pl = np.ones((1, 1))
        for k in range(1, d + 1):
            c = cores[k - 1]
            r0, n, r1 = c.shape
            v = stencil(c, md[k - 1], mo[k - 1])
            w = np.zeros((r0, n, r1))
            for q in range(r0):
                w = w + pl[:, q, None, None] * v[None, q, :, :]
            p = np.zeros((r1, r1))
            for i in range(n):
                pi = np.zeros((r1, r1))
                for a in range(r0):
                    pi = pi + c[a, i, :, None] * w[a, i, None, :]
                p = p + pi
            W[k] = w
            pl, ex = pow2(p)
            eL[k] = eL[k - 1] + ex
    return dict(W=W, PR=PR, eL=eL, eR=eR, z_mant=float(pl[0, 0]), z_exp=int(eL[d]))


def den_of(z_mant, z_exp, gvol):
    return np.float64(z_mant) + np.ldexp(np.float64(gvol), _clamp(-z_exp))


def logz_of(z_mant, z_exp, gvol):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(z_exp) * np.float64(LN2) + np.log(den_of(z_mant, z_exp, gvol)))


def scale_of(ch, k, gvol, coef):
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        q = (np.float64(2.0) * np.float64(coef)) / den_of(ch["z_mant"], ch["z_exp"], gvol)
        return np.ldexp(q, _clamp(ch["eL"][k - 1] + ch["eR"][k] - ch["z_exp"]))


def lognorm_grad(cores, md, mo=None, gvol=0.0, coef=1.0, g0=None, ch=None):
    """(z_mant, z_exp, logz, [G_1 .. G_d]): the definition"""
    cores = [_f(c) for c in cores]
    d = len(cores)
    ch = chains(cores, md, mo) if ch is None else ch
    G = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, d + 1):
            w, pr = ch["W"][k], ch["PR"][k]
            dd = np.zeros(w.shape)
            for q in range(w.shape[2]):
                dd = dd + w[:, :, q, None] * pr[None, None, :, q]
            base = np.zeros(w.shape) if g0 is None else _f(g0[k - 1])
            G.append(base + scale_of(ch, k, gvol, coef) * dd)
    return ch["z_mant"], ch["z_exp"], logz_of(ch["z_mant"], ch["z_exp"], gvol), G


def left_count(c):
    return c.shape[1] + 2 * c.shape[0] + 7


def right_count(c):
    return c.shape[1] + 2 * c.shape[2] + 7


def _abs(cores, md, mo):
    d = len(cores)
    mo = [None] * d if mo is None else list(mo)
    return [np.abs(_f(c)) for c in cores], [np.abs(_f(m)) for m in md], [None if m is None else np.abs(_f(m)) for m in mo]


def rel_s(cores, md, mo, gvol, ch=None):
    """(NZ Zabs + 2 (|Z| + gvol)) / |Z + gvol| in the units of z_exp"""
    ch = chains(cores, md, mo) if ch is None else ch
    ca = chains(*_abs(cores, md, mo))
    nz = sum(left_count(_f(c)) for c in cores)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        zabs = np.ldexp(np.float64(ca["z_mant"]), _clamp(ca["z_exp"] - ch["z_exp"]))
        gv = np.ldexp(np.float64(gvol), _clamp(-ch["z_exp"]))
        return float((nz * zabs + 2.0 * (abs(ch["z_mant"]) + gv)) / abs(ch["z_mant"] + gv))


def bound(cores, md, mo=None, gvol=0.0, coef=1.0, g0=None):
    """2 u [(NG_k + rel_s) |s_k| Dabs_k + |G0_k|] for every core"""
    cores = [_f(c) for c in cores]
    d = len(cores)
    ch, ca = chains(cores, md, mo), chains(*_abs(cores, md, mo))
    rs = rel_s(cores, md, mo, gvol, ch)
    lc, rc = [left_count(c) for c in cores], [right_count(c) for c in cores]
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, d + 1):
            w, pr = ca["W"][k], ca["PR"][k]
            dabs = np.zeros(w.shape)
            for q in range(w.shape[2]):
                dabs = dabs + w[:, :, q, None] * pr[None, None, :, q]
            # into the units of the signed D_k
            dabs = np.ldexp(dabs, _clamp((ca["eL"][k - 1] + ca["eR"][k]) - (ch["eL"][k - 1] + ch["eR"][k])))
            ng = sum(lc[:k - 1]) + sum(rc[k:]) + cores[k - 1].shape[0] + cores[k - 1].shape[2] + 10
            base = 0.0 if g0 is None else np.abs(_f(g0[k - 1]))
            out.append(2.0 * U * ((ng + rs) * abs(scale_of(ch, k, gvol, coef)) * dabs + base))
    return out


def mfma_bound(cores, md, mo=None, gvol=0.0, coef=1.0, g0=None, ch=None):
    """2 u [(r_k + 4) |s_k| A_k + |G0_k|] for every core"""
    cores = [_f(c) for c in cores]
    ch = chains(cores, md, mo) if ch is None else ch
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, len(cores) + 1):
            w, pr = np.abs(ch["W"][k]), np.abs(ch["PR"][k])
            a = np.zeros(w.shape)
            for q in range(w.shape[2]):
                a = a + w[:, :, q, None] * pr[None, None, :, q]
            base = 0.0 if g0 is None else np.abs(_f(g0[k - 1]))
            out.append(2.0 * U * ((w.shape[2] + 4) * abs(scale_of(ch, k, gvol, coef)) * a + base))
    return out


def logz_allowance(z_mant, z_exp, gvol):
    with np.errstate(invalid="ignore", divide="ignore"):
        return 4.0 * U * (abs(z_exp) * LN2 + abs(float(np.log(den_of(z_mant, z_exp, gvol)))) + 1.0)


def tridiag_dense(md, mo):
    md = _f(md)
    m = np.diag(md)
    if mo is not None and md.size > 1:
        mo = _f(mo)[:md.size - 1]
        m = m + np.diag(mo, 1) + np.diag(mo, -1)
    return m


def dense_longdouble(cores, md, mo=None, sub=None):
    """(Z, [dZ/dU_k]) by unscaled long-double einsum chains.  sub = (k, E): <T, T_(U_k <- E)>_M instead of Z (k 0-based), no gradient"""
    ld = np.longdouble
    cs = [_f(c).astype(ld) for c in cores]
    d = len(cs)
    mo = [None] * d if mo is None else list(mo)
    M = [tridiag_dense(md[k], mo[k]).astype(ld) for k in range(d)]
    other = list(cs)
    if sub is not None:
        other[sub[0]] = _f(sub[1]).astype(ld)
    PL = [np.ones((1, 1), dtype=ld)]
    for k in range(d):
        PL.append(np.einsum("ac,aib,ij,cjd->bd", PL[k], cs[k], M[k], other[k]))
    if sub is not None:
        return PL[d][0, 0]
    PR = [None] * (d + 1)
    PR[d] = np.ones((1, 1), dtype=ld)
    for k in range(d - 1, -1, -1):
        PR[k] = np.einsum("bd,aib,ij,cjd->ac", PR[k + 1], cs[k], M[k], cs[k])
    return PL[d][0, 0], [2 * np.einsum("ac,ij,bd,cjd->aib", PL[k], M[k], PR[k + 1], cs[k]) for k in range(d)]


def mass_tridiag(nodes):
    """(md, mo) of the hat functions' mass matrix on ascending nodes: M[i, i] = (h[i-1] + h[i]) / 3 with one term at each end,
    M[i, i+1] = h[i] / 6; a single node gives ([1.], [])"""
    t = _f(nodes)
    if t.size == 1:
        return np.ones(1), np.zeros(0)
    h = t[1:] - t[:-1]
    diag = np.empty(t.size)
    diag[0], diag[-1] = h[0] / 3.0, h[-1] / 3.0
    diag[1:-1] = (h[:-1] + h[1:]) / 3.0
    return diag, h / 6.0


# ---- the negative log-likelihood -------------------------------------------------------------------------------------------------
def dot_rule(a, b):
    """ttx_cores_dot's order (include/ttx.h): 256 segments of L = 256 ceil(tot / 65536); lane t of a segment sums its elements
    e = t (mod 256) ascending from 0.0; the lane sums are halved (t, t + 128) .. (0, 1); the segment sums added ascending from 0.0"""
    a, b = _f(a).ravel(), _f(b).ravel()
    tot = a.size
    L = 256 * ((tot + 65535) // 65536)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = np.zeros(256 * L)
        prod[:tot] = a * b
        lanes = np.zeros((256, 256))
        live = np.zeros(256 * L, dtype=bool)
        live[:tot] = True
        pr, lv = prod.reshape(256, L // 256, 256), live.reshape(256, L // 256, 256)
        for j in range(L // 256):
            lanes = np.where(lv[:, j, :], lanes + pr[:, j, :], lanes)
        o = 128
        while o:
            lanes[:, :o] = lanes[:, :o] + lanes[:, o:2 * o]
            o >>= 1
        s = np.float64(0.0)
        for k in range(256):
            s = s + lanes[k, 0]
    return float(s)


def nll_points(val, w, gamma):
    """(c, lt, wv): c_p = -((2 w_p) val_p) / (val_p val_p + gamma), lt_p = log(val_p val_p + gamma), wv = w or ones"""
    val = _f(val)
    wv = np.ones(val.shape) if w is None else _f(w)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        den = val * val + np.float64(gamma)
        return -((2.0 * wv) * val) / den, np.log(den), wv


def nll_value(lt, wv, logz):
    s, wsum = dot_rule(wv, lt), dot_rule(wv, np.ones(wv.shape))
    with np.errstate(invalid="ignore"):
        return float(-np.float64(s) + np.float64(wsum) * np.float64(logz)), wsum


def nll_allowance(lt, wv, z_mant, z_exp, gvol, val_rel=0.0):
    """|nll - nll'| for two evaluations from the same val, z_mant and z_exp.  S = sum w_p l_p: l_p a libm log of a den that rounds twice
    (2 u relative in den moves log by 2 u; the log itself 1 ulp: u |l_p|), one multiply, a sum of P terms in some tree (P roundings at
    most): (P + 3) u sum w_p (|l_p| + 2), plus val_rel 2 sum w_p for values that differ by val_rel relatively (d log(v^2) = 2 dv / v).
    Wsum is a sum of P terms: P u Wsum, times |logz|.  logz: logz_allowance, times Wsum.  The product and the final sum: 2 u |nll| <=
    2 u (sum w |l| + Wsum |logz|).  Twice the first-order sum, as everywhere."""
    lt, wv = _f(lt), _f(wv)
    p = lt.size
    wsum, logz = float(np.sum(wv)), logz_of(z_mant, z_exp, gvol)
    sabs = float(np.sum(wv * (np.abs(lt) + 2.0)))
    return 2.0 * ((p + 3) * U * sabs + 2.0 * val_rel * wsum + p * U * wsum * abs(logz) + wsum * logz_allowance(z_mant, z_exp, gvol) + 2.0 * U * (sabs + wsum * abs(logz)))


# ---- L-BFGS with a fixed history and Armijo backtracking (TTCross.fit_density restated) ---------------------------------------------
def lbfgs(fun, x0, max_iter=20, history=5, c1=1e-4, shrink=0.5, max_back=20, dot=None):
    """Minimise fun(x) -> (f, g) from the packed x0.  Every scalar operation is one double operation in the order written; dot is the
    fixed-order product (dot_rule).  Iteration: q = g; two-loop recursion over the stored pairs (newest first: al_j = rho_j dot(s_j, q),
    q <- (-al_j) y_j + q; q <- gam q with gam = dot(s, y) / dot(y, y) of the newest pair (1 without pairs); oldest first:
    be = rho_j dot(y_j, q), q <- (al_j - be) s_j + q); direction p = -q; slope = dot(g, p), a slope that is not negative restarts from
    p = -g without pairs.  Step t = 1 (1 / sqrt(dot(g, g)) capped at 1 without pairs), Armijo: accept the first trial with a finite
    f_new <= f + c1 t slope, else t <- shrink t, at most max_back trials (all rejected: stop).  A pair with dot(s, y) > 0 is stored.
    Returns dict(x, f, hist): hist is a list of (f_trial, accepted) for every trial in order."""
    dot = dot_rule if dot is None else dot
    x = _f(x0).copy()
    f, g = fun(x)
    S, Y, R = [], [], []
    hist, fs = [], [f]
    for _ in range(max_iter):
        q = g.copy()
        al = []
        for s, y, rho in zip(reversed(S), reversed(Y), reversed(R)):
            a = rho * dot(s, q)
            al.append(a)
            q = (-a) * y + 1.0 * q
        if S:
            gam = dot(S[-1], Y[-1]) / dot(Y[-1], Y[-1])
            q = gam * q + 0.0 * q
        for (s, y, rho), a in zip(zip(S, Y, R), reversed(al)):
            be = rho * dot(y, q)
            q = (a - be) * s + 1.0 * q
        p = -1.0 * q + 0.0 * q
        slope = dot(g, p)
        if not slope < 0.0:
            S, Y, R = [], [], []
            p = -1.0 * g + 0.0 * g
            slope = dot(g, p)
            if not slope < 0.0:
                break
        t = 1.0
        if not S:
            gn = np.sqrt(dot(g, g))
            t = 1.0 / gn if gn > 1.0 else 1.0
        done = False
        for _b in range(max_back):
            xn = t * p + 1.0 * x
            fn, gn_ = fun(xn)
            ok = bool(np.isfinite(fn) and fn <= f + c1 * t * slope)
            hist.append((fn, ok, f + c1 * t * slope))
            if ok:
                done = True
                break
            t = shrink * t
        if not done:
            break
        s, y = xn + (-1.0) * x, gn_ + (-1.0) * g
        sy = dot(s, y)
        if sy > 0.0:
            S.append(s); Y.append(y); R.append(1.0 / sy)
            if len(S) > history:
                S.pop(0); Y.pop(0); R.pop(0)
        x, f, g = xn, fn, gn_
        fs.append(f)
    return dict(x=x, f=f, hist=hist, fs=fs)


# ---- ttx_sq_nll_batch and fit_density restated ------------------------------------------------------------------------------------
def pack(blocks):
    return np.concatenate([_f(b).ravel(order="F") for b in blocks])


def unpack(flat, shapes):
    out, o = [], 0
    for s in shapes:
        m = int(np.prod(s))
        out.append(_f(flat[o:o + m]).reshape(s, order="F"))
        o += m
    return out


def nll_numpy(cores, x, nodes, w, gamma, md, mo=None, gvol=0.0):
    """dict(nll, logz, val, c, wsum, g, lt, wv, z_mant, z_exp): ttx_sq_nll_batch with ("linear", nodes[k]) in every mode"""
    import basis_core_grad_ref as C
    import basis_ref as B
    cores = [_f(c) for c in cores]
    x = _f(x)
    phis = [B.linear_table(nodes[k], x[:, k]) for k in range(len(cores))]
    val = B.chain(cores, phis)
    c, lt, wv = nll_points(val, w, gamma)
    _, G = C.core_grad_chain(cores, phis, c)
    s, wsum = dot_rule(wv, lt), dot_rule(wv, np.ones(wv.shape))
    zm, ze, lz, G = lognorm_grad(cores, md, mo, gvol, wsum, g0=G)
    with np.errstate(invalid="ignore"):
        nll = float(-np.float64(s) + np.float64(wsum) * np.float64(lz))
    return dict(nll=nll, logz=lz, val=val, c=c, wsum=wsum, g=G, lt=lt, wv=wv, z_mant=zm, z_exp=ze)


def fit_problem(npts=160, seed=11):
    """The pinned problem of the fit tests: d = 3, n = [5, 6, 4], r = [1, 3, 2, 1], hat functions on uneven nodes.  The data are drawn
    by rejection from the square of a smooth positive target train; the start train is that train perturbed.  Returns dict(cores
    (start), nodes, x, w, xh (held-out points), gamma, md, mo, gvol)."""
    rng = np.random.default_rng(seed)
    n, r = [5, 6, 4], [1, 3, 2, 1]
    nodes = [np.cumsum(np.concatenate([[0.0], rng.uniform(0.5, 1.5, nk - 1)])) for nk in n]
    target = [rng.uniform(0.2, 1.0, (r[k], n[k], r[k + 1])) for k in range(3)]
    target[0][:, :2, :] *= 3.0                                                  # mass towards the low end of the first mode
    import basis_ref as B

    def f(cs, pts):
        return B.chain(cs, [B.linear_table(nodes[k], pts[:, k]) for k in range(3)])
    lo, hi = np.array([t[0] for t in nodes]), np.array([t[-1] for t in nodes])
    cand = rng.uniform(lo, hi, (40 * npts, 3))
    dens = f(target, cand) ** 2
    keep = cand[rng.uniform(0.0, dens.max(), dens.size) < dens]
    assert keep.shape[0] >= 2 * npts
    x, xh = keep[:npts].copy(), keep[npts:2 * npts].copy()
    start = [u * (1.0 + 0.6 * rng.uniform(-1.0, 1.0, u.shape)) for u in target]
    md, mo = zip(*[mass_tridiag(t) for t in nodes])
    vol = float(np.prod(hi - lo))
    gamma = 1e-3
    return dict(cores=start, nodes=nodes, x=x, w=rng.uniform(0.5, 1.5, npts), xh=xh, gamma=gamma, md=list(md), mo=list(mo), gvol=gamma * vol)


def fit_density_numpy(prob=None, max_iter=6, history=5, c1=1e-4, shrink=0.5, max_back=20):
    """TTCross.fit_density on the pinned problem, in numpy: dict(nll, hist, iters, cores, allow) -- allow[j] the nll allowance of trial j"""
    prob = fit_problem() if prob is None else prob
    shapes = [u.shape for u in prob["cores"]]
    allow = []

    def fun(flat):
        r = nll_numpy(unpack(flat, shapes), prob["x"], prob["nodes"], prob["w"], prob["gamma"], prob["md"], prob["mo"], prob["gvol"])
        allow.append(nll_allowance(r["lt"], r["wv"], r["z_mant"], r["z_exp"], prob["gvol"]))
        return r["nll"], pack(r["g"])
    res = lbfgs(fun, pack(prob["cores"]), max_iter, history, c1, shrink, max_back)
    return dict(nll=res["fs"], hist=res["hist"], iters=len(res["fs"]) - 1, cores=unpack(res["x"], shapes), allow=allow[1:])
