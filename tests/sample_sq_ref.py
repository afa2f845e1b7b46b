"""Reference for ttx_sample_sq (include/ttx.h), numpy only (test side): the squared-density sampler on grid indices.

tables(cores, w, fixed, gamma) restates the head pass twice, independently:
  * the FACTOR route in float64, as the definition states it: H_k = F_(k-1) G_k, F_k = the R factor (numpy's Householder QR) of the
    rows sqrt(e_k(i)) H_k(a, i, :), or that matrix itself where it has no more rows than columns, scaled by the power of two that
    takes its largest entry into [0.5, 1); rows p(i) = w(i) (sum_a (sum_b H_k(a, i, b) x(b))^2 + g_k);
  * the GRAM route in numpy.longdouble: P_k = sum_i e_k(i) G_k(:, i, :)^T P_(k-1) G_k(:, i, :) from the cores alone, rows
    p(i) = w(i) (y_i^T P_(k-1) y_i + gamma prod_(j<k) W_j), y_i = G_k(:, i, :) x, brought into the factor route's units by the exact
    factor 2^(-2 s_(k-1)).  It squares the conditioning, which is why the device does not take it; in long double (64 bits of
    mantissa) it still serves as the independent check of the float64 factor route.
draw(..) draws by either route.  verify(cores, u, w, fixed, gamma, ind_dev) walks every sample along the DEVICE's indices, as
sample_ref.verify does, so that a difference at one mode cannot cascade, and decides per mode whether the device had a choice.

The allowance of a mode, in the units of the running sum c (the domain of t = u c(n)), has two terms.

1. Rounding of the rows and the sums.  The state x is the device's own: the chain step is TTX_EVAL_EXACT's operation sequence,
   which _step restates operation for operation, so along the device's indices x carries no difference.  Given H and x,
   m(a, i) = sum_b H(a, i, b) x(b) has r_k products and r_k additions: |dm| <= (r_k + 1) u mb(a, i), mb = sum_b |H| |x|, in any
   order of the sum.  s(i) = sum_a m^2: |ds| <= sum_a 2 |m| |dm| + (l_(k-1) + 1) u s <= (2 r_k + l_(k-1) + 3) u sb(i) with
   sb(i) = sum_a mb(a, i)^2 >= s(i).  p = w (s + g) adds two roundings, the running sum over i at most n_k in any association
   order, t = u c(n) and the comparison one each: at most 2 r_k + l_(k-1) + n_k + 8 roundings, which sample_ref.count's
   N = 2 sum_j (r_j + 2) + max n + 4 exceeds (its sum contains 2 (r_k + 2) + 2 (r_(k-1) + 2) and l_(k-1) <= r_(k-1)).  Device
   against reference is 2 N u on each of the two numbers compared, t and an edge c(i): 4 N u Bc(n_k) with
   Bc(n_k) = sum_i w(i) (sb(i) + g), exactly the form of sample_ref's bound with the |H| |x| rows in place of the |cores| chain.

2. The factor pass.  The device's F_(k-1) and numpy's are two computed factors of the same P_(k-1): each satisfies
   F^T F = 2^(-2 s) (P + dP) with ||dP||_2 <= eps_k ||P_(k-1)||_2, where eps_k collects, over the k - 1 bonds behind mode k, the
   product H = F G (r_(j-1) + 1 roundings per element), the multiplication by sqrt(e) (two roundings) and the Householder QR,
   whose columnwise backward error grows with the number of columns r_j that the reflectors sweep: of the order of sum_j (r_j + 2)
   u per factor, doubled because the error enters F^T F twice, doubled again for device against reference: eps_k = 4 N u with
   the same N.  (This is the figure the feature's issue sets; a first-order count, not a rigorous constant.)  A row changes by
   y_i^T dP y_i <= eps_k ||P_(k-1)||_2 ||y_i||^2, the running sum by at most eps_k ||P_(k-1)||_2 sum_i w_k(i) ||y_i||^2, with
   ||P_(k-1)||_2 = ||F_(k-1)||_2^2 in the factor's units.

A mode is DECIDED when t is further than the sum of the two terms from both edges c(i_ref - 1) and c(i_ref) of the reference's own
choice; an edge beyond which no index with p > 0 lies cannot be crossed.  On a decided mode the device's index must be the
reference's; on an undecided one it may also be the neighbouring index with p > 0 on the near side.

logq.  A log term is log(p(i_k) / c(n_k)); p(i_k) and c(n_k) each differ from the reference's by at most the mode's allowance A_k, so
the term differs by at most A_k / p(i_k) + A_k / c(n_k) to first order, plus 8 u (1 + |term|) for the division, the two logs and the
addition (sample_ref's count).  verify returns the sum over the drawn modes as logq_tol."""
import numpy as np

import sample_ref as S

U = S.U
LD = np.longdouble


def _prep(cores, w, fixed):
    cores, w, fixed = S._prep(cores, w, fixed)
    for q in w:
        assert np.all(np.isfinite(q)) and np.all(q >= 0.0), "weights must be finite and non-negative"
    return cores, w, fixed


def tables(cores, w=None, fixed=None, gamma=0.0, gram=True):
    """dict: H[k] (l_k, n_k, r_(k+1)) float64, F2[k] = ||F_k||_2^2, cum[k] = s_k (F_0 = [1], s_0 = 0), g[k] the defensive term of
    0-based mode k in the factor's units, and for the Gram route P[k] (long double, unscaled) and gW[k] = gamma prod_(j<k) W_j"""
    cores, w, fixed = _prep(cores, w, fixed)
    d = len(cores)
    F, cum, gw = np.ones((1, 1)), 0, float(gamma)
    P = np.ones((1, 1), dtype=LD)
    out = dict(H=[], F2=[], cum=[], g=[], P=[], gW=[], l=[])
    for k, (c, q, f) in enumerate(zip(cores, w, fixed)):
        r0, n, r1 = c.shape
        e = np.eye(n)[f - 1] if f else q
        H = np.einsum("xa,aib->xib", F, c)
        out["H"].append(H); out["F2"].append(float(np.linalg.norm(F, 2)) ** 2); out["cum"].append(cum); out["l"].append(F.shape[0])
        with np.errstate(all="ignore"):
            out["g"].append(float(np.ldexp(LD(gw), int(np.clip(-2 * cum, -100000, 100000)))))
        out["P"].append(P); out["gW"].append(LD(gw))
        if k == d - 1:
            break
        A = (np.sqrt(e)[None, :, None] * H).reshape(F.shape[0] * n, r1)
        R = np.linalg.qr(A, mode="r") if A.shape[0] > r1 else A
        m = np.abs(R).max()
        ex = int(np.frexp(m)[1]) if (m > 0.0 and np.isfinite(m)) else 0
        F = np.ldexp(R, -ex)
        cum += ex
        gw = gw * (1.0 if f else float(np.cumsum(q)[-1]))
        if gram:
            cl = c.astype(LD)
            Pn = np.zeros((r1, r1), dtype=LD)
            for i in range(n):
                if e[i] != 0.0:
                    Pn = Pn + LD(e[i]) * (cl[:, i, :].T @ (P @ cl[:, i, :]))
            P = Pn
    return out


def _rows_factor(T, w, k, x):
    """p[s, i] = w(i) (sum_a (sum_b H_k(a, i, b) x[s, b])^2 + g_k), float64"""
    m = np.einsum("aib,sb->sai", T["H"][k], x)
    return w[k][None, :] * ((m * m).sum(1) + T["g"][k])


def _rows_gram(T, cores, w, k, x):
    """the same rows from P_(k-1) in long double, in the factor route's units"""
    y = np.einsum("aib,sb->sai", cores[k].astype(LD), x.astype(LD))
    s = (y * np.einsum("ab,sbi->sai", T["P"][k], y)).sum(1)
    return np.ldexp(w[k].astype(LD)[None, :] * (s + T["gW"][k]), -2 * T["cum"][k])


def draw(cores, u, w=None, fixed=None, gamma=0.0, route="factor"):
    """(ind [npts][d] int32 1-based, logq, val, failed mask) by the definition; route "factor" (float64) or "gram" (long double)"""
    cores, w, fixed = _prep(cores, w, fixed)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    npts, d = u.shape
    T = tables(cores, w, fixed, gamma, gram=route == "gram")
    ind = np.zeros((npts, d), dtype=np.int32)
    logq = np.zeros(npts)
    drawn = np.array([f == 0 for f in fixed])
    with np.errstate(invalid="ignore"):
        failed = ~np.all((u >= 0.0) | ~drawn[None, :], axis=1)
    x = np.ones((npts, 1))
    with np.errstate(all="ignore"):
        for k in range(d - 1, -1, -1):
            if fixed[k]:
                i0 = np.full(npts, fixed[k] - 1)
            else:
                p = _rows_factor(T, w, k, x) if route == "factor" else _rows_gram(T, cores, w, k, x)
                c = np.cumsum(p, axis=1)
                tot = c[:, -1]
                i0 = S._choose(p, c, u[:, k].astype(p.dtype) * tot, u[:, k])
                failed |= ~(tot > 0.0) | np.isinf(tot) | (i0 < 0)
                i0 = np.where(failed, 0, i0)
                logq = logq + np.log(p[np.arange(npts), i0] / tot).astype(np.float64)
            ind[:, k] = i0 + 1
            x = S._step(cores[k], i0, x)
    ind[failed] = 0
    return ind, np.where(failed, np.nan, logq), np.where(failed, 0.0, x[:, 0]), failed


def verify(cores, u, w, fixed, gamma, ind_dev, routes=False):
    """Walk the samples along ind_dev (module docstring).  Raises AssertionError on an index the definition does not allow; returns
    dict(undecided = samples with an undecided mode, mask = which, logq = the reference's logq along the device's indices, logq_tol = its
    allowance per sample, N, and with routes=True gap = the largest |c_factor - c_gram| over all modes, samples and indices as a
    fraction of the mode's allowance)."""
    cores, w, fixed = _prep(cores, w, fixed)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    ind_dev = np.asarray(ind_dev)
    npts, d = u.shape
    N = S.count(cores)
    eps = 4.0 * N * U
    T = tables(cores, w, fixed, gamma, gram=routes)
    ref_failed = draw(cores, u, w, fixed, gamma)[3]
    dev_failed = np.all(ind_dev == 0, axis=1)
    assert np.array_equal(dev_failed, ref_failed), ("failed samples differ", np.flatnonzero(dev_failed != ref_failed)[:10])
    ok = ~dev_failed
    assert np.all((ind_dev[ok] >= 1) & (ind_dev[ok] <= np.array([c.shape[1] for c in cores])[None, :]))
    idx = np.where(ok[:, None], ind_dev - 1, 0)
    x = np.ones((npts, 1))
    undecided = np.zeros(npts, bool)
    logq, logq_tol = np.zeros(npts), np.zeros(npts)
    rows = np.arange(npts)
    gap = 0.0
    for k in range(d - 1, -1, -1):
        i_dev = idx[:, k]
        if fixed[k]:
            assert np.all(ind_dev[ok, k] == fixed[k]), f"mode {k + 1} is fixed at {fixed[k]}"
        else:
            with np.errstate(all="ignore"):
                p = _rows_factor(T, w, k, x)
                c = np.cumsum(p, axis=1)
                t = u[:, k] * c[:, -1]
                mb = np.einsum("aib,sb->sai", np.abs(T["H"][k]), np.abs(x))
                Bc = (w[k][None, :] * ((mb * mb).sum(1) + T["g"][k])).sum(1)
                y = np.einsum("aib,sb->sai", cores[k], x)
                tol = 4.0 * N * U * Bc + eps * T["F2"][k] * (w[k][None, :] * (y * y).sum(1)).sum(1)
                i_ref = np.maximum(S._choose(p, c, t, u[:, k]), 0)
                if routes:
                    cg = np.cumsum(_rows_gram(T, cores, w, k, x), axis=1)
                    dg = (np.abs(c.astype(LD) - cg).max(1) / tol.astype(LD))[ok & (tol > 0.0)]
                    if dg.size:
                        gap = max(gap, float(dg.max()))
            pos = p > 0
            below = np.cumsum(pos, axis=1) - pos                     # indices with p > 0 below i
            above = pos.sum(1)[:, None] - below - pos
            c_lo = np.where(i_ref > 0, c[rows, np.maximum(i_ref - 1, 0)], 0.0)
            c_hi = c[rows, i_ref]
            near_lo = (np.abs(t - c_lo) <= tol) & (below[rows, i_ref] > 0)
            near_hi = (np.abs(t - c_hi) <= tol) & (above[rows, i_ref] > 0) & (u[:, k] < 1.0)
            nb_lo = np.array([np.flatnonzero(pos[s, :i_ref[s]])[-1] if below[s, i_ref[s]] > 0 else -1 for s in range(npts)])
            nb_hi = np.array([i_ref[s] + 1 + np.flatnonzero(pos[s, i_ref[s] + 1:])[0] if above[s, i_ref[s]] > 0 else -1 for s in range(npts)])
            good = (i_dev == i_ref) | (near_lo & (i_dev == nb_lo)) | (near_hi & (i_dev == nb_hi))
            bad = ok & ~good
            assert not bad.any(), (f"mode {k + 1}: {int(bad.sum())} samples off", [(int(s), int(i_dev[s]), int(i_ref[s]), float(t[s]), float(c_lo[s]), float(c_hi[s]), float(tol[s])) for s in np.flatnonzero(bad)[:5]])
            assert np.all(pos[rows, i_dev][ok]), f"mode {k + 1}: an index with p = 0 was drawn"
            undecided |= ok & (near_lo | near_hi)
            with np.errstate(all="ignore"):
                psel = p[rows, i_dev]
                term = np.where(ok, np.log(psel / c[:, -1]), 0.0)
                logq_tol = logq_tol + np.where(ok, tol / psel + tol / c[:, -1] + 8.0 * U * (1.0 + np.abs(term)), 0.0)
            logq = logq + term
        x = S._step(cores[k], i_dev, x)
    return dict(undecided=int(undecided.sum()), mask=undecided, logq=np.where(ok, logq, np.nan), logq_tol=logq_tol, N=N, gap=gap)


def dense_density(cores, w=None, fixed=None, gamma=0.0):
    """(T(i)^2 + gamma) prod w / (Z + gamma prod W) over the drawn modes with the fixed ones held (a fixed mode keeps a singleton
    axis; its weight does not enter), in long double"""
    cores, w, fixed = _prep(cores, w, fixed)
    t = np.asarray(cores[0], dtype=LD)
    for c in cores[1:]:
        t = np.tensordot(t, c.astype(LD), axes=([t.ndim - 1], [0]))
    t = t[0, ..., 0] ** 2 + LD(gamma)
    for k, (q, f) in enumerate(zip(w, fixed)):
        sh = [1] * len(cores)
        if f:
            t = np.take(t, [f - 1], axis=k)
        else:
            sh[k] = q.size
            t = t * q.astype(LD).reshape(sh)
    return t / t.sum()


def chi2_quantile(df, z=4.753424):
    """Wilson-Hilferty: the quantile of chi-square with df degrees of freedom at the normal deviate z (4.753424: 1 - 1e-6)"""
    return df * (1.0 - 2.0 / (9.0 * df) + z * np.sqrt(2.0 / (9.0 * df))) ** 3


def chi2(ind, rho):
    """the statistic of the index rows ind (1-based, no failed ones) against the cell probabilities rho"""
    cnt = np.zeros(rho.shape)
    np.add.at(cnt, tuple((np.asarray(ind) - 1).T), 1.0)
    ex = np.asarray(rho, dtype=np.float64) * len(ind)
    return float(((cnt - ex) ** 2 / ex).sum())


def case(name, signed=False):
    """(cores, u, w) of sample_ref.case with |w| as weights: ttx_sample_sq takes non-negative weights only"""
    cores, u, w = S.case(name, signed)
    return cores, u, [np.abs(q) for q in w]


# the train whose bonds carry the ranks d8_unequal lacks (4, 5, 15, 16), a mode of one index and a rank-1 bond
EDGE_RANKS = ([3, 2, 1, 4, 3, 2], [1, 4, 5, 15, 16, 1, 1])
# the dense identity and the chi-square test: d3 signed, these uniforms
CHI_NPTS, CHI_SEED, CHI_GAMMA = 20000, 20221, 0.25


def edge_case():
    n, r = EDGE_RANKS
    rng = np.random.default_rng(4516)
    cores = [rng.standard_normal((r[k], n[k], r[k + 1])) for k in range(len(n))]
    return cores, rng.random((S.NPTS, len(n))), [rng.uniform(0.5, 1.5, nk) for nk in n]


LONG_BIG = 60


def long_case(npts=200):
    """d = 255, n = 3, rank 8.  The first LONG_BIG cores have entries of size 1e3 and weights of size 1e4: per such mode the prefix
    Gram matrix grows by about 1e6 n r 1e4 and its factor by 5.7 decades, so an unscaled F would pass 1e308 after 54 of them.  The
    state of the chain and its squares are plain doubles (the weights do not enter the state), so T^2 has to stay inside the double
    range: the other 195 cores have entries of size 0.105, which take the state down to about 1e-103 before the large cores take
    it up again by 3.45 decades each, to about 1e104."""
    rng = np.random.default_rng(255)
    d, n, r = 255, 3, 8
    rk = [1] + [r] * (d - 1) + [1]
    cores = [rng.standard_normal((rk[k], n, rk[k + 1])) * (1e3 if k < LONG_BIG else 0.105) for k in range(d)]
    return cores, rng.random((npts, d)), [rng.uniform(0.5, 1.5, n) * (1e4 if k < LONG_BIG else 1.0) for k in range(d)]
