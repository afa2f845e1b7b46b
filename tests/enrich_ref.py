"""Reference for ttx_basis_enrich_batch / ttx_basis_enrich_tab, numpy float64 only (test side).

sketch restates steps 1 - 5 of include/ttx.h.  phis[m] is the table of mode m + 1, shape (npts, n_m); c the weights, shape (npts,).
The states X_i and L_i are basis_core_grad_ref.states'.  Bond b = 1 .. d-1 lies between the cores b and b + 1 (1-based); its k_b is
plan_k's, its Omega_b (k_b, n_(b+1), r_(b+1)) is engine.roundsum_omega(seed, b, shape): entry (q, j, bb) from the flat index
q + k_b (j + n_(b+1) bb).  Then
    t_j(q) = sum_bb Omega_b(q, j, bb) X_(b+1)(p, bb), from 0.0 over ascending bb;   z_q(p) = sum_j phi_(b+1, j)(p) t_j(q), from 0.0 over
    ascending j;   Y_b(a, j, q) = sum_p ((c[p] * L_b(p, a)) * (phi_(b, j)(p) * z_q(p))), a plain loop over ascending p from 0.0.
numpy's elementwise * and + round once each, so this is the operation sequence of TTX_EVAL_EXACT.  ynorm2 is basis_jvp_ref.dot(Y, Y)
over the packed (column-major) block.

Bound.  Y_b is G_b of basis_core_grad_ref for the train in which core b + 1 is replaced by Omega_b read as a core of shape
(k_b, n_(b+1), r_(b+1)) -- G_b does not depend on core b itself -- so its terms are followed exactly as there: forward steps of the
cores m < b, (n_m r_(m-1) + 2) u each; backward steps of the cores m > b + 1, (n_m r_m + 2) u each; the Omega step, which multiplies a
term twice (phi * X and Omega, in either order: the definition's Omega * X then phi, or the MFMA's phi * X then Omega) and adds it into
a sum of n_(b+1) r_(b+1) terms: (n_(b+1) r_(b+1) + 2) u, the count of a backward step; the three multiplies and the sum over the
points: P + 4.  That is basis_core_grad_ref.count of the replaced train, and
    |computed Y_b - true| <= N_b u B_b,   two evaluations in different orders differ by at most 2 N_b u B_b,
B_b the same sums on |U|, |phi|, |c|, |Omega|.  Omega is generated exactly (every step of the hash is exact in a double), so it adds
no error of its own.

Steps 6 - 7: new_directions forms Q_b with numpy's Householder QR of [U_b^L | 2^-e Y_b] and enriched assembles the new cores; a QR
leaves signs (and, through R, the order of elimination) open, so tests compare the projector Q_b Q_b^T, never Q_b's bits."""
import math

import numpy as np

import basis_core_grad_ref as C
import basis_jvp_ref as J
import basis_ref as B
from basis_ref import U  # noqa: F401
from ttcross_amd.engine import roundsum_omega


def plan_k(n, r, add):
    """k_b for b = 1 .. d-1 (list of d - 1): max(0, min(add, r(b-1) n(b) - r(b), n(b+1) r(b+1), 128 - r(b)))"""
    d = len(n)
    a = np.broadcast_to(np.asarray(add, dtype=np.int64), (d - 1,))
    return [int(max(0, min(a[b - 1], r[b - 1] * n[b - 1] - r[b], n[b] * r[b + 1], 128 - r[b]))) for b in range(1, d)]


def plan(n, r, add):
    """what tests/enrich_plan_main.cpp prints for a shape: k, the new ranks if every bond takes its k, the state stride ldx (the largest
    of the ranks and the k_b, rounded up to four), S = d ldx, and the QR shapes (rows, cols) of the bonds that take directions"""
    k = plan_k(n, r, add)
    ldx = (max(max(r), max(k)) + 3) // 4 * 4
    return dict(k=k, rnew=[1] + [r[b] + k[b - 1] for b in range(1, len(n))] + [1], ldx=ldx, S=len(n) * ldx,
                qr=[(r[b - 1] * n[b - 1], r[b] + k[b - 1]) for b in range(1, len(n)) if k[b - 1]])


def omegas(n, r, k, seed):
    return [roundsum_omega(seed, b, (k[b - 1], n[b], r[b + 1])) for b in range(1, len(n))]


def _sketch(cores, phis, c, oms):
    cores = [np.asarray(u, dtype=np.float64) for u in cores]
    phis = [np.asarray(p, dtype=np.float64) for p in phis]
    c = np.asarray(c, dtype=np.float64)
    d, npts = len(cores), phis[0].shape[0]
    X, L = C.states(cores, phis)
    Z, Y = [], []
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(1, d):
            om = oms[b - 1]
            k, n2, r2 = om.shape
            z = np.zeros((npts, k))
            for j in range(n2):
                t = np.zeros((npts, k))
                for bb in range(r2):
                    t = t + om[None, :, j, bb] * X[b + 1][:, bb, None]
                z = z + phis[b][:, j, None] * t
            cl = c[:, None] * L[b - 1]
            g = np.zeros((cores[b - 1].shape[0], cores[b - 1].shape[1], k))
            for p in range(npts):
                g = g + cl[p][:, None, None] * (phis[b - 1][p][None, :, None] * z[p][None, None, :])
            Z.append(z)
            Y.append(g)
    return Z, Y


def shape_of(cores):
    return [u.shape[1] for u in cores], [1] + [u.shape[2] for u in cores]


def sketch(cores, phis, c, add, seed):
    """dict(k, z, y, ynorm2, maxabs): steps 1 - 5"""
    n, r = shape_of(cores)
    k = plan_k(n, r, add)
    Z, Y = _sketch(cores, phis, c, omegas(n, r, k, seed))
    return dict(k=k, z=Z, y=Y, ynorm2=[J.dot(y.ravel(order="F"), y.ravel(order="F")) for y in Y],
                maxabs=[float(np.max(np.abs(y))) if y.size else 0.0 for y in Y])


def count(cores, b, k, npts):
    """N_b of the bound, bond b 1-based: basis_core_grad_ref.count of the train with core b + 1 replaced by Omega_b"""
    rep = list(cores)
    rep[b] = np.zeros((k, cores[b].shape[1], cores[b].shape[2]))
    return C.count(rep, b - 1, npts)


def bound(cores, phis, c, add, seed):
    """2 N_b u B_b for every bond: what two evaluations of Y_b in different summation orders may differ by"""
    n, r = shape_of(cores)
    k = plan_k(n, r, add)
    a = lambda Lst: [np.abs(np.asarray(t, dtype=np.float64)) for t in Lst]     # noqa: E731
    _, Bb = _sketch(a(cores), a(phis), np.abs(np.asarray(c, dtype=np.float64)), a(omegas(n, r, k, seed)))
    npts = np.asarray(phis[0]).shape[0]
    return [2.0 * count(cores, b, k[b - 1], npts) * U * Bb[b - 1] for b in range(1, len(cores))]


def dense_longdouble(cores, phis, c, add, seed):
    """Y_b = G2_b Omega_b^T in long double with the two-site gradient G2_b formed explicitly by einsum"""
    ld = np.longdouble
    n, r = shape_of(cores)
    k = plan_k(n, r, add)
    oms = [o.astype(ld) for o in omegas(n, r, k, seed)]
    cores = [np.asarray(u, dtype=np.float64).astype(ld) for u in cores]
    phis = [np.asarray(p, dtype=np.float64).astype(ld) for p in phis]
    c = np.asarray(c, dtype=np.float64).astype(ld)
    d, npts = len(cores), phis[0].shape[0]
    X = [None] * (d + 1)
    X[d] = np.ones((npts, 1), dtype=ld)
    for i in range(d - 1, -1, -1):
        X[i] = np.einsum("ajk,pj,pk->pa", cores[i], phis[i], X[i + 1])
    L = [np.ones((npts, 1), dtype=ld)]
    for i in range(d - 1):
        L.append(np.einsum("pa,ajk,pj->pk", L[i], cores[i], phis[i]))
    out = []
    for b in range(1, d):
        G2 = np.einsum("p,pa,pj,pm,pb->ajmb", c, L[b - 1], phis[b - 1], phis[b], X[b + 1])
        out.append(np.einsum("ajmb,qmb->ajq", G2, oms[b - 1]))
    return out


def new_directions(core, y):
    """(Q_b (r0 n, k), |R| diagonal entries scaled back, e): columns r1 .. r1 + k - 1 of numpy's explicit Householder Q of [U^L | 2^-e Y]"""
    r0, nn, r1 = core.shape
    k = y.shape[2]
    UL = core.reshape((r0 * nn, r1), order="F")
    m = float(np.max(np.abs(y)))
    e = math.frexp(m)[1]
    A = np.hstack([UL, np.ldexp(y.reshape((r0 * nn, k), order="F"), -e)])
    Q, R = np.linalg.qr(A)
    return Q[:, r1:r1 + k], np.ldexp(np.abs(np.diag(R)[r1:r1 + k]), e), e


def enriched(cores, y, added):
    """step 7 with numpy's Q: the new cores for the directions every bond takes (added[b - 1] = k_b or 0)"""
    d = len(cores)
    ka = [0] + list(added) + [0]
    out = []
    for i in range(d):
        r0, nn, r1 = cores[i].shape
        new = np.zeros((r0 + ka[i], nn, r1 + ka[i + 1]))
        new[:r0, :, :r1] = cores[i]
        if ka[i + 1]:
            new[:r0, :, r1:] = new_directions(cores[i], y[i])[0].reshape((r0, nn, ka[i + 1]), order="F")
        out.append(new)
    return out


def projector(Q):
    return Q @ Q.T


def sketch_rank(n, b, k):
    """what the shapes alone allow rank(Y_b) to be: L_b (x) phi_b spans at most prod_(m <= b) n_m directions, phi_(b+1) (x) X_(b+1) at most
    prod_(m > b) n_m, and Y_b has k columns.  Below k the sketch is rank-deficient whatever c and the seed are, and a QR pins down only
    the span of that many directions"""
    return int(min(k, math.prod(n[:b]), math.prod(n[b:])))


def projected(core, y):
    """(M, its singular values): the part of Y_b outside range(U_b^L), rows x k"""
    r0, nn, r1 = core.shape
    UL = core.reshape((r0 * nn, r1), order="F")
    Qu = np.linalg.qr(UL)[0]
    Ym = y.reshape((r0 * nn, -1), order="F")
    M = Ym - Qu @ (Qu.T @ Ym)
    return M, np.linalg.svd(M, compute_uv=False)


def projected_cond(core, y, rank=None):
    """condition number of the part of Y_b outside range(U_b^L), over its first `rank` singular values (all by default): what decides
    how well a QR pins the new span down"""
    s = projected(core, y)[1]
    lo = s[(rank or s.size) - 1]
    return float(s[0] / lo) if lo > 0.0 else math.inf


# ---- the recovery run: a fit that stalls at ranks that are too low, one enrichment, a fit that finishes -----------------------------
def tt_truncate(cores, ranks):
    """the train rounded to the given ranks by the TT-SVD: right-to-left orthogonalisation, then left-to-right truncated SVDs"""
    cores = [np.array(u, dtype=np.float64) for u in cores]
    d = len(cores)
    for i in range(d - 1, 0, -1):
        r0, nn, r1 = cores[i].shape
        Q, R = np.linalg.qr(cores[i].reshape(r0, nn * r1).T)
        cores[i] = Q.T.reshape(-1, nn, r1)
        cores[i - 1] = np.einsum("ajk,lk->ajl", cores[i - 1], R)
    for i in range(d - 1):
        r0, nn, r1 = cores[i].shape
        Um, s, Vt = np.linalg.svd(cores[i].reshape(r0 * nn, r1), full_matrices=False)
        q = min(ranks[i + 1], s.size)
        cores[i] = Um[:, :q].reshape(r0, nn, q)
        cores[i + 1] = np.einsum("ak,kjl->ajl", s[:q, None] * Vt[:q], cores[i + 1])
    return cores


def truth():
    """basis_core_grad_ref.fit_problem()'s second train, the one its targets come from"""
    rng = np.random.default_rng(20240521)
    for k in range(3):
        rng.standard_normal((C.FIT_R[k], C.FIT_N[k], C.FIT_R[k + 1]))
    return [rng.standard_normal((C.FIT_R[k], C.FIT_N[k], C.FIT_R[k + 1])) for k in range(3)]


def recovery_start():
    """(cores of ranks [1, 2, 1, 1], phis, y): the truth truncated below its ranks [1, 3, 2, 1]"""
    _, phis, y = C.fit_problem()
    return tt_truncate(truth(), [1, 2, 1, 1]), phis, y


def recovery_numpy(seed=0, stall_iter=24, after_iter=20):
    """(stalled loss, loss after one enrichment by one direction per bond and a second fit, the ranks then)"""
    cores, phis, y = recovery_start()
    f1 = J.fit_numpy(cores, phis, y, max_iter=stall_iter)
    stalled = float(f1["loss"][f1["iters"]])
    res = B.chain(f1["cores"], phis) - y
    sk = sketch(f1["cores"], phis, res, 1, seed)
    grown = enriched(f1["cores"], sk["y"], sk["k"])
    f2 = J.fit_numpy(grown, phis, y, max_iter=after_iter)
    return stalled, float(f2["loss"][f2["iters"]]), [1] + [u.shape[2] for u in grown]
