"""Reference for ttx_basis_jvp_batch / ttx_basis_jvp_tab, the vector operations ttx_cores_dot / ttx_cores_axpby_dev and the solver
ttx_basis_fit_batch / ttx_basis_fit_tab, numpy float64 only (test side).

jvp_chain restates the definition of include/ttx.h.  phis[m] is the table of mode m + 1, shape (npts, n_m); V a list of blocks of the
cores' shapes.  From the last mode to the first, from X = (1), Y = (0.0):
    t_j(a) = sum_k U(a, j, k) X(k),  s_j(a) = sum_k U(a, j, k) Y(k),  v_j(a) = sum_k V(a, j, k) X(k),  each from 0.0 over ascending k;
    z(a) = sum_j phi_j t_j(a),  y(a) = sum_j phi_j (s_j(a) + v_j(a)),  each from 0.0 over ascending j;  X <- z, Y <- y;
val = z(1), dval = y(1) after mode 1.  numpy's elementwise * and + round once each, so this is the operation sequence of
TTX_EVAL_EXACT; the z half is basis_ref.chain's, so val equals it bit for bit.  abs_jvp is the same on |U|, |V|, |phi|: B_J, the sum of
the absolute values of all terms of dval.

Bound.  dval_p is the sum, over the cores i and over all index tuples, of the terms prod_m phi_m [prod_(m != i) U_m] V_i.  Follow one
term of core i.  Through a mode m > i it travels in X, as in basis_ref: multiplied twice, it joins a sum of n_m r_m terms.  At mode i
it enters v_j, and through a mode m < i it travels in Y inside s_j; in both cases it is multiplied twice and joins the sum that forms
y(a), which has the 2 n_m r_m terms of s and v together, in any order (the definition's, or the MFMA's U b_y and V b_x alternating):
at most 2 n_m r_m - 1 additions.  So a mode costs at most 2 n_m r_m + 1 roundings, with the first-order constant rounded up by one u
a factor within (2 n_m r_m + 2) u; errors of incoming states pass linearly through later steps and meet the same factors:
    |computed dval - true| <= N_J u B_J,   N_J = count(cores) = sum_m (2 n_m r_m + 2),
and two evaluations in different orders differ by at most 2 N_J u B_J.  Without negative entries B_J is dval itself: 2 N_J u
relative, and a dropped tile or a missing MFMA of the three shows.

Adjoint identity.  sum_p c_p dval_p = sum_i <G_i, V_i> with G of basis_core_grad_ref.core_grad_chain.  The left side is P values of
jvp_chain weighted and summed (P + 2 more, as in basis_core_grad_ref), the right side d dot products over tot = sum_i size_i terms of
blocks that carry N_i u B_i each; each side is given twice its first-order bound:
    2 (N_J + P + 2) u sum_p |c_p| B_J(p)  +  sum_i 2 (N_i + tot + 1) u <B_i, |V_i|>.

Homogeneity.  f is homogeneous of degree d in the cores, so dval(V = U) = d val; with V = U, B_J = d B (B of basis_ref), and the two
computed sides differ by at most 2 N_J u B_J + 2 d (N + 1) u B (N = basis_ref.count, one more rounding for the product d * val).

dot restates ttx_cores_dot: 256 segments of L = 256 ceil(tot / 65536) elements; in a segment lane t adds the products of its elements
e = t (mod 256) in ascending order from 0.0; the lane sums are halved (t, t + 128) .. (0, 1); the segment sums are added in ascending
order from 0.0.  A slot past the end adds the product +0.0, which changes no bit of a sum that started from +0.0.  axpby restates
y <- (alpha * x) + (beta * y).  fit_numpy restates the controller of ttcross_amd/csrc/ttx_fit_plan.h operation by operation."""
import math

import numpy as np

import basis_core_grad_ref as C
import basis_ref as B
from basis_ref import U  # noqa: F401


def jvp_chain(cores, phis, V):
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    V = [np.asarray(v, dtype=np.float64) for v in V]
    phis = [np.asarray(p, dtype=np.float64) for p in phis]
    assert len(cores) == len(phis) == len(V)
    npts = phis[0].shape[0]
    x, y = np.ones((npts, 1)), np.zeros((npts, 1))
    with np.errstate(invalid="ignore", over="ignore"):
        for c, v, ph in zip(cores[::-1], V[::-1], phis[::-1]):
            r0, n, r1 = c.shape
            assert v.shape == c.shape and ph.shape == (npts, n) and x.shape == (npts, r1)
            z, e = np.zeros((npts, r0)), np.zeros((npts, r0))
            for j in range(n):
                t, s, w = np.zeros((npts, r0)), np.zeros((npts, r0)), np.zeros((npts, r0))
                for k in range(r1):
                    t = t + c[None, :, j, k] * x[:, k, None]
                    s = s + c[None, :, j, k] * y[:, k, None]
                    w = w + v[None, :, j, k] * x[:, k, None]
                z = z + ph[:, j, None] * t
                e = e + ph[:, j, None] * (s + w)
            x, y = z, e
    assert x.shape == (npts, 1)
    return x[:, 0].copy(), y[:, 0].copy()


def abs_jvp(cores, phis, V):
    a = lambda L: [np.abs(np.asarray(t, dtype=np.float64)) for t in L]      # noqa: E731
    return jvp_chain(a(cores), a(phis), a(V))[1]


def count(cores):
    """N_J of the bound: sum_m (2 n_m r_m + 2), r_m the right rank of core m"""
    return sum(2 * c.shape[1] * c.shape[2] + 2 for c in cores)


def bound(cores, phis, V):
    """2 N_J u B_J: what two evaluations of dval in different summation orders may differ by"""
    return 2.0 * count(cores) * U * abs_jvp(cores, phis, V)


def dense_longdouble(cores, phis, V):
    """dval by einsum in long double: sum_i of the chain with core i replaced by V_i"""
    ld = np.longdouble
    cores = [np.asarray(u, dtype=np.float64).astype(ld) for u in cores]
    V = [np.asarray(v, dtype=np.float64).astype(ld) for v in V]
    phis = [np.asarray(p, dtype=np.float64).astype(ld) for p in phis]
    npts = phis[0].shape[0]
    tot = np.zeros(npts, dtype=ld)
    for i in range(len(cores)):
        x = np.ones((npts, 1), dtype=ld)
        for m in range(len(cores) - 1, -1, -1):
            x = np.einsum("ajk,pj,pk->pa", V[m] if m == i else cores[m], phis[m], x)
        tot = tot + x[:, 0]
    return tot


def adjoint_allowance(cores, phis, c, V, B_blocks):
    npts = np.asarray(phis[0]).shape[0]
    tot = sum(np.size(v) for v in V)
    left = 2.0 * (count(cores) + npts + 2) * U * float(np.sum(np.abs(c) * abs_jvp(cores, phis, V)))
    right = sum(2.0 * (C.count(cores, i, npts) + tot + 1) * U * float(np.sum(b * np.abs(v))) for i, (b, v) in enumerate(zip(B_blocks, V)))
    return left + right


def homogeneity_allowance(cores, phis):
    d = len(cores)
    return bound(cores, phis, cores) + 2.0 * d * (B.count(cores) + 1) * U * B.abs_chain(cores, phis)


# ---- the vector operations -------------------------------------------------------------------------------------------------------
def pack(blocks):
    return np.concatenate([np.asarray(b, dtype=np.float64).ravel(order="F") for b in blocks])


def unpack(flat, shapes):
    out, o = [], 0
    for s in shapes:
        m = int(np.prod(s))
        out.append(flat[o:o + m].reshape(s, order="F"))
        o += m
    return out


def dot_seg(tot):
    return 256 * ((tot + 65535) // 65536)


def dot(a, b):
    a, b = np.asarray(a, dtype=np.float64).reshape(-1), np.asarray(b, dtype=np.float64).reshape(-1)
    tot = a.size
    assert b.size == tot
    L = dot_seg(tot)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = np.zeros(256 * max(L, 256))
        prod[:tot] = a * b
        prod = prod[:256 * L].reshape(256, L // 256, 256) if L else np.zeros((256, 0, 256))
        s = np.zeros((256, 256))
        for m in range(prod.shape[1]):
            s = s + prod[:, m, :]
        h = 128
        while h >= 1:
            s = s[:, :h] + s[:, h:2 * h]
            h //= 2
        total = 0.0
        for k in range(256):
            total = total + float(s[k, 0])
    return float(total)


def axpby(alpha, x, beta, y):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.float64(alpha) * np.asarray(x, dtype=np.float64)) + (np.float64(beta) * np.asarray(y, dtype=np.float64))


# ---- the solver ------------------------------------------------------------------------------------------------------------------
FIT_DEFAULTS = dict(max_iter=20, cg_max=40, max_reject=8, lambda0=1.0, lambda_down=0.3, lambda_up=4.0, cg_tol=1e-2, loss_tol=0.0)


def fit_loss(cores, phis, y, w):
    val = B.chain(cores, phis)
    res = val - y
    c = res if w is None else w * res
    return 0.5 * dot(c, res), c


def fit_numpy(cores, phis, y, w=None, **opts):
    """the controller of ttx_fit_plan.h: dict(loss, lambda_, cg_iters, accepted, iters, stop, cores, n_jvp, n_core_grad)"""
    o = dict(FIT_DEFAULTS)
    o.update(opts)
    cores = [np.array(u, dtype=np.float64) for u in cores]
    shapes = [u.shape for u in cores]
    mi = o["max_iter"]
    hl, hlam, hcg, hacc = np.zeros(mi + 1), np.zeros(mi), np.zeros(mi, dtype=np.int32), np.zeros(mi, dtype=np.int32)
    n_jvp = n_cg = 0
    lam, it, stop, rejects, have_g = float(o["lambda0"]), 0, 1, 0, False
    cur, c = fit_loss(cores, phis, y, w)
    hl[0] = cur
    g = rho0 = None
    if not math.isfinite(cur):
        stop = 5
    elif cur <= o["loss_tol"]:
        stop = 2
    else:
        while it < mi:
            if not have_g:
                g = pack(C.core_grad_chain(cores, phis, c)[1])
                n_cg += 1
                rho0 = dot(g, g)
                have_g = True
                if rho0 == 0.0:
                    stop = 3
                    break
            lam_it = lam
            s = np.zeros_like(g)
            r = axpby(-1.0, g, 1.0, np.zeros_like(g))
            p = r.copy()
            rho, passes, updates = rho0, 0, 0
            for _ in range(o["cg_max"]):
                q = jvp_chain(cores, phis, unpack(p, shapes))[1]
                n_jvp += 1
                passes += 1
                Ap = pack(C.core_grad_chain(cores, phis, q if w is None else w * q)[1])
                n_cg += 1
                Ap = axpby(lam_it, p, 1.0, Ap)
                pAp = dot(p, Ap)
                if not (pAp > 0.0) or not math.isfinite(pAp):
                    break
                alpha = rho / pAp
                s = axpby(alpha, p, 1.0, s)
                updates += 1
                r = axpby(-alpha, Ap, 1.0, r)
                rho_new = dot(r, r)
                if rho_new <= (o["cg_tol"] * o["cg_tol"]) * rho0:
                    break
                p = axpby(1.0, r, rho_new / rho, p)
                rho = rho_new
            accepted = False
            if updates > 0:
                trial_cores = [u + 1.0 * sb for u, sb in zip(cores, unpack(s, shapes))]
                trial, tc = fit_loss(trial_cores, phis, y, w)
                if math.isfinite(trial) and trial < cur:
                    accepted, cur, cores, c = True, trial, trial_cores, tc
            if accepted:
                lam, rejects, have_g = lam * o["lambda_down"], 0, False
            else:
                lam, rejects = lam * o["lambda_up"], rejects + 1
            hlam[it], hcg[it], hacc[it], hl[it + 1] = lam_it, passes, int(accepted), cur
            it += 1
            if accepted and cur <= o["loss_tol"]:
                stop = 2
                break
            if rejects >= o["max_reject"]:
                stop = 4
                break
    for k in range(it, mi):
        hl[k + 1], hlam[k], hcg[k], hacc[k] = cur, lam, 0, 0
    return dict(loss=hl, lambda_=hlam, cg_iters=hcg, accepted=hacc, iters=it, stop=stop, cores=cores, n_jvp=n_jvp, n_core_grad=n_cg)


def perturbed_truth(seed, rel=0.1):
    """basis_core_grad_ref.fit_problem()'s truth train (the one its targets come from) with every entry changed by up to rel of itself"""
    rng = np.random.default_rng(20240521)
    for k in range(3):
        rng.standard_normal((C.FIT_R[k], C.FIT_N[k], C.FIT_R[k + 1]))
    truth = [rng.standard_normal((C.FIT_R[k], C.FIT_N[k], C.FIT_R[k + 1])) for k in range(3)]
    pr = np.random.default_rng(seed)
    return [u * (1.0 + rel * pr.uniform(-1.0, 1.0, u.shape)) for u in truth]
