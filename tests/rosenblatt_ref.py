"""Reference for ttx_rosenblatt_sq_real (include/ttx.h), numpy only (test side): the forward Rosenblatt map x -> u, logq, val of the
squared interpolant, the way back of ttx_sample_sq_real.

Everything up to the cell masses is sample_sq_real_ref's, imported and not edited: tables (the head pass by the factor route in
float64), _rows_factor, _clamp, _masses, cubic, count, hat and _chain.  walk(cores, nodes, x, cond, gamma) restates the definition
along the GIVEN x, from the last mode to the first with the state x_(d+1) = [1].  A held mode gives u_k = 0.0 and cell 0 and takes
the chain step with the hat row of cond_k.  A drawn mode k with the nodes t, i = hat's cell of x_k (TTX_BASIS_LINEAR's rule),
l = (x_k - t_i) / h_i:
    C = the running sum of the cell masses A (numpy's sequential cumsum),
    inside = min(max(h_i Q(l), 0), A(i)),   Q the cubic in the device's Horner form (cubic; sqr_cdf's scaling by a power of two is
                                            exact in the normal range and is not restated), 0 for l <= 0 and Q(1) for l >= 1,
    u_k = min(max((C(i-1) + inside) / C(n-2), 0), 1),   cell = i + 1,
    log term = log(max(dens, 0) / C(n-2)),   dens = f0^2 s(i) + 2 f0 f1 c(i) + f1^2 s(i+1) + g_k.
A point fails where a drawn coordinate is NaN or outside [t_0, t_(n-1)], or where C(n-2) is 0, negative, NaN or Inf at some mode:
its row of u is NaN, cell 0, logq NaN, val 0.0.  forward(..) returns (u, cell, logq, val, failed) alone.

The allowance.  sample_sq_real_ref's docstring derives, per drawn mode and in units of mass,
    tol_k = 6 N u Bc + 4 N u F2 Yc + 64 u qmax h_j + u qmax max|t_k|,   u = 2^-53,
for the distance between the reference's CDF at the device's x and the target min(u_k, 1) C(n-2).  Here x is GIVEN, the same
numbers to device and reference, so the fourth term, the rounding of x = t_j + lambda h_j, drops out.  The others stay:
1. 6 N u Bc: device against reference is 2 N u Bc on each number compared (N = count(cores), Bc the total on |H| and |state|), and
   the same three enter.  The total C(n-2), by which both divide: an error dC of the total moves u_k C(n-2) by u_k dC <= dC.  The
   running sum C(i-1) together with the part inside the cell: the cubic's weights of q0, qm, q1 times h_i are at most the cell's own
   (Q(l) <= Q(1) termwise on |.|), so both are covered by the bound on C(i), in any association order of the sums (the device adds
   in rounds of 64 by a wave scan, numpy one by one).  The clip of the part inside into [0, A(i)]: where it acts, the distance between
   two of a side's own sums that stand for the same true number.
2. 4 N u F2 Yc: the factor pass, unchanged: device and numpy hold two computed factors of the same P_(k-1).
3. 64 u qmax h_j: the cubic.  The inversion's share (32 u qmax for the residual of sqr_invert and 4 u around it) has no counterpart
   here and is kept as slack; the forward evaluation, l = (x - t_i) / h_i and the Horner form, is the 28 u the derivation already
   counts as the reference's own, now on both sides by the same operations on numbers that differ by the terms above.
So  tol_fwd = 6 N u Bc + 4 N u F2 Yc + 64 u qmax h_j  and, dividing by the reference's total,
    |u_dev - u_ref| <= tol_fwd / C_ref(n-2) + 4 u
per drawn mode: 4 u for the two divisions, each within 1 ulp = 2 u of a quotient that is at most 1.  Clamping into [0, 1] moves
neither side away from the other.
Round trip.  For x = draw(u), sample_sq_real_ref.verify allows |C_ref(j-1) + h_j Q_ref(l) - min(u_k, 1) C_ref(n-2)| <= tol_k along
that x; the left side is this module's numerator before the clip, and the clip only moves it towards the target, which lies in [C(j-1),
C(j)] up to the same allowance.  Against a device's forward map the allowances add: walk returns tol_inv = tol_k beside tol_fwd, and
    |u_fwd - min(u_k, 1)| <= (tol_inv + tol_fwd) / C_ref(n-2) + 4 u
must hold for the reference alone (tests/test_rosenblatt_cpu.py) before it is asked of the device.
logq.  Along a given x the log term is the sampler's expression, so the bound is verify's logq_bound unchanged:
    |logq_dev - logq_ref| <= sum over drawn modes of (tol_num / dens + tol_tot / C(n-2) + 8 u (1 + |term|)),
tol_num = 2 (N + 8) u Bnum + 4 N u F2 Ynum, tol_tot = 2 N u Bc + 4 N u F2 Yc.  A cell without mass has dens = 0 on both sides
(its s and c are sums of exact zeros): the term is -inf on both and is compared for equality.
No constant comes from a run of the device code."""
import numpy as np

import sample_sq_real_ref as Q
from sample_sq_real_ref import _clamp, _masses, _rows_factor, count, cubic, hat, tables

U = Q.U
_chain = Q.R._chain


def walk(cores, nodes, x, cond=None, gamma=0.0):
    """dict: u [npts][d], cell [npts][d] int32, logq, val, failed (mask) by the definition along x; per point and mode (zero on a held
    mode) tol_fwd, tol_inv and total = C(n-2) of the module docstring; logq_bound, N"""
    cores, nodes, held, xh, eff = Q._prep(cores, nodes, cond)
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    npts, d = x.shape
    N = count(cores)
    eps = 4.0 * N * U
    T = tables(cores, nodes, cond, gamma, gram=False)
    drawn = ~np.array(held)
    with np.errstate(invalid="ignore"):
        inbox = np.stack([(x[:, k] >= nodes[k][0]) & (x[:, k] <= nodes[k][-1]) for k in range(d)], axis=1)
    failed = ~np.all(inbox | ~drawn[None, :], axis=1)
    us, cell = np.zeros((npts, d)), np.zeros((npts, d), dtype=np.int32)
    logq, lqb = np.zeros(npts), np.zeros(npts)
    tol_fwd, tol_inv, total = np.zeros((npts, d)), np.zeros((npts, d)), np.zeros((npts, d))
    st = np.ones((npts, 1))
    rows = np.arange(npts)
    with np.errstate(all="ignore"):
        for k in range(d - 1, -1, -1):
            t = nodes[k]
            xk = np.full(npts, xh[k]) if held[k] else np.where(inbox[:, k], x[:, k], t[0])
            i, f0, f1 = hat(t, xk)
            if not held[k]:
                g = T["g"][k]
                s, c = _rows_factor(T, k, st)
                c = _clamp(s, c)
                A, q0, qm, q1 = _masses(s, c, g, t)
                C = np.cumsum(A, axis=1)
                tot = C[:, -1]
                failed |= ~(tot > 0.0) | np.isinf(tot)
                h = t[i + 1] - t[i]
                lam = (xk - t[i]) / h
                q0i, qmi, q1i = q0[rows, i], qm[rows, i], q1[rows, i]
                Ql = np.where(lam <= 0.0, 0.0, np.where(lam >= 1.0, ((q0i + qmi) + q1i) / 3.0, cubic(q0i, qmi, q1i, lam)))
                inside = np.minimum(np.maximum(h * Ql, 0.0), A[rows, i])
                cprev = np.where(i > 0, C[rows, np.maximum(i - 1, 0)], 0.0)
                us[:, k] = np.minimum(np.maximum((cprev + inside) / tot, 0.0), 1.0)
                cell[:, k] = i + 1
                # the allowances: sample_sq_real_ref.verify's quantities along this x
                mb = np.einsum("aib,sb->sai", np.abs(T["H"][k]), np.abs(st))
                sb = (mb * mb).sum(1)
                cb = np.sqrt(sb[:, :-1] * sb[:, 1:])
                Bc = _masses(sb, cb, g, t)[0].sum(1)
                y = np.einsum("aib,sb->sai", cores[k], st)
                yy = (y * y).sum(1)
                yc = np.sqrt(yy[:, :-1] * yy[:, 1:])
                Yc = _masses(yy, yc, 0.0, t)[0].sum(1)
                tol_tot = 2.0 * N * U * Bc + eps * T["F2"][k] * Yc
                qmax = np.maximum(np.maximum(q0i, q1i), np.abs(qmi))
                tol_fwd[:, k] = 6.0 * N * U * Bc + eps * T["F2"][k] * Yc + 64.0 * U * qmax * h
                tol_inv[:, k] = tol_fwd[:, k] + U * qmax * np.abs(t).max()
                total[:, k] = tot
                dens = (((f0 * f0) * s[rows, i] + ((2.0 * f0) * f1) * c[rows, i]) + (f1 * f1) * s[rows, i + 1]) + g
                densb = (((f0 * f0) * sb[rows, i] + ((2.0 * f0) * f1) * cb[rows, i]) + (f1 * f1) * sb[rows, i + 1]) + g
                densy = ((f0 * f0) * yy[rows, i] + ((2.0 * f0) * f1) * yc[rows, i]) + (f1 * f1) * yy[rows, i + 1]
                tol_num = 2.0 * (N + 8) * U * densb + eps * T["F2"][k] * densy
                term = np.log(np.maximum(dens, 0.0) / tot)
                logq = logq + term
                lqb = lqb + np.where(np.isfinite(term), tol_num / dens + tol_tot / tot + 8.0 * U * (1.0 + np.abs(term)), 0.0)
            st = _chain(cores[k], i, f0, f1, st)
    us[failed] = np.nan
    cell[failed] = 0
    return dict(u=us, cell=cell, logq=np.where(failed, np.nan, logq), val=np.where(failed, 0.0, st[:, 0]), failed=failed, tol_fwd=tol_fwd, tol_inv=tol_inv,
                total=total, logq_bound=np.where(failed, 0.0, lqb), N=N)


def forward(cores, nodes, x, cond=None, gamma=0.0):
    """(u [npts][d], cell [npts][d] int32, logq, val, failed mask) by the definition"""
    w = walk(cores, nodes, x, cond, gamma)
    return w["u"], w["cell"], w["logq"], w["val"], w["failed"]


def u_bound(w, extra=None):
    """the bound on |u_dev - u_ref| per point and mode from walk's result w (module docstring); extra: tol_inv for the round trip"""
    tol = w["tol_fwd"] if extra is None else w["tol_fwd"] + extra
    with np.errstate(all="ignore"):
        return np.where(w["total"] > 0.0, tol / np.where(w["total"] > 0.0, w["total"], 1.0), 0.0) + 4.0 * U


def dense_u(cores, nodes, x, gamma=0.0):
    """u [npts][d] of a small train without held modes from its dense tensor in long double, independent of the head pass: the
    conditional CDF of mode k given x_(k+1 .. d) is the integral over the modes before k, by their mass matrices, of the squared
    interpolant plus gamma, integrated along mode k cell by cell (a cubic per cell)"""
    LD = np.longdouble
    t = Q.S.dense(cores).astype(LD)
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    d = t.ndim
    M = [Q.mass_matrix(tk) for tk in nodes]
    out = np.zeros(x.shape, dtype=LD)
    for p in range(x.shape[0]):
        v = t
        for k in range(d - 1, -1, -1):
            tk = np.asarray(nodes[k], dtype=LD)
            w = v
            gw = LD(gamma)
            for j in range(k):
                w = np.moveaxis(np.tensordot(M[j], w, axes=([1], [j])), 0, j)
                gw = gw * (tk.dtype.type(nodes[j][-1]) - tk.dtype.type(nodes[j][0]))
            G = np.tensordot(v, w, axes=(list(range(k)), list(range(k))))
            h = np.diff(tk)
            q0, qm, q1 = np.diag(G)[:-1] + gw, np.diag(G, 1) + gw, np.diag(G)[1:] + gw
            A = (q0 + qm + q1) / LD(3) * h
            i = int(np.clip(np.searchsorted(nodes[k], x[p, k], side="right") - 1, 0, tk.size - 2))
            l = (LD(x[p, k]) - tk[i]) / h[i]
            inside = h[i] * (q0[i] * l + (qm[i] - q0[i]) * l * l + (q0[i] - 2 * qm[i] + q1[i]) * l * l * l / LD(3))
            out[p, k] = (A[:i].sum() + inside) / A.sum()
            row = np.zeros(tk.size, dtype=LD)
            row[i], row[i + 1] = LD(1) - l, l
            v = np.tensordot(v, row, axes=([k], [0]))
    return out
