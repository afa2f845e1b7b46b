"""Plain high-precision reference for the table evaluators of TTX_ARITH=fast (ttcross_amd/csrc/ttx_fast.h), with a derived
first-order rounding bound per value.  mpmath at 60 digits; nothing here is fitted to an observed error.

Definitions (oracle/ttx_oracle.c: ttxo_fun; ttx_kernels.h: f_ising, f_mvn)
--------------------------------------------------------------------------
Ising D/E, multi-index (x_1 .. x_m) with weights (w_1 .. w_m):  a = prod over ALL contiguous ranges [s,e] of g(u)^2,
g(u) = (1-u)/(1+u), u = x_s ... x_e;  b = 1/(v w), v = 1 + sum of suffix products, w = 1 + sum of prefix products;
D: f = 2 a b w_1...w_m, E: f = 2 a w_1...w_m.
mvn:  f = exp(-Q/2) / norm,  Q = dv' S dv,  dv = fl(x - mu) (one fp64 subtraction, the same in every evaluator: taken as data),
S = fl((C + C')/2) entry by entry as create_integrand_tables forms it, norm = sqrt((2 pi)^d det) with the fp64 constant pi
the sources use.

Tables of a pivot (ttx_fast.h), nodes xs[0..len) in natural order, the bond behind the last (side 0) or before the first (side 1):
near[t] = product of the t dims nearest to the bond (near[0] = 1); N = number of leading entries above 2^-54;
T = prod g(u) over the ranges inside the pivot; W = product of weights; S = sum_{t>=1} near[t]; P = sum of the products that
start at the far end (prefix products on the left, suffix products on the right); F = product of all nodes.
mvn: dv, Y = S dv (all m rows), Q = dv' S dv over the pivot's dims.

The bound (eps = 2^-53, first order, the sum multiplied by 2 for the second-order terms)
----------------------------------------------------------------------------------------
rho = prod g(u) is formed as N/D, N = prod (1-u), D = prod (1+u), in whatever association.
 * A KEPT range of L dims.  Its argument is a product of L nodes, at most L roundings whatever the association (scratch scan,
   child update x * near_p[t-1], (x_j near_L[a]) * (x_k near_R[t]) inside an fma): relative error L eps, which the factors
   1 -/+ u amplify by u/(1-u) and u/(1+u).  One rounding for each of the two factors (1 -/+ u or the fma), one for each
   multiplication into N and D:   (4 + L u/(1-u) + L u/(1+u)) eps.
 * A DROPPED range (argument at or below 2^-54; every scan stops there, arguments are non-increasing): the missing factor is
   (1+u)/(1-u) = 1 + 2u/(1-u) <= 1 + 2^-53 (1 + ...):   2u/(1-u).
   A range whose exact argument lies within 4 L eps of the cut may be either: the larger of the two.
 * Every wave product is a tree of at most 63 further multiplications (63 eps); a table entry from scratch takes two (N, D) and
   one division; a child step multiplies the parent's T by its own N/D: 2*63 + 2 per step.  The fixed side of a fiber adds one
   more N/D (2*63 + 2), the scalar products of rho and de_fast_value at most 16.
 * Weights: m multiplications and two wave trees:  (m + 130) eps.
 * b (D only): v and w are sums of at most m + 1 positive terms, each a product of at most m nodes, formed with at most m + 4
   additions (de_fast_b: 1 + P + F x_j (1 + x_k (1 + S)) and its mirror image; point route: the running sums), so each has
   relative error (2m + 10) eps plus the terms left out at the cut -- each such term IS one prefix / suffix product of the
   full multi-index at or below 2^-54 (S, P stop there; the child's P adds F only above the cut), compared with v, w >= 1:
   their exact sum.  Then one multiplication and one division.
 value = 2 b (rho W) rho:  relative bound  2 [2 err(rho) + err(W) + err(b) + 8 eps].
mvn: Q is a sum of at most (d + 2)^2 products S_ab d_a d_b regrouped as Q_L + Q_R + 2 X + ..., every partial sum a chain of at
most c d fused or plain operations with c = 4 (Y by len fmas, Q by len more and a wave tree, the cross term by p, the scalar
part by 16): |dQ| <= (4 d + 16) eps sum |S_ab d_a d_b|.  exp(-Q/2) turns |dQ|/2 into a relative error; ttx_exp.h states that
ttx_exp is the run-time library's exp bit for bit, whose documented error is below 1 ulp = 2 eps; the division 1 eps; norm (integer
power by squaring, one product, one square root) 12 eps.
Table entries: near[t]: t eps; T: as rho; W, F: (len + 63) eps; S, P: absolute, (2 len + 8) eps times the sum plus the exact sum
of the terms at or below the cut; Y[row]: (len + 2) eps sum_k |S_row,k d_k|; Q: (4 len + 8) eps sum |S_ab d_a d_b|; all times 2.

The exact evaluation order of the oracle (every range by (u-1)/(u+1), squared, multiplied into a; mvn: d^2 additions) gets a bound of
the same kind (`oracle_rel`): per range (8 + 2 L u/(1-u) + 2 L u/(1+u)) eps (+ 4u/(1-u) where the factor is exactly 1 in
fp64), (2m + 10) eps for each of v, w, m + 4 multiplications; mvn: (d^2 + 3) eps sum |C_ab d_a d_b| / 2 plus one eps of the
symmetrised matrix.
"""
import mpmath as mp
import numpy as np

DPS = 60          # every public function works at this precision whatever the caller's mpmath context says
EPS = 2.0 ** -53
CUT = 2.0 ** -54
PI = 3.141592653589793
M1 = mp.mpf(1)


def _pow2(x):
    return x == 0.0 or np.frexp(x)[0] == 0.5


def _contrib(u, L):
    """relative error of rho from one range with (float of the) exact argument u over L dims"""
    if u >= 1.0 or u <= 0.0:
        return 0.0
    kept = (4.0 + L * u / (1.0 - u) + L * u / (1.0 + u)) * EPS
    if u > CUT * (1.0 + 4 * L * EPS):
        return kept
    drop = 2.0 * u / (1.0 - u) * (1 + 1e-9)
    return drop if u < CUT * (1.0 - 4 * L * EPS) else max(kept, drop)


def _ranges(x):
    """N = prod(1-u), D = prod(1+u) over all contiguous ranges of the mp values x, the summed range contributions of the fast
    evaluators and those of the oracle's chain"""
    N, D, c, o = M1, M1, 0.0, 0.0
    m = len(x)
    for s in range(m):
        u = M1
        for e in range(s, m):
            u = u * x[e]
            o += 8 * EPS                                      # the oracle's chain: see oracle_rel
            if u == 0:
                o += 8 * EPS * (m - 1 - e)
                break
            N = N * (1 - u); D = D * (1 + u)
            uf, L = float(u), e - s + 1
            c += _contrib(uf, L)
            if uf < 1.0:
                o += (2 * L * uf / (1 - uf) + 2 * L * uf / (1 + uf)) * EPS + (4 * uf / (1 - uf) if uf < 4 * CUT else 0.0)
    return N, D, c, o


def _split(par, n):
    par = np.asarray(par, dtype=np.float64)
    return par[:n], par[n:2 * n], int(par[2 * n])


def _cutsum(terms):
    """(exact sum, sum of the terms at or below the cut window) of positive mp terms"""
    tot, drop = mp.mpf(0), 0.0
    for k, t in enumerate(terms):
        tot += t
        if float(t) <= CUT * (1 + 4 * (k + 1) * EPS):
            drop += float(t) * (1 + 1e-9)
    return tot, drop


@mp.workdps(DPS)
def ising_de_detail(par, n, ind):
    nodes, weights, fid = _split(par, n)
    x = [mp.mpf(float(nodes[i - 1])) for i in ind]
    w = [mp.mpf(float(weights[i - 1])) for i in ind]
    m = len(x)
    N, D, c, orc = _ranges(x)
    rho = N / D
    W = M1
    for t in w:
        W = W * t
    pre, suf, u, v = [], [], M1, M1
    for k in range(m):
        u = u * x[k]; v = v * x[m - 1 - k]
        pre.append(u); suf.append(v)
    sw, dw = _cutsum(pre)
    sv, dv = _cutsum(suf)
    b = 1 / ((1 + sv) * (1 + sw)) if fid == 2 else M1
    val = 2 * rho * rho * b * W
    err_b = (2 * (2 * m + 10) * EPS + dw + dv + 2 * EPS) if fid == 2 else 0.0
    orc += (2 * (2 * m + 10) * EPS + 2 * EPS if fid != 3 else 0.0) + (m + 4) * EPS
    return dict(value=val, rho=rho, ranges=c, err_b=err_b, m=m, oracle_rel=2 * orc)


def ising_de(par, n, ind):
    """the Ising D/E integrand (id = par[2n]: 2 = D, 3 = E) at the 1-based multi-index ind, by the definition"""
    return ising_de_detail(par, n, ind)["value"]


def ising_elem_bound(det, len_l, len_r, mode, route):
    """relative bound of a fast-mode value given ising_de_detail of its multi-index; route 'lottery', 'col', 'row' or 'point'"""
    m = det["m"]
    if route == "point":
        tree = (2 * 63 + 4) * EPS
    else:
        tree = ((len_l + len_r) * (2 * 63 + 2) if mode == "chain" else 2 * (2 * 63 + 1)) * EPS + 16 * EPS
        if route != "lottery":
            tree += (2 * 63 + 2) * EPS
    return 2 * (2 * (det["ranges"] + tree) + (m + 130) * EPS + det["err_b"] + 8 * EPS)


@mp.workdps(DPS)
def ising_pivot(par, n, idx, side, mode="scratch"):
    """table reference of one pivot: idx = its 1-based mode indices in natural order.  Values are mp numbers, *_rel relative and
    *_abs absolute bounds (floats); count = exact number of near entries above 2^-54, count_safe = no entry sits within rounding
    of the cut (entries that are products of powers of two are exact, so never unsafe)."""
    nodes, weights, _ = _split(par, n)
    xf = [float(nodes[i - 1]) for i in idx]
    x = [mp.mpf(t) for t in xf]
    ln = len(x)
    order = list(range(ln - 1, -1, -1)) if side == 0 else list(range(ln))     # from the bond outwards
    near, u, exact, safe, count = [M1], M1, True, True, 1
    alive = True
    for t, k in enumerate(order, start=1):
        u = u * x[k]
        exact = exact and _pow2(xf[k])
        near.append(u)
        uf = float(u)
        if not exact and abs(uf / CUT - 1.0) <= 4 * t * EPS:
            safe = False
        alive = alive and uf > CUT
        if alive:
            count = t + 1
    N, D, c, _ = _ranges(x)
    tree = (ln * (2 * 63 + 2) if mode == "chain" else 2 * 63 + 1) * EPS
    W = M1
    for i in idx:
        W = W * mp.mpf(float(weights[i - 1]))
    S, dS = _cutsum(near[1:])
    far, u = [], M1
    for k in (range(ln) if side == 0 else range(ln - 1, -1, -1)):
        u = u * x[k]
        far.append(u)
    P, dP = _cutsum(far)
    F = near[ln]
    return dict(near=near, near_rel=[2 * t * EPS for t in range(ln + 1)], count=count, count_safe=safe,
                T=N / D, T_rel=2 * (c + tree), W=W, W_rel=2 * (ln + 63) * EPS, F=F, F_rel=2 * (ln + 63) * EPS,
                S=S, S_abs=2 * ((2 * ln + 8) * EPS * float(S) + dS), P=P, P_abs=2 * ((2 * ln + 8) * EPS * float(P) + dP))


# ---- mvn ---------------------------------------------------------------------------------------------------------------
class Mvn:
    @mp.workdps(DPS)
    def __init__(self, aux, d):
        aux = np.asarray(aux, dtype=np.float64)
        self.d = d
        self.mu = aux[:d].copy()
        self.C = aux[d:d + d * d].reshape(d, d, order="F").copy()
        self.S = 0.5 * (self.C + self.C.T)                    # fp64, entry by entry as create_integrand_tables
        self.det = float(aux[d + d * d])
        self.norm = mp.sqrt(mp.mpf(2.0 * PI) ** d * mp.mpf(self.det))
        self.Smp = [[mp.mpf(float(self.S[a, b])) for b in range(d)] for a in range(d)]

    def dv(self, par, ind, d0=0):
        par = np.asarray(par, dtype=np.float64)
        return np.array([par[i - 1] - self.mu[d0 + k] for k, i in enumerate(ind)], dtype=np.float64)

    @mp.workdps(DPS)
    def quad(self, dv, d0=0):
        """(Q, sum |S_ab d_a d_b|) over the dims d0 .. d0+len"""
        q, a = mp.mpf(0), 0.0
        z = [mp.mpf(float(t)) for t in dv]
        for i in range(len(z)):
            for j in range(len(z)):
                q += self.Smp[d0 + i][d0 + j] * z[i] * z[j]
                a += abs(float(self.S[d0 + i, d0 + j]) * float(dv[i]) * float(dv[j]))
        return q, a

    @mp.workdps(DPS)
    def detail(self, par, ind):
        d = self.d
        dv = self.dv(par, ind)
        q, a = self.quad(dv)
        val = mp.exp(-q / 2) / self.norm
        rel = 2 * ((4 * d + 16) * EPS * a / 2 + 2 * EPS + EPS + 12 * EPS)
        ac = float(np.abs(self.C * np.outer(dv, dv)).sum())
        orc = 2 * ((d * d + 3) * EPS * ac / 2 + EPS * a / 2 + 2 * EPS + EPS + 12 * EPS)
        return dict(value=val, rel=rel, oracle_rel=orc)

    @mp.workdps(DPS)
    def pivot(self, par, idx, d0):
        """table reference of a pivot over dims d0 .. d0+len: dv (fp64, exact), Y [d] with absolute bounds, Q with its bound"""
        d, ln = self.d, len(idx)
        dv = self.dv(par, idx, d0)
        z = [mp.mpf(float(t)) for t in dv]
        Y, Yb = [], []
        for row in range(d):
            Y.append(sum((self.Smp[row][d0 + k] * z[k] for k in range(ln)), mp.mpf(0)))
            Yb.append(2 * (ln + 2) * EPS * float(sum(abs(float(self.S[row, d0 + k]) * float(dv[k])) for k in range(ln))))
        q, a = self.quad(dv, d0)
        return dict(dv=dv, Y=Y, Y_abs=Yb, Q=q, Q_abs=2 * (4 * ln + 8) * EPS * a)


def mvn(par, aux, ind):
    """the mvn density of the drivers at the 1-based multi-index ind (par = nodes, aux = mu, inverse covariance, det)"""
    return Mvn(aux, len(ind)).detail(par, ind)["value"]


# ---- the inputs of tests/test_gpu_fast_elements.py, checked without a GPU by tests/test_fast_ref_cpu.py ---------------------------
def _pick(rng, n, r, ln):
    return rng.integers(1, n + 1, size=(r, ln)).astype(np.int32)


def _from_bond(side, seq, ln, fill):
    """natural-order index row of a pivot given its indices listed FROM THE BOND OUTWARDS (padded with `fill` at the far end)"""
    s = list(seq) + [fill] * (ln - len(seq))
    return s[::-1] if side == 0 else s


def _par(nodes, weights, fid):
    return np.array(list(nodes) + list(weights) + [float(fid)])


def ising_cases():
    """list of dict(name, d, n, par, p, left, right, caps, points [, counts: hand-computed FP_N per side])"""
    out = []
    rng = np.random.default_rng(20240607)
    w5 = [1.0, 0.7, 1.3, 1.9, 0.55]
    for fid in (2, 3):
        par = _par([0.9, 0.5, 0.25, 0.07, 0.6], w5, fid)
        for d, bonds in ((3, (1, 2)), (4, (1, 2, 3)), (6, (1, 3, 5))):
            for p in bonds:
                rl, rr = (1 if p == 1 else 3), (1 if p == d - 1 else 4)
                out.append(dict(name=f"small_{'DE'[fid - 2]}{d}_p{p}", d=d, n=5, par=par, p=p, left=_pick(rng, 5, rl, p - 1),
                                right=_pick(rng, 5, rr, d - p - 1), caps=(0, 2, d + 1), points=_pick(rng, 5, 6, d)))
    # decay counts 22, 23, 24, 25 on both sides: c - 1 nodes 0.5 next to the bond, then 2^-40 ends the vector
    nodes, ln = [0.5, 2.0 ** -40, 0.75], 26
    for fid in (2, 3):
        side = [[_from_bond(sd, [1] * (c - 1) + [2], ln, 3 if c % 2 else 1) for c in (22, 23, 24, 25)] for sd in (0, 1)]
        out.append(dict(name=f"reglimit_{'DE'[fid - 2]}54", d=2 * ln + 2, n=3, par=_par(nodes, [1.1, 0.6, 1.7], fid), p=ln + 1,
                        left=np.array(side[0], dtype=np.int32), right=np.array(side[1], dtype=np.int32), caps=(20, 22, 23, 24, 25, 30),
                        points=_pick(rng, 3, 4, 2 * ln + 2), counts=([22, 23, 24, 25], [22, 23, 24, 25]), need_nfar=True))
    # powers of two: every argument exact.  indices: 1 = 1/2, 2 = 2^-6, 3 = 2^-27, 4 = 2^-9, 5 = 2^-26
    nodes = [0.5, 2.0 ** -6, 2.0 ** -27, 2.0 ** -9, 2.0 ** -26]
    left = [[5, 5, 1, 1, 1],      # 1, 2^-26, 2^-52, 2^-53 kept, 2^-54 dropped            -> 4
            [3, 3, 1, 1, 1],      # 1, 2^-27, 2^-54 = 2^-27 * 2^-27 dropped               -> 2
            [2, 2, 2, 2, 2],      # 2^-30 at the end                                      -> 6
            [3, 4, 4, 4, 4]]      # 1, 2^-27, 2^-36, 2^-45, 2^-54 dropped                 -> 4
    right = [[3, 3, 1, 1, 1],     #                                                       -> 2
             [3, 5, 1, 1, 1],     # 1, 2^-27, 2^-53 kept, 2^-54 dropped                   -> 3
             [1, 1, 1, 1, 1],     #                                                       -> 6
             [4, 4, 4, 4, 4]]     # 2^-45 at the end                                      -> 6
    for fid in (2, 3):
        out.append(dict(name=f"pow2_{'DE'[fid - 2]}12", d=12, n=5, par=_par(nodes, w5, fid), p=6,
                        left=np.array([_from_bond(0, s, 5, 1) for s in left], dtype=np.int32),
                        right=np.array([_from_bond(1, s, 5, 1) for s in right], dtype=np.int32), caps=(0, 3, 13),
                        points=_pick(rng, 5, 6, 12), counts=([4, 2, 6, 4], [2, 3, 6, 6])))
    # nine dims 2^-6: near[9] = 2^-54 is dropped, near[8] = 2^-48 kept
    out.append(dict(name="pow2_D13", d=13, n=5, par=_par(nodes, w5, 2), p=11, left=np.array([[2] * 10, [1] * 10], dtype=np.int32),
                    right=np.array([[2], [3]], dtype=np.int32), caps=(0, 9, 10, 14), points=_pick(rng, 5, 4, 13), counts=([9, 11], [2, 2])))
    # nodes exactly 0 and exactly 1
    for fid in (2, 3):
        out.append(dict(name=f"zero_one_{'DE'[fid - 2]}6", d=6, n=4, par=_par([0.0, 1.0, 0.5, 0.3], [1.0, 0.8, 1.5, 0.6], fid), p=3,
                        left=np.array([[3, 4], [1, 3], [2, 4], [4, 4]], dtype=np.int32), right=np.array([[3, 3], [4, 1], [3, 2], [4, 3]], dtype=np.int32),
                        caps=(0, 2, 7), points=np.array([[3, 4, 3, 4, 3, 4], [1, 3, 3, 3, 3, 3], [3, 3, 2, 3, 3, 3], [1, 2, 3, 4, 3, 3], [4, 4, 4, 4, 4, 4]],
                                                        dtype=np.int32), zeros=True))
    # d = 70: decay counts above 64 (0.6: 68 of 67 dims, 9/16: 66), mixed with small nodes so that counts differ inside a block
    nodes, wts = [0.6, 9.0 / 16.0, 2.0 ** -6, 0.05], [1.2, 0.9, 1.6, 0.7]
    # third pivot: 0.6^30 2^-6 (9/16)^t > 2^-54 for t <= 31: 1 + 30 + 1 + 31 = 63 entries
    lng = [[1] * 67, [2] * 67, [1] * 30 + [3] + [2] * 36]
    for fid, p in ((2, 68), (3, 2)):
        sd = 0 if p == 68 else 1
        long_ = np.array([_from_bond(sd, s, 67, 1) for s in lng], dtype=np.int32)
        short = np.array([[1], [2], [4]], dtype=np.int32)
        out.append(dict(name=f"long_{'DE'[fid - 2]}70_p{p}", d=70, n=4, par=_par(nodes, wts, fid), p=p, left=long_ if sd == 0 else short,
                        right=short if sd == 0 else long_, caps=(40, 71), points=np.array([[1] * 70, [2] * 70, [1] * 35 + [4] + [2] * 34], dtype=np.int32),
                        counts=([68, 66, 63], [2, 2, 2]) if sd == 0 else ([2, 2, 2], [68, 66, 63]), need_nfar=True))
    return out


def mvn_cases():
    out = []
    rng = np.random.default_rng(20240608)
    for d, r, n in ((4, 3, 5), (12, 3, 5), (70, 2, 3)):
        off = np.array([-0.5, -0.2, 0.1, 0.35, 0.6])[:n]
        for p in (1, d // 2, d - 1):
            out.append(dict(name=f"mvn{d}_p{p}", d=d, n=n, off=off, p=p, left=_pick(rng, n, 1 if p == 1 else r, p - 1),
                            right=_pick(rng, n, 1 if p == d - 1 else r, d - p - 1), points=_pick(rng, n, 4, d)))
    # the drivers' distribution treats every dimension alike (equal means, equal diagonal): a wrong dimension index would not show.
    # The same cases once more with every dimension rescaled differently and an antisymmetric part added (mvn_aux)
    for c in [c for c in out if c["d"] in (4, 12)]:
        out.append(dict(c, name=c["name"] + "_skew", skew=True))
    return out


def mvn_aux(c, base):
    """aux of a case from the drivers' aux (mu, inverse covariance column-major, det).  skew: dimension i is rescaled by s_i =
    1 + i/(4d) (C -> diag(s) C diag(s), det -> det / prod s^2), its mean moved by i/100, and K - K' with K_ab = a b / 16 (a < b) is
    added to C: the quadratic form, and so the density, depends on the symmetric part only."""
    if not c.get("skew"):
        return base
    d = c["d"]
    aux = np.array(base, dtype=np.float64)
    sc = 1.0 + np.arange(d) / (4.0 * d)
    C = aux[d:d + d * d].reshape(d, d, order="F") * np.outer(sc, sc)
    K = np.triu(np.outer(np.arange(d), np.arange(d)) / 16.0, 1)
    aux[d:d + d * d] = (C + K - K.T).ravel(order="F")
    aux[:d] += np.arange(d) / 100.0
    aux[d + d * d] /= float(np.prod(sc) ** 2)
    return aux


def mvn_nodes(c, aux):
    return aux[0] + c["off"]


def block_indices(c):
    """every full multi-index of the case's block, in the order [rL][n][n][rR], as a list of tuples"""
    L, R, n = np.asarray(c["left"]), np.asarray(c["right"]), c["n"]
    return [tuple(L[i]) + (j, k) + tuple(R[q]) for i in range(L.shape[0]) for j in range(1, n + 1) for k in range(1, n + 1) for q in range(R.shape[0])]
