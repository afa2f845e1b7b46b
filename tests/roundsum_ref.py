"""Reference for ttx_lincomb_round, numpy float64 only (test side).  Cores have shape (r_(k-1), n_k, r_k).

The definition (include/ttx.h restates it; modes k = 1 .. d, S(k) = sum_t r_t(k)):
  1. l(0) = l(d) = 1, l(k) = min(L, S(k), prod_(j<=k) n_j, prod_(j>k) n_j), a product no longer multiplied once it is above 128;
     then left to right l(k) <= l(k-1) n_k, then right to left l(k-1) <= n_k l(k)                                   (sketch_ranks)
  2. Omega_k (l(k-1), n_k, l(k)) from the integer recipe, engine.roundsum_omega                                       (omegas)
  3. W_t(d) = [1], W_t(k-1) = sum_i X_(t,k)(:, i, :) W_t(k) Omega_k(:, i, :)^T; the stack of all terms times 2^-e after each step,
     (f, e) = frexp(max |W|)
  4. Y_t(1) = c_t X_(t,1); for k = 1 .. d-1: Z = Y(k) W(k), Z = Q R, new core k = Q, M = Q^T Y(k), Y_t(k+1) = M_t x_1 X_(t,k+1);
     new core d = sum_t Y_t(d) in term order
roundsum() is the restatement (QR by LAPACK, terms in order); roundsum_mgs() evaluates the same definition independently: QR by
modified Gram-Schmidt applied twice, the terms summed in the opposite order, Z as a sum of per-term products.

The allowances (derived, not measured; u = 2^-53, gamma_N written as N u as in algebra_ref.py; B = sum_t |c_t| |x_t|_F, the scale
of the numbers that enter: projections do not increase it).  The device and the reference compute the same projection of the same
sum, T = Q_1 Q_1^T ... applied to the unfoldings of sum_t c_t x_t; they differ by their roundings.  Relative to B, first order:
  w(k)   the stacked W(k): every step from d down to k + 1 is two sums of lengths r^(j) = max_t r_t(j) and l(j), summed over the
         n_j indices; the power of two is exact:                                 w(k) = sum_(j>k) (r^(j) + l(j) + n_j)
  y(k)   Y(k): y(1) = 1, the multiply by c_t; a step adds M = Q^T Y, sums of length l(k-1) n_k, and the advance, sums of length
         r^(k):                                                                   y(k+1) = y(k) + l(k-1) n_k + r^(k)
  z(k)   Z_k = Y(k) W(k), sums of length S(k), and its Householder QR, (l(k-1) n_k) l(k) (Higham, Accuracy and Stability, Thm 19.4,
         the constant taken as 1):                                                z(k) = y(k) + w(k) + S(k) + l(k-1) n_k l(k)
A relative change eps of Z_k turns its range, and with it Q_k Q_k^T, by at most cond(Z_k) eps; what passes through the projector
changes by that much of B.  The last core adds y(d) + m without a projector.  Each evaluation therefore lies within
(sum_k z(k) + y(d) + m) u max_k cond(Z_k) B of the exact projection, and two evaluations differ as tensors (Frobenius norm) by
    allowance = c(d, n, l) u max_k cond(Z_k) B,        c(d, n, l) = 2 (sum_(k<d) z(k) + y(d) + m),
cond(Z_k) taken from roundsum()'s own Z_k.  Where l(k) reaches the rank of the sum's unfolding at every bond (the exact-rank
cases), the range of Z_k is the range of that unfolding whatever the sketch is: the projector does not act, both sides equal the
dense sum in exact arithmetic, and they differ from it by the same expression without the condition number,
    allowance_exact = c(d, n, l) u B.
None of this is tuned on the device: test_roundsum_cpu.py holds the two evaluations here against a quarter of it."""
import numpy as np

from ttcross_amd import engine as E

U = 2.0 ** -53


def _f64(cores):
    return [np.asarray(c, dtype=np.float64) for c in cores]


def ranks(cores):
    return [cores[0].shape[0]] + [c.shape[2] for c in cores]


def sketch_ranks(n, S, L):
    """step 1; n: mode sizes, S[k]: rank sums at the bonds 0 .. d (S[0], S[d] unused)"""
    d = len(n)
    pl, pr = [1] * (d + 1), [1] * (d + 1)
    for k in range(1, d + 1):
        pl[k] = pl[k - 1] if pl[k - 1] > 128 else pl[k - 1] * int(n[k - 1])
    for k in range(d - 1, -1, -1):
        pr[k] = pr[k + 1] if pr[k + 1] > 128 else pr[k + 1] * int(n[k])
    l = [1] * (d + 1)
    for k in range(1, d):
        l[k] = min(int(L), int(S[k]), pl[k], pr[k])
    for k in range(1, d):
        l[k] = min(l[k], l[k - 1] * int(n[k - 1]))
    for k in range(d - 1, 0, -1):
        l[k] = min(l[k], int(n[k]) * l[k + 1])
    return l


def rank_sums(trains):
    d = len(trains[0])
    return [len(trains)] + [sum(ranks(x)[k] for x in trains) for k in range(1, d)] + [len(trains)]


def omegas(seed, n, l):
    return [E.roundsum_omega(seed, k + 1, (l[k], n[k], l[k + 1])) for k in range(len(n))]


def _mat(y):
    """(l0, n, r) -> the matrix of l0 n rows (row a + l0 i)"""
    return y.reshape((y.shape[0] * y.shape[1], y.shape[2]), order="F")


def _sketch_pass(trains, om, scale, reverse=False):
    """step 3: W[k][t] = W_t(k) for k = 1 .. d (W[0] unused)"""
    d, m = len(trains[0]), len(trains)
    W = [None] * (d + 1)
    W[d] = [np.ones((1, 1)) for _ in range(m)]
    for k in range(d, 1, -1):
        if reverse:                 # the other association: X with Omega first, then W
            cur = [np.einsum("aib,bpi->ap", x[k - 1], np.einsum("bq,piq->bpi", w, om[k - 1])) for x, w in zip(trains, W[k])]
        else:
            cur = [np.einsum("aiq,piq->ap", np.einsum("aib,bq->aiq", x[k - 1], w), om[k - 1]) for x, w in zip(trains, W[k])]
        if scale:
            mx = max(float(np.max(np.abs(w))) for w in cur)
            e = int(np.frexp(mx)[1]) if (mx > 0.0 and np.isfinite(mx)) else 0
            cur = [np.ldexp(w, -e) for w in cur]
        W[k - 1] = cur
    return W


def _mgs2(z):
    """Q of a QR by modified Gram-Schmidt applied twice.  A column of which the projections leave no more than rows x columns x u
    of its norm (the QR count of the docstring) is dependent to working accuracy and stays ZERO: Q Q^T is then the projector on
    the other columns, which span the range of Z as well as rounding lets anything span it.  (Householder QR fills such columns
    with directions made of rounding noise instead; on a Z of full column rank the two give the same projector.)"""
    q = np.array(z, dtype=np.float64)
    thr = q.shape[0] * q.shape[1] * U
    for _ in range(2):
        for j in range(q.shape[1]):
            before = float(np.sqrt(q[:, j] @ q[:, j]))
            for i in range(j):
                q[:, j] = q[:, j] - (q[:, i] @ q[:, j]) * q[:, i]
            nrm = float(np.sqrt(q[:, j] @ q[:, j]))
            q[:, j] = q[:, j] / nrm if nrm > thr * before else 0.0
    return q


def _round(coefs, trains, L, seed, scale, other, w_edit=None):
    trains = [_f64(x) for x in trains]
    d, m = len(trains[0]), len(trains)
    n = [c.shape[1] for c in trains[0]]
    l = sketch_ranks(n, rank_sums(trains), L if L else 128)
    om = omegas(seed, n, l)
    with np.errstate(over="ignore", invalid="ignore"):
        W = _sketch_pass(trains, om, scale, reverse=other)
        if w_edit is not None:
            W = [None if ws is None else [w_edit(w) for w in ws] for ws in W]
        Y = [np.float64(c) * x[0] for c, x in zip(coefs, trains)]
        cores, Zs = [], []
        order = range(m - 1, -1, -1) if other else range(m)
        for k in range(1, d):
            Ym = [_mat(y) for y in Y]
            if other:
                Z = np.zeros((Ym[0].shape[0], l[k]))
                for t in order:
                    Z = Z + Ym[t] @ W[k][t]
                Q = _mgs2(Z)
            else:
                Z = np.hstack(Ym) @ np.vstack(W[k])
                Q = np.linalg.qr(Z)[0]
            Zs.append(Z)
            cores.append(Q.reshape((l[k - 1], n[k - 1], l[k]), order="F"))
            Y = [np.einsum("pb,bic->pic", Q.T @ ym, x[k]) for ym, x in zip(Ym, trains)]
        last = np.zeros_like(Y[0])
        for t in order:
            last = last + Y[t]
        cores.append(last)
    return dict(cores=cores, Z=Zs, l=l, W=W)


def roundsum(coefs, trains, L, seed, scale=True, w_edit=None):
    """the restatement: dict(cores, Z (the Z_k, k = 1 .. d-1), l, W).  w_edit: a function applied to every W_t(k) before the second
    pass -- for tests that ask what a wrong sketch would do to the result"""
    return _round(coefs, trains, L, seed, scale, False, w_edit)


def roundsum_mgs(coefs, trains, L, seed):
    """the independent evaluation of the same definition"""
    return _round(coefs, trains, L, seed, True, True)


def dense(cores):
    t = _f64(cores)[0]
    for c in _f64(cores)[1:]:
        t = np.tensordot(t, c, axes=([t.ndim - 1], [0]))
    return t.reshape(t.shape[1:-1])


def dense_sum(coefs, trains):
    s = 0.0
    for c, x in zip(coefs, trains):
        s = s + np.float64(c) * dense(x)
    return s


def tt_svd(T, l):
    """the deterministic TT-SVD of a dense tensor at the given ranks l(0 .. d) (left to right, LAPACK SVD): cores"""
    n, d = T.shape, T.ndim
    cores, rest, r0 = [], np.asarray(T, dtype=np.float64).reshape((n[0], -1), order="F"), 1
    for k in range(d - 1):
        u, s, vt = np.linalg.svd(rest.reshape((r0 * n[k], -1), order="F"), full_matrices=False)
        r1 = min(int(l[k + 1]), s.size)
        cores.append(u[:, :r1].reshape((r0, n[k], r1), order="F"))
        rest, r0 = s[:r1, None] * vt[:r1], r1
    cores.append(rest.reshape((r0, n[d - 1], 1), order="F"))
    return cores


def scale_b(coefs, trains):
    """B = sum_t |c_t| |x_t|_F"""
    return float(sum(abs(float(c)) * np.linalg.norm(dense(x)) for c, x in zip(coefs, trains)))


def c_count(trains, l):
    """c(d, n, l) of the docstring"""
    d, m = len(trains[0]), len(trains)
    n = [c.shape[1] for c in trains[0]]
    S = rank_sums(trains)
    rh = [max(ranks(x)[k] for x in trains) for k in range(d + 1)]
    w = [0] * (d + 1)
    for k in range(d - 1, 0, -1):
        w[k] = w[k + 1] + rh[k + 1] + l[k + 1] + n[k]
    y = [0] * (d + 1)
    y[1] = 1
    for k in range(1, d):
        y[k + 1] = y[k] + l[k - 1] * n[k - 1] + rh[k]
    z = sum(y[k] + w[k] + S[k] + l[k - 1] * n[k - 1] * l[k] for k in range(1, d))
    return 2 * (z + y[d] + m)


def cond_max(ref):
    with np.errstate(divide="ignore", invalid="ignore"):
        return max(float(np.linalg.cond(z)) for z in ref["Z"])


def allowance(coefs, trains, ref, exact_rank):
    """the Frobenius-norm allowance of the docstring for this call; ref = roundsum(...)"""
    a = c_count([_f64(x) for x in trains], ref["l"]) * U * scale_b(coefs, trains)
    return a if exact_rank else a * cond_max(ref)


# ---- the cases, shared by test_roundsum_cpu.py and test_gpu_roundsum.py ---------------------------------------------------------
def rand_train(seed, n, r, lo=-1.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return [rng.uniform(lo, hi, (r[k], n[k], r[k + 1])) for k in range(len(n))]


def _chain(d, r):
    return [1] + [r] * (d - 1) + [1]


def lincomb_cores(coefs, trains):
    """the block assembly of ttx_lincomb (algebra_ref.lincomb_cores), kept here so that this module stands alone"""
    d = len(trains[0])
    rr = [1] + rank_sums(trains)[1:d] + [1]
    out = []
    for k in range(d):
        z = np.zeros((rr[k], trains[0][k].shape[1], rr[k + 1]))
        ro = co = 0
        for c, x in zip(coefs, trains):
            g = x[k]
            z[ro:ro + g.shape[0], :, co:co + g.shape[2]] = np.float64(c) * g if k == 0 else g
            ro += g.shape[0] if k > 0 else 0
            co += g.shape[2] if k < d - 1 else 0
        out.append(z)
    return out


def case_fails_today():
    """12 terms, d = 6, n = 4, each a lincomb of the same three rank-4 base trains: formal rank 12 each, 144 in all, true rank 12"""
    n = [4] * 6
    base = [rand_train(100 + b, n, _chain(6, 4)) for b in range(3)]
    rng = np.random.default_rng(7)
    terms = [lincomb_cores(rng.uniform(-1.0, 1.0, 3), base) for _ in range(12)]
    coefs = rng.uniform(-2.0, 2.0, 12)
    return coefs, terms


EDGE_N = [7, 3, 7, 1, 7, 2, 7]      # d = 7, n from {1, 2, 3, 7}, a mode of size 1 in the middle; 14406 elements
# bond limits of these modes: products from the left 7, 21, 147, ..., from the right ..., 98, 98, 14, 7
# r1, r3, r5, r5b: random trains of those ranks.  r17 and r63, r63b: FORMAL ranks 17 and 63 at every bond, block assemblies
# (lincomb_cores) of r1, r3, r5 / r5b taken several times, so that their true ranks stay <= 14: a sum that reaches l(k) = 89 or 98 with
# true rank 89 would have a SQUARE sketch at those bonds, whose smallest singular value -- not the arithmetic -- sets the error
# (numpy: 5e-6 on a sum of norm 3e4), and no allowance without a condition number holds for it.
EDGE_BLOCKS = {"r17": ["r5", "r5", "r3", "r3", "r1"], "r63": ["r5"] * 12 + ["r3"], "r63b": ["r5b"] * 6 + ["r5"] * 6 + ["r3"]}
# Trains whose sum has TRUE rank 98 at the middle bond (two random trains of rank 49 there; the modes allow 147 on either side), for
# the cases below that truncate it at l = 17, 40 and 72: the sketch and the new cores span two, three and five tiles of 16 columns,
# and what every tile holds decides the result (the exact-rank cases above are blind to the columns beyond the sum's rank).
MULTI_N = [7, 3, 7, 7, 3, 7]        # 21609 elements; bond limits 7, 21, 147, 21, 7
MULTI_R = {"m49a": [1, 7, 21, 49, 21, 7, 1], "m49b": [1, 7, 21, 49, 21, 7, 1]}
MULTI_SEED = 0
_edge_cache = {}


def edge_train(name):
    if name not in _edge_cache:
        if name in EDGE_BLOCKS:
            rng = np.random.default_rng(sum(map(ord, name)))
            parts = EDGE_BLOCKS[name]
            _edge_cache[name] = lincomb_cores(rng.uniform(0.5, 1.5, len(parts)) * rng.choice([-1.0, 1.0], len(parts)), [edge_train(p) for p in parts])
        elif name in MULTI_R:
            _edge_cache[name] = rand_train(sum(map(ord, name)) + MULTI_SEED, MULTI_N, MULTI_R[name])
        else:
            _edge_cache[name] = rand_train(sum(map(ord, name)), EDGE_N, _chain(7, int(name[1])))
    return _edge_cache[name]


# name -> (coefs, names of the trains, rank, exact_rank); a name that appears twice is the same engine on the device.
# exact_rank: l(k) reaches the rank of the sum's unfolding at every bond (L does not bind, or the sum has low rank by construction)
EDGE = {
    "ranks_1_3_5_17_63_rank_128": ([1.0, -0.5, 2.0, 0.25, -1.5], ["r1", "r3", "r5", "r17", "r63"], 128, True),      # l = 1 7 21 89 89 14 7 1
    "rank_sum_143_rank_0_is_128": ([1.0, 0.5, -1.0], ["r63", "r63b", "r17"], 0, True),                             # l(3) = l(4) = 98, the modes' limit
    "ranks_1_3_5_17_63_rank_17": ([1.0, -0.5, 2.0, 0.25, -1.5], ["r1", "r3", "r5", "r17", "r63"], 17, True),                        # true rank <= 9
    "rank_7": ([1.0, 2.0, -1.0], ["r5", "r17", "r3"], 7, False),
    "rank_1": ([1.0, 2.0], ["r3", "r5"], 1, False),
    "one_term_rank_at_least_r": ([-2.5], ["r17"], 17, True),
    "sum_r_below_rank": ([1.0, 1.0], ["r1", "r3"], 7, True),
    "same_engine_repeated": ([0.5, 3.0, -0.25], ["r3", "r5", "r3"], 17, True),
    "x_minus_x_plus_y": ([1.0, -1.0, 1.0], ["r5", "r5", "r3"], 17, True),                                            # l = 13 against rank 3: Z is rank deficient
    "coefficients_zero": ([0.0, 1.0, 0.0], ["r5", "r3", "r17"], 7, True),
    "true_rank_98_rank_17": ([1.0, -0.75], ["m49a", "m49b"], 17, False),                                               # l = 1 7 17 17 17 7 1
    "true_rank_98_rank_40": ([1.0, -0.75], ["m49a", "m49b"], 40, False),                                               # l = 1 7 21 40 21 7 1
    "true_rank_98_rank_72": ([1.0, -0.75], ["m49a", "m49b"], 72, False),                                               # l = 1 7 21 72 21 7 1
}
MULTI_TILE = ("true_rank_98_rank_17", "true_rank_98_rank_40", "true_rank_98_rank_72")
D2_N = [5, 7]
D2 = ([1.5, -0.75], [[1, 3, 1], [1, 4, 1]], 7, True)                                                                 # d = 2: l(1) = 5, the first mode's size


def d2_trains():
    return [rand_train(21 + t, D2_N, r) for t, r in enumerate(D2[1])]


def decay_terms(seed, m=20, d=6, nk=4):
    """m rank-2 terms of weights 2^-j"""
    n = [nk] * d
    return [2.0 ** -j for j in range(m)], [rand_train(1000 * seed + j, n, _chain(d, 2)) for j in range(m)]


DECAY_SEED = 2
DECAY_RANKS = (4, 8, 12)
SKETCH_SEED = 7                     # with DECAY_SEED: cond(Z) 53 / 94 / 440 at L = 4 / 8 / 12, the reference within 3 x TT-SVD (conditions on the inputs)


def long_train(d=255):
    """two rank-4 terms with entries of size 8 (8 x uniform(-0.6, 0.6)), n = 4: finite as a tensor, not as an unscaled W chain"""
    n = [4] * d
    return [1.0, -0.5], [rand_train(900 + t, n, _chain(d, 4), -4.8, 4.8) for t in range(2)]
