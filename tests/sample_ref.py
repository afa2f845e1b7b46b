"""Reference for ttx_sample (include/ttx.h), numpy float64 only (test side).

draw(cores, u, w, fixed) restates the definition with plain sequential sums: prefix vectors from the effective weights, head
tables H_k(i, b) = w_k(i) sum_a l_(k-1)(a) G_k(a, i, b), modes drawn from the last to the first, p = |H_k x|, c the sequential
running sum, t = u c(n), the smallest i with p(i) > 0 and t < c(i) (else the largest i with p > 0), x <- G_k(:, i_k, :) x.

verify(cores, u, w, fixed, ind_dev) walks every sample along the DEVICE's indices, so that a difference at one mode cannot cascade
into the modes after it, and decides per mode whether the device had a choice.

The bound.  c_k(i) is a sum over j <= i of |sum_b H_k(j, b) x(b)|.  One term of that double sum is a product
l-chain . G_k . x-chain . w_k(j) and reaches the result through
  * the prefix chain l_(k-1) = M_1 .. M_(k-1): per bond one multiply, the inner sum over r_k terms and the weight's multiply,
    at most r_k + 2 roundings, summed over the bonds: sum_k (r_k + 2);
  * the state chain x_(k+1) = G_(k+1) .. G_d: per bond one multiply and r_k additions, again at most sum_k (r_k + 2);
  * the running sum over i, at most max n_k additions in any association order;
  * four single operations: the weight w_k(j) in H, the product with x's entry, t = u c(n) and the slack of the comparison.
That is N = 2 sum_(k=0..d) (r_k + 2) + max n_k + 4 roundings along the chain, and for every order of the sums
|computed - true| <= N 2^-53 B with B the same quantity on |cores|, |w| and |state| (the argument of test_gpu_contract.py's
docstring); device against reference is 2 N u B on each of the two numbers compared, t and an edge c(i): 4 N u Bc(n_k).
What N does NOT count: inside M_j the sum over the n_j indices of a prefix mode adds up to n_j roundings per prefix mode when it
is done sequentially (the device keeps four partial sums there).  On the long modes of these tests that is of the order of N
itself; a mode is therefore declared decided a little too readily, which can only make verify stricter, never more lenient.

A mode is DECIDED when t is further than 4 N u Bc(n_k) from both edges c(i_ref - 1) and c(i_ref) of the reference's own choice;
an edge beyond which no index with p > 0 lies cannot be crossed and counts as far.  On a decided mode the device's index must be
the reference's; on an undecided one it may also be the neighbouring index with p > 0 on the near side."""
import numpy as np

U = 2.0 ** -53


def _prep(cores, w, fixed):
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    d = len(cores)
    w = [np.ones(c.shape[1]) for c in cores] if w is None else [np.asarray(q, dtype=np.float64).ravel() for q in w]
    fixed = [0] * d if fixed is None else [int(f) for f in fixed]
    return cores, w, fixed


def ranks(cores):
    return [cores[0].shape[0]] + [c.shape[2] for c in cores]


def count(cores):
    """N of the bound"""
    return 2 * sum(rk + 2 for rk in ranks(cores)) + max(c.shape[1] for c in cores) + 4


def heads(cores, w, fixed):
    """H_k as (n_k, r_k) arrays (None for a fixed mode), every sum sequential and ascending from 0.0"""
    lv, out = np.ones(1), []
    for c, q, f in zip(cores, w, fixed):
        r0, n, r1 = c.shape
        e = q if not f else np.eye(n)[f - 1]
        if f:
            out.append(None)
        else:
            s = np.zeros((n, r1))
            for a in range(r0):
                s = s + lv[a] * c[a]
            out.append(q[:, None] * s)
        m = np.zeros((r0, r1))
        for i in range(n):
            m = m + e[i] * c[:, i, :]
        nl = np.zeros(r1)
        for a in range(r0):
            nl = nl + lv[a] * m[a]
        lv = nl
    return out


def _p_rows(Hk, x):
    """p[s, i] = |sum_b H_k(i, b) x[s, b]|, ascending b from 0.0"""
    m = np.zeros((x.shape[0], Hk.shape[0]))
    for b in range(Hk.shape[1]):
        m = m + Hk[None, :, b] * x[:, b:b + 1]
    return np.abs(m)


def _step(c, idx0, x):
    """x_new[s, a] = sum_b G(a, idx0[s], b) x[s, b], ascending b from 0.0"""
    z = np.zeros((x.shape[0], c.shape[0]))
    for b in range(c.shape[2]):
        z = z + c[:, idx0, b].T * x[:, b:b + 1]
    return z


def _choose(p, c, t, u):
    """per row: the smallest i with p > 0 and t < c(i); none, or u >= 1: the largest i with p > 0 (-1: no p > 0)"""
    n = p.shape[1]
    pos = p > 0
    hit = pos & (t[:, None] < c) & (u[:, None] < 1.0)
    first = np.where(hit.any(1), hit.argmax(1), -1)
    last = np.where(pos.any(1), n - 1 - pos[:, ::-1].argmax(1), -1)
    return np.where(first >= 0, first, last)


def draw(cores, u, w=None, fixed=None):
    """(ind [npts][d] int32 1-based, logq, val, failed mask) by the definition"""
    cores, w, fixed = _prep(cores, w, fixed)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    npts, d = u.shape
    H = heads(cores, w, fixed)
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
                p = _p_rows(H[k], x)
                c = np.cumsum(p, axis=1)
                tot = c[:, -1]
                i0 = _choose(p, c, u[:, k] * tot, u[:, k])
                failed |= ~(tot > 0.0) | np.isinf(tot) | (i0 < 0)
                i0 = np.where(failed, 0, i0)
                logq = logq + np.log(p[np.arange(npts), i0] / tot)
            ind[:, k] = i0 + 1
            x = _step(cores[k], i0, x)
    ind[failed] = 0
    return ind, np.where(failed, np.nan, logq), np.where(failed, 0.0, x[:, 0]), failed


def verify(cores, u, w, fixed, ind_dev):
    """Walk the samples along ind_dev (module docstring).  Raises AssertionError on an index the definition does not allow;
    returns dict(undecided = samples with an undecided mode, logq = the reference's logq along the device's indices,
    maxlog = max |log term| per sample, N)."""
    cores, w, fixed = _prep(cores, w, fixed)
    u = np.atleast_2d(np.asarray(u, dtype=np.float64))
    ind_dev = np.asarray(ind_dev)
    npts, d = u.shape
    N = count(cores)
    H = heads(cores, w, fixed)
    HB = heads([np.abs(c) for c in cores], [np.abs(q) for q in w], fixed)
    ref_failed = draw(cores, u, w, fixed)[3]
    dev_failed = np.all(ind_dev == 0, axis=1)
    assert np.array_equal(dev_failed, ref_failed), ("failed samples differ", np.flatnonzero(dev_failed != ref_failed)[:10])
    ok = ~dev_failed
    assert np.all((ind_dev[ok] >= 1) & (ind_dev[ok] <= np.array([c.shape[1] for c in cores])[None, :]))
    idx = np.where(ok[:, None], ind_dev - 1, 0)
    x, xb = np.ones((npts, 1)), np.ones((npts, 1))
    undecided = np.zeros(npts, bool)
    logq, maxlog = np.zeros(npts), np.zeros(npts)
    rows = np.arange(npts)
    for k in range(d - 1, -1, -1):
        i_dev = idx[:, k]
        if fixed[k]:
            assert np.all(ind_dev[ok, k] == fixed[k]), f"mode {k + 1} is fixed at {fixed[k]}"
        else:
            with np.errstate(all="ignore"):
                p = _p_rows(H[k], x)
                c = np.cumsum(p, axis=1)
                t = u[:, k] * c[:, -1]
                tol = 4.0 * N * U * np.cumsum(_p_rows(HB[k], xb), axis=1)[:, -1]
                i_ref = np.maximum(_choose(p, c, t, u[:, k]), 0)
            pos = p > 0
            below = np.cumsum(pos, axis=1) - pos                     # indices with p > 0 below i
            above = pos.sum(1)[:, None] - below - pos
            c_lo = np.where(i_ref > 0, c[rows, np.maximum(i_ref - 1, 0)], 0.0)
            c_hi = c[rows, i_ref]
            near_lo = (np.abs(t - c_lo) <= tol) & (below[rows, i_ref] > 0)
            near_hi = (np.abs(t - c_hi) <= tol) & (above[rows, i_ref] > 0) & (u[:, k] < 1.0)
            # the neighbour with p > 0 on either side of the reference's choice
            nb_lo = np.array([np.flatnonzero(pos[s, :i_ref[s]])[-1] if below[s, i_ref[s]] > 0 else -1 for s in range(npts)])
            nb_hi = np.array([i_ref[s] + 1 + np.flatnonzero(pos[s, i_ref[s] + 1:])[0] if above[s, i_ref[s]] > 0 else -1 for s in range(npts)])
            good = (i_dev == i_ref) | (near_lo & (i_dev == nb_lo)) | (near_hi & (i_dev == nb_hi))
            bad = ok & ~good
            assert not bad.any(), (f"mode {k + 1}: {int(bad.sum())} samples off", [(int(s), int(i_dev[s]), int(i_ref[s]), float(t[s]), float(c_lo[s]), float(c_hi[s]), float(tol[s])) for s in np.flatnonzero(bad)[:5]])
            assert np.all(pos[rows, i_dev][ok]), f"mode {k + 1}: an index with p = 0 was drawn"
            undecided |= ok & (near_lo | near_hi)
            with np.errstate(all="ignore"):
                term = np.where(ok, np.log(p[rows, i_dev] / c[:, -1]), 0.0)
            logq = logq + term
            maxlog = np.maximum(maxlog, np.abs(term))
        x = _step(cores[k], i_dev, x)
        xb = _step(np.abs(cores[k]), i_dev, xb)
    return dict(undecided=int(undecided.sum()), logq=np.where(ok, logq, np.nan), maxlog=maxlog, N=N)


def dense(cores):
    """the full tensor of a small train"""
    t = np.asarray(cores[0], dtype=np.float64)
    for c in cores[1:]:
        t = np.tensordot(t, c, axes=([t.ndim - 1], [0]))
    return t[0, ..., 0]


def dense_density(cores, w=None, fixed=None):
    """|T(i)| w(i) / Z over the drawn modes with the fixed ones held (fixed modes keep a singleton axis); weights of fixed modes do not enter"""
    cores, w, fixed = _prep(cores, w, fixed)
    t = np.abs(dense(cores))
    for k, (q, f) in enumerate(zip(w, fixed)):
        sh = [1] * len(cores)
        if f:
            t = np.take(t, [f - 1], axis=k)
        else:
            sh[k] = q.size
            t = t * np.abs(q).reshape(sh)
    return t / t.sum()


# the (cores, u) pairs of tests/test_gpu_sample.py, shared with the CPU test that checks the cap on the reference alone
NPTS = 2000
CASES = {
    "d2": ([5, 3], [1, 2, 1]),
    "d3": ([5, 7, 4], [1, 3, 2, 1]),
    "d6_size1_rank1": ([4, 1, 6, 1, 5, 3], [1, 3, 5, 1, 4, 2, 1]),
    "d8_unequal": ([3, 5, 2, 7, 4, 6, 3, 5], [1, 3, 17, 64, 65, 9, 128, 2, 1]),
    "long_modes": ([65, 130, 64], [1, 4, 3, 1]),
    "above_lds_cap": ([4, 1025, 3], [1, 3, 2, 1]),               # TTX_SM_LDSROW = 1024: the row of p of mode 2 lies in global memory
}
SIGNED = ("d3", "d8_unequal")


def case(name, signed=False):
    """(cores, u, w) of a test case: seeded, cores uniform(0.1, 1) and positive weights, or standard normal cores and weights"""
    n, r = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + (1000 if signed else 0))
    if signed:
        cores = [rng.standard_normal((r[k], n[k], r[k + 1])) for k in range(len(n))]
        w = [rng.standard_normal(nk) for nk in n]
    else:
        cores = [rng.uniform(0.1, 1.0, (r[k], n[k], r[k + 1])) for k in range(len(n))]
        w = [rng.uniform(0.5, 1.5, nk) for nk in n]
    return cores, rng.random((NPTS, len(n))), w
