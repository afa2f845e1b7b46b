"""Batched element evaluation on the device: ttx_ijk_batch / ttx_ijk_batch_dev / ttx_value_batch (ttcross_amd/csrc/ttx_eval.h).

The checker is the oracle's dtt_ijk (oracle/ttx_oracle_tt.c:ttxo_tt_ijk).  Exact mode must equal it bit for bit at every point.
MFMA mode sums in another order; its bound is derived, not measured: for a chain of d matrix products with inner dimensions
r_k, every summation order obeys |computed - true| <= sum_k (r_k + 1) u B with u = 2^-53 and B the same chain on |cores|
(componentwise bound of a matrix-chain product); applied to both sides that is |mfma - exact| <= 2 sum_{k=0..d} (r_k + 1) 2^-53 B."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle_lib as O
import tt_ref as R
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

NPTS = 2000


def _cores(tt):
    return [tt.core(k) for k in range(1, tt.d + 1)]


def _points(n, seed, npts=NPTS):
    n = np.asarray(n, dtype=np.int64)
    rng = np.random.default_rng(seed)
    ind = (rng.integers(0, 2 ** 31 - 1, (npts, n.size)) % n + 1).astype(np.int32)
    return np.ascontiguousarray(np.vstack([ind, np.ones((1, n.size), np.int32), n[None, :].astype(np.int32)]))


def _oracle(cores, ind):
    ot = O.OracleTT(cores)
    return np.array([ot.ijk(row) for row in ind])


def _bound(cores, ind):
    r = [cores[0].shape[0]] + [c.shape[2] for c in cores]
    return 2.0 * sum(rk + 1 for rk in r) * 2.0 ** -53 * _oracle([np.abs(c) for c in cores], ind)


def _nonneg(seed, n, r):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1])) / (0.5 * r[k + 1]) for k in range(len(n))]


def _chain(d, r):
    return [1] + [r] * (d - 1) + [1]


RANDOM_TRAINS = {
    "d2": ([5, 7], [1, 3, 1]),
    "d5_modes_of_size_1_rank_1_bond": ([4, 1, 6, 1, 5], [1, 3, 5, 1, 4, 1]),
    "d63_r32": ([3] * 63, _chain(63, 32)),
    "r3": ([6] * 7, _chain(7, 3)),
    "r64": ([5] * 6, _chain(6, 64)),
    "r65": ([4] * 5, _chain(5, 65)),
    "r128": ([4] * 4, _chain(4, 128)),
    "r80_81": ([3, 3, 3, 3], [1, 80, 81, 80, 1]),                     # one step below and one above the 64 KB slice image
    "unequal_ranks": ([3, 5, 2, 7, 4, 6, 3, 5], [1, 3, 17, 64, 65, 9, 128, 2, 1]),
}


def _sweep(kind):
    if kind == "ising_c":
        s = D.ising_setup("c", 6, 33)
        return E.TTCross(s["n"], s["fun_id"], s["par"], 12, pivoting=2, accuracy=s["acc"], quad=s["quad"], tru=s["tru"]).run()
    s = D.box_setup("stdnorm", 5, 17)
    return E.TTCross(s["n"], s["fun_id"], s["par"], 6, pivoting=2, accuracy=s["acc"], quad=s["quad"], tru=s["tru"]).run()


def _train(name, tmp_path):
    if name in ("ising_c", "stdnorm"):
        return _sweep(name)
    if name == "after_svd":
        return E.TTCross.from_cores(R.rand_train(11, [5] * 7, _chain(7, 12))).svd(1e-2)
    if name == "from_read":
        p = os.path.join(str(tmp_path), "t.tt")
        E.TTCross.from_cores(R.rand_train(12, [4, 6, 3, 5], [1, 4, 9, 5, 1])).write(p)
        return E.TTCross.read(p)
    n, r = RANDOM_TRAINS[name]
    return E.TTCross.from_cores(R.rand_train(sum(map(ord, name)), n, r))


ALL_TRAINS = ["ising_c", "stdnorm", "after_svd", "from_read"] + sorted(RANDOM_TRAINS)


@pytest.mark.parametrize("name", ALL_TRAINS)
def test_exact_is_the_oracle_bit_for_bit_and_mfma_within_the_derived_bound(name, tmp_path):
    tt = _train(name, tmp_path)
    cores = _cores(tt)
    ind = _points(tt._n, 7)
    want = _oracle(cores, ind)
    got = tt.tijk_batch(ind, "exact")
    assert tt.eval_last_mode == "exact"
    print(name, "exact: points", ind.shape[0], "differing", int((got != want).sum()))
    assert np.array_equal(got, want)                                   # == on float64, every point
    mf = tt.tijk_batch(ind, "mfma")
    assert tt.eval_last_mode == "mfma"
    bnd = _bound(cores, ind)
    with np.errstate(divide="ignore", invalid="ignore"):
        print(name, "mfma: max |mfma - exact| / bound", float(np.nanmax(np.where(bnd > 0, np.abs(mf - got) / bnd, 0.0))))
    assert np.all(np.abs(mf - got) <= bnd)
    auto = tt.tijk_batch(ind)                                          # auto runs one of the two
    assert np.array_equal(auto, got if tt.eval_last_mode == "exact" else mf)


@pytest.mark.parametrize("d,n,r", [(63, 3, 32), (20, 5, 64), (8, 6, 128)])
def test_mfma_sharp_bound_on_non_negative_trains(d, n, r):
    """cores >= 0: B equals the value, the bound is a relative tolerance of about 1e-13 .. 1e-12"""
    cores = _nonneg(d * r, [n] * d, _chain(d, r))
    tt = E.TTCross.from_cores(cores)
    ind = _points(tt._n, 3)
    ex, mf = tt.tijk_batch(ind, "exact"), tt.tijk_batch(ind, "mfma")
    want = _oracle(cores, ind)
    assert np.array_equal(ex, want)
    tol = 2.0 * sum(rk + 1 for rk in _chain(d, r)) * 2.0 ** -53
    print("d", d, "r", r, "relative tolerance", tol, "max relative difference", float(np.max(np.abs(mf - ex) / want)))
    assert np.all(np.abs(mf - ex) <= tol * want)


@pytest.mark.parametrize("mode", ["exact", "mfma"])
def test_a_value_does_not_depend_on_the_batch(mode, monkeypatch):
    n, r = RANDOM_TRAINS["unequal_ranks"]
    cores = R.rand_train(5, n, r)
    tt = E.TTCross.from_cores(cores)
    ind = _points(n, 21)
    base = tt.tijk_batch(ind, mode)
    perm = np.random.default_rng(1).permutation(ind.shape[0])
    assert np.array_equal(tt.tijk_batch(ind[perm], mode), base[perm])
    dup = np.repeat(ind[:300], 3, axis=0)
    assert np.array_equal(tt.tijk_batch(dup, mode), np.repeat(base[:300], 3))
    for k in (1, 63, 64, 65):
        assert np.array_equal(tt.tijk_batch(ind[:k], mode), base[:k])
    assert tt.tijk_batch(np.zeros((0, len(n)), np.int32), mode).shape == (0,)
    monkeypatch.setenv("TTX_IJK_CHUNK", "257")                          # several chunks, the last one short
    assert np.array_equal(tt.tijk_batch(ind, mode), base)
    t2 = E.TTCross.from_cores(cores)
    assert np.array_equal(t2.tijk_batch(ind, mode), base)
    assert np.array_equal(t2.value_batch(np.full((600, 2), 0.3), mode), np.full(600, t2.value_batch(np.full((1, 2), 0.3), mode)[0]))


@pytest.mark.parametrize("mode", ["exact", "mfma"])
def test_invalid_indices_get_minus_three_and_touch_nobody_else(mode):
    n, r = [5, 4, 6, 3, 7], [1, 4, 6, 5, 3, 1]
    tt = E.TTCross.from_cores(R.rand_train(9, n, r))
    ind = _points(n, 4, 500)
    base = tt.tijk_batch(ind, mode)
    bad = ind.copy()
    rows = {}
    for q, (k, v) in enumerate([(0, 0), (0, -2), (0, n[0] + 1), (2, 0), (2, -1), (2, n[2] + 1), (4, 0), (4, -7), (4, n[4] + 1), (1, 2 ** 31 - 1)]):
        rows[17 * q + 3] = (k, v)
        bad[17 * q + 3, k] = v
    got = tt.tijk_batch(bad, mode)
    mask = np.zeros(ind.shape[0], bool)
    mask[list(rows)] = True
    assert np.all(got[mask] == -3.0)
    assert np.array_equal(got[~mask], base[~mask])
    assert np.array_equal(tt.tijk_batch(bad[mask], mode), np.full(mask.sum(), -3.0))      # a batch of invalid points only


def test_argument_errors_and_the_refusal_ttx_ijk_gives():
    L = E.load_library()
    tt = E.TTCross.from_cores(R.rand_train(2, [3, 3, 3], [1, 2, 2, 1]))
    ind = np.ones((4, 3), np.int32)
    out = np.zeros(4)
    x = np.zeros((4, 3))
    nul_i, nul_d = ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_double)()
    EINVAL = 1
    assert L.ttx_ijk_batch(tt._h, 4, nul_i, E._dp(out), 0) == EINVAL
    assert L.ttx_ijk_batch(tt._h, 4, E._ip(ind), nul_d, 0) == EINVAL
    assert L.ttx_ijk_batch(tt._h, -1, E._ip(ind), E._dp(out), 0) == EINVAL
    assert L.ttx_ijk_batch(tt._h, 4, E._ip(ind), E._dp(out), 3) == EINVAL
    assert L.ttx_ijk_batch_dev(tt._h, 4, None, None, 0) == EINVAL
    assert L.ttx_ijk_batch_dev(tt._h, -1, None, None, 0) == EINVAL
    assert L.ttx_value_batch(tt._h, 4, 3, nul_d, E._dp(out), 0) == EINVAL
    assert L.ttx_value_batch(tt._h, 4, 3, E._dp(x), nul_d, 0) == EINVAL
    assert L.ttx_value_batch(tt._h, -1, 3, E._dp(x), E._dp(out), 0) == EINVAL
    assert L.ttx_value_batch(tt._h, 4, 0, E._dp(x), E._dp(out), 0) == EINVAL
    assert L.ttx_ijk_batch(tt._h, 0, nul_i, nul_d, 0) == 0              # npts = 0 succeeds
    assert L.ttx_ijk_batch(tt._h, 4, E._ip(ind), E._dp(out), 2) == 0
    # an engine of a two-process job that has not run: ttx_ijk refuses it in tt_prepare, and whatever code it answers the batch
    # entry points answer -- they go through the same tt_prepare before anything else (a two-process engine that HAS run needs
    # two processes and is refused by the next line of tt_prepare; that line is not reached here)
    s = D.ising_setup("c", 6, 9)
    mp = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"], nproc=2, world_rank=0, world_size=2)
    i5, v = np.ones((1, 5), np.int32), ctypes.c_double()
    want = L.ttx_ijk(mp._h, E._ip(i5), ctypes.byref(v))
    assert want != 0
    assert L.ttx_ijk_batch(mp._h, 1, E._ip(i5), E._dp(out), 0) == want
    assert L.ttx_ijk_batch_dev(mp._h, 1, None, None, 0) == want
    assert L.ttx_value_batch(mp._h, 1, 5, E._dp(np.zeros((1, 5))), E._dp(out), 0) == want


@pytest.mark.parametrize("mode", ["exact", "mfma"])
@pytest.mark.parametrize("n,dd", [([4] * 6, 2), ([3, 5, 2, 7, 4, 6, 3], 3), ([5] * 6, 6), ([6] * 5, 1), ([3, 4, 5], 4)])
def test_value_batch_is_tijk_batch_of_the_digits(n, dd, mode):
    d = len(n)
    r = [1] + [5] * (d - 1) + [1]
    tt = E.TTCross.from_cores(R.rand_train(d * 10 + dd, n, r))
    rng = np.random.default_rng(dd)
    x = rng.uniform(0.0, 1.0, (1500, dd))
    x[0], x[1], x[2] = 0.0, 1.0, 1.25
    x[3:40] = rng.uniform(1.0, 9.0, (37, dd))
    x[40:60, rng.integers(0, dd)] = -rng.uniform(0.0, 2.0, 20)
    x[60] = -0.0
    got = tt.value_batch(x, mode)
    ind, neg = E.value_indices(n, x)
    want = tt.tijk_batch(ind, mode)
    want[neg] = 0.0
    assert neg.sum() >= 20 and np.all(got[neg] == 0.0)
    assert np.array_equal(got, want)
    if d % dd:
        assert np.all(got[~neg] == -3.0)                                # modes left without a digit
    else:
        assert np.all(got[~neg] != -3.0)


@pytest.mark.parametrize("mode", ["exact", "mfma"])
def test_device_pointer_path_equals_the_host_path(mode):
    """torch tensors by data_ptr() through ttx_ijk_batch_dev, in a child process (tijk_dev_worker.py says why)"""
    import json
    import subprocess
    import sys
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tijk_dev_worker.py"), mode],
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert res["is_cuda"] and res["dtype"] == "torch.float64"
    assert res["equal"] and res["invalid"] == -3.0
    assert res["host_calls_unchanged"] and res["empty"] == [0] and res["int64_refused"]
    assert res.get("other_device_refused", True)
    if mode == "exact":
        assert abs(res["single"] - res["first"]) <= 1e-12 * abs(res["first"])


def test_nothing_else_moves():
    tt = _sweep("ising_c")
    s = D.ising_setup("c", 6, 33)
    ind = _points(tt._n, 5)

    def state():
        return tt.ranks().tobytes(), [c.tobytes() for c in _cores(tt)], tt.quad(s["quad"]), tt.norm(), tt.tijk(ind[3])

    before = state()
    for mode in ("exact", "mfma", "auto"):
        tt.tijk_batch(ind, mode)
        tt.value_batch(np.full((10, 5), 0.4), mode)
        assert state() == before
    # ort, then the batch: the pair test_gpu_parity.py checks for ort + tijk, with its tolerance
    cores0 = _cores(tt)
    ot = O.OracleTT(cores0)
    nrm0 = ot.norm()
    ref = np.array([ot.ijk(row) for row in ind])
    tt.ort()
    tol = 1e-11 * nrm0 / np.sqrt(float(np.prod(np.asarray(tt._n, dtype=np.float64)))) + 1e-12 * np.abs(ref)
    for mode in ("exact", "mfma"):
        assert np.all(np.abs(tt.tijk_batch(ind, mode) - ref) <= tol)
    o1 = O.OracleTT(cores0)
    o1.ort()
    assert np.all(np.abs(tt.tijk_batch(ind, "exact") - np.array([o1.ijk(row) for row in ind])) <= tol)


def test_auto_takes_the_exact_kernel_for_small_batches_and_the_mfma_path_for_large_ones():
    """the rule of DESIGN.md 4.5: MFMA where npts (1.25 ps w + 0.286 ns d) >= 23 us d + 3.2 ns w, w = sum r(k-1) r(k); a short
    low-rank train changes over near 75 k points, a long train of rank 64 already below 10 k"""
    n, r = [5, 4, 6, 3, 7], [1, 4, 6, 5, 3, 1]
    tt = E.TTCross.from_cores(R.rand_train(9, n, r))
    ind = _points(n, 4, 90000 - 2)
    small = tt.tijk_batch(ind[:60000])
    assert tt.eval_last_mode == "exact" and np.array_equal(small, tt.tijk_batch(ind[:60000], "exact"))
    large = tt.tijk_batch(ind)
    assert tt.eval_last_mode == "mfma" and np.array_equal(large, tt.tijk_batch(ind, "mfma"))
    n, r = [3] * 40, _chain(40, 64)
    t2 = E.TTCross.from_cores(_nonneg(40, n, r))
    ind = _points(n, 6, 9998)
    t2.tijk_batch(ind[:2000])
    assert t2.eval_last_mode == "exact"
    t2.tijk_batch(ind)
    assert t2.eval_last_mode == "mfma"


def test_fortran_tijk_of_many_indices_equals_its_own_loop():
    """the drop-in tt_lib: tijk(tt, ind(:,:)) (dtt_ijk_many, one ttx_ijk_batch call) against the program's own loop over
    tijk(tt, ind(:,p)), on a host train of rank 3 and after svd; 1e-12 of the element scale, the tolerance
    test_gpu_boundary.py uses for tijk / elem; points with an index outside 1..n(k) give -3 both ways"""
    import subprocess
    from conftest import fortran_exe
    exe = fortran_exe("test_tijk_batch")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("done"), p.stdout[-2000:] + p.stderr[-2000:]
    for tag in ("host", "svd"):
        rows = np.array([[float(x) for x in ln.split()[1:]] for ln in p.stdout.splitlines() if ln.split() and ln.split()[0] == tag])
        assert rows.shape == (40, 3)
        bad = np.isin(rows[:, 0], (5, 9, 11))
        assert np.all(rows[bad, 1] == -3.0) and np.all(rows[bad, 2] == -3.0)
        scale = np.abs(rows[~bad, 2]).max()
        assert scale > 0.1 and len(set(rows[~bad, 2])) > 30              # the elements differ from point to point
        assert np.all(np.abs(rows[~bad, 1] - rows[~bad, 2]) <= 1e-12 * scale)
