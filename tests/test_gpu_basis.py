"""The resident train in a function basis at real points on the device: ttx_basis_batch / ttx_basis_tab and their _dev forms
(ttcross_amd/csrc/ttx_basis.h).

The checker is tests/basis_ref.py: chain restates the definition of include/ttx.h in numpy, and exact mode must equal it bit for
bit.  MFMA mode sums in another order; its bound is the one derived in basis_ref's docstring, |mfma - chain| <= 2 N u B with
N = sum_i (n_i r_i + 2) and B the chain on absolute values -- 2 N u relative for trains and tables without negative entries, where a
dropped tile or term shows.  Nothing tighter is asserted between the two modes.  Each shape's reference is computed once."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import basis_ref as B
import tt_ref as R
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {
    "mixed": ([7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]),
    "two_rows_mr5": ([4, 5, 3, 2], [1, 16, 33, 65, 1]),           # rank 65: two rows per lane in exact mode, MR = 5 in MFMA mode
    "bond128": ([2, 2, 2], [1, 128, 128, 1]),
    "mr6_mr8": ([3, 2, 3], [1, 96, 113, 1]),                      # MR = 6 and, below 128, MR = 8
    "d2": ([5, 7], [1, 3, 1]),
}
NPTS = (1, 15, 17, 255, 257, 300)
PMAX = max(NPTS)
MODES = ("exact", "mfma")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _case(name, nonneg):
    """cores, the engine, the tables of PMAX points, chain and bound at them: computed once, never changed"""
    n, r = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 1000 * nonneg)
    if nonneg:
        cores = [rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1])) / (0.5 * r[k + 1]) for k in range(len(n))]
        phis = [rng.uniform(0.0, 1.0, (PMAX, nk)) for nk in n]
    else:
        cores = R.rand_train(sum(map(ord, name)), n, r)
        phis = [rng.standard_normal((PMAX, nk)) for nk in n]
    tab = B.hstack(phis)
    ref, bnd = B.chain(cores, phis), B.bound(cores, phis)
    for a in (tab, ref, bnd):
        a.setflags(write=False)
    return dict(n=n, cores=cores, tt=E.TTCross.from_cores(cores), tab=tab, ref=ref, bnd=bnd, N=B.count(cores))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_exact_tab_is_the_numpy_chain_bit_for_bit(name, monkeypatch):
    for nonneg in (False, True):
        c = _case(name, nonneg)
        for p in NPTS:
            got = c["tt"].basis_tab(c["tab"][:p], "exact")
            assert np.array_equal(_bits(got), _bits(c["ref"][:p])), (nonneg, p)
    c = _case(name, False)
    monkeypatch.setenv("TTX_BASIS_CHUNK", "64")                                  # 300 points cross four chunk borders, the last chunk is short
    assert np.array_equal(_bits(c["tt"].basis_tab(c["tab"], "exact")), _bits(c["ref"]))
    assert c["tt"].basis_last()["mode"] == "exact"


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mfma_tab_is_within_the_derived_bound(name, monkeypatch):
    for nonneg in (False, True):
        c = _case(name, nonneg)
        monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
        for p in NPTS + (-64,):
            if p < 0:
                monkeypatch.setenv("TTX_BASIS_CHUNK", str(-p))
                p = PMAX
            got = c["tt"].basis_tab(c["tab"][:p], "mfma")
            err = np.abs(got - c["ref"][:p])
            print(name, "nonneg" if nonneg else "signed", p, "max err / bound", float(np.max(err / c["bnd"][:p])))
            assert np.all(err <= c["bnd"][:p]), (nonneg, p)
            if nonneg:
                assert np.all(c["ref"][:p] > 0.0) and np.all(err <= 2 * c["N"] * B.U * c["ref"][:p]), p
    assert c["tt"].basis_last()["mode"] == "mfma"


def _ind(n, seed, npts):
    rng = np.random.default_rng(seed)
    n = np.asarray(n)
    ind = rng.integers(0, 2 ** 31 - 1, (npts, n.size)) % n + 1
    ind[0], ind[-1] = 1, n
    return np.ascontiguousarray(ind.astype(np.int32))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_unit_vector_tables_give_tijk_batch_bit_for_bit(name):
    c = _case(name, False)
    ind = _ind(c["n"], 5, 257)
    tab = B.hstack(B.unit_tables(c["n"], ind))
    want = c["tt"].tijk_batch(ind, "exact")
    assert np.array_equal(c["tt"].basis_tab(tab, "exact"), want)                # == : the sign of a zero is not compared
    assert np.any(want != 0.0)


def _bases(n, rng):
    """per mode a COS or a LINEAR entry, alternating, and points that lie inside, on the ends and (LINEAR) outside"""
    basis, cols = [], []
    for k, nk in enumerate(n):
        if k % 2 == 0:
            a, b = -1.0 - k, 2.5 + k
            basis.append(("cos", a, b, True) if k % 4 == 0 else ("cos", a, b))
            x = rng.uniform(a, b, PMAX)
            x[:2] = a, b
        else:
            t = np.sort(rng.uniform(-2.0, 3.0, nk))
            basis.append(("linear", t))
            x = rng.uniform(t[0] - 0.5, t[-1] + 0.5, PMAX)
            x[:nk] = t[:PMAX]
        cols.append(x)
    return basis, np.ascontiguousarray(np.stack(cols, axis=1))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_basis_batch_is_basis_tab_of_the_host_tables_bit_for_bit(name, monkeypatch):
    c = _case(name, False)
    tt, n = c["tt"], c["n"]
    basis, x = _bases(n, np.random.default_rng(31))
    tab = B.hstack([E.basis_table(e, nk, x[:, k]) for k, (e, nk) in enumerate(zip(basis, n))])
    assert np.isfinite(tab).all()
    for mode in MODES:
        want = tt.basis_tab(tab, mode)
        for p in (1, 17, 300):
            assert np.array_equal(_bits(tt.basis_batch(x[:p], basis, mode)), _bits(want[:p])), (mode, p)
        monkeypatch.setenv("TTX_BASIS_CHUNK", "64")
        assert np.array_equal(_bits(tt.basis_batch(x, basis, mode)), _bits(want)), mode
        monkeypatch.delenv("TTX_BASIS_CHUNK")
    one = ("cos", -3.0, 4.0, True)                                              # a single entry stands for all modes
    tab = B.hstack([E.basis_table(one, nk, x[:, k]) for k, nk in enumerate(n)])
    assert np.array_equal(_bits(tt.basis_batch(x, one, "exact")), _bits(tt.basis_tab(tab, "exact")))


def test_device_pointer_entries_equal_the_host_entries():
    """torch tensors by data_ptr() through ttx_basis_batch_dev / ttx_basis_tab_dev, in a child process (basis_dev_worker.py says why)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "basis_dev_worker.py")], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert res[mode] == dict(batch_is_cuda=True, batch_equal=True, tab_is_cuda=True, tab_equal=True, chunked_equal=True, empty=[0]), (mode, res[mode])
    assert res["float32_refused"] and res["shape_refused"] and res.get("other_device_refused", True)


@pytest.mark.parametrize("name", ["mixed", "two_rows_mr5", "bond128"])
def test_a_points_value_does_not_depend_on_the_batch(name, monkeypatch):
    c = _case(name, False)
    tt, tab = c["tt"], c["tab"]
    five = tab[[3, 77, 150, 151, 299]]
    rng = np.random.default_rng(2)
    for mode in MODES:
        monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
        base = tt.basis_tab(five, mode)
        for total, chunk in ((17, None), (300, None), (300, 64), (300, 7)):
            pos = np.sort(rng.choice(total, 5, replace=False))
            batch = tab[rng.integers(0, PMAX, total)].copy()
            batch[pos] = five
            if chunk is None:
                monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
            else:
                monkeypatch.setenv("TTX_BASIS_CHUNK", str(chunk))
            assert np.array_equal(_bits(tt.basis_tab(batch, mode)[pos]), _bits(base)), (mode, total, chunk)


def test_cos_coefficient_train_evaluates_to_the_product_of_its_cosines():
    """A rank-1 train of delta coefficients, core m = e_(k_m): f(x) = prod_m c_(k_m) cos(k_m pi (x_m - a_m)/(b_m - a_m)).
    Against the product P of the host table entries the device sums the same single non-zero term among zeros: within 2 N u B of
    basis_ref.  Against the true product: every factor is at most 1 in magnitude, a table entry is within (2 + 7 |arg|) u of the
    true cosine (test_basis_cpu.py) and numpy's cosine within 1 u, the d - 1 products of the comparison value round once each:
    |P - numpy| <= sum_m (3 + 7 |arg_m|) u + d u."""
    n, ks = [9, 6, 12, 5], [3, 0, 11, 4]
    box = [(-10.0, 10.0), (0.0, 1.0), (-2.0, 5.0), (1.0, 1.5)]
    cores = [np.zeros((1, nk, 1)) for nk in n]
    for c, k in zip(cores, ks):
        c[0, k, 0] = 1.0
    tt = E.TTCross.from_cores(cores)
    rng = np.random.default_rng(6)
    x = np.stack([rng.uniform(a, b, 300) for a, b in box], axis=1)
    basis = [("cos", a, b, True) for a, b in box]
    phis = [E.basis_table(e, nk, x[:, m]) for m, (e, nk) in enumerate(zip(basis, n))]
    args = [k * np.pi * (x[:, m] - a) / (b - a) for m, (k, (a, b)) in enumerate(zip(ks, box))]
    true = np.prod([np.cos(g) * (0.5 if k == 0 else 1.0) for g, k in zip(args, ks)], axis=0)
    slack = (sum(3 + 7 * np.abs(g) for g in args) + len(n)) * B.U
    bnd = B.bound(cores, phis)
    for mode in MODES:
        got = tt.basis_batch(x, basis, mode)
        assert np.all(np.abs(got - B.chain(cores, phis)) <= bnd), mode
        assert np.all(np.abs(got - true) <= bnd + slack), mode
    assert np.abs(true).max() > 0.1


@pytest.mark.parametrize("name", ["mixed", "two_rows_mr5", "d2"])
def test_linear_basis_at_its_nodes_is_tijk_batch_bit_for_bit(name):
    c = _case(name, False)
    tt, n = c["tt"], c["n"]
    rng = np.random.default_rng(12)
    nodes = [np.sort(rng.uniform(-1.0, 1.0, nk)) * (k + 1) for k, nk in enumerate(n)]
    ind = _ind(n, 3, 257)
    x = np.ascontiguousarray(np.stack([t[ind[:, k] - 1] for k, t in enumerate(nodes)], axis=1))
    got = tt.basis_batch(x, [("linear", t) for t in nodes], "exact")
    assert np.array_equal(got, tt.tijk_batch(ind, "exact"))                     # == : the sign of a zero is not compared


def test_nan_coordinates_and_arguments_beyond_the_cosines_range_stay_with_their_point():
    c = _case("mixed", False)
    tt, n = c["tt"], c["n"]
    rng = np.random.default_rng(44)
    basis = [("cos", 0.0, 1.0), ("linear", [0.0, 1.0]), ("cos", 0.0, 1.0, True), ("cos", 0.0, 1.0), ("linear", np.linspace(0.0, 1.0, 9))]
    x = rng.uniform(0.0, 1.0, (300, 5))
    bad = x.copy()
    bad[7, 1] = np.nan                                                          # LINEAR: a NaN row
    bad[100, 2] = np.nan                                                        # COS: NaN
    bad[130, 0] = 2.0 ** 18                                                     # COS, n = 7: j pi 2^18 > 2^19 from j = 1 on
    bad[299, 4] = np.nan
    hit = np.zeros(300, bool)
    hit[[7, 100, 130, 299]] = True
    for mode in MODES:
        clean, got = tt.basis_batch(x, basis, mode), tt.basis_batch(bad, basis, mode)
        assert np.isfinite(clean).all()
        assert np.isnan(got[hit]).all(), mode
        assert np.array_equal(_bits(got[~hit]), _bits(clean[~hit])), mode


def test_conditions_refusals_and_figures():
    L = E.load_library()
    c = _case("mixed", False)
    tt, n, tab = c["tt"], c["n"], c["tab"]
    EINVAL, nul = 1, ctypes.POINTER(ctypes.c_double)()
    out, x = np.zeros(4), np.full((4, 5), 0.5)
    arr = (E._Basis * 5)(*[E._Basis(E.TTX_BASIS_COS, 0, 0.0, 1.0, None) for _ in range(5)])
    t4 = np.ascontiguousarray(tab[:4])

    def refused(rc, entry):
        return rc == EINVAL and entry in L.ttx_last_error().decode()

    # npts = 0 succeeds and launches nothing
    assert L.ttx_basis_tab(tt._h, 0, nul, nul, 0) == 0 and L.ttx_basis_batch(tt._h, 0, nul, None, nul, 1) == 0
    assert L.ttx_basis_tab_dev(tt._h, 0, None, None, 2) == 0 and L.ttx_basis_batch_dev(tt._h, 0, None, None, None, 0) == 0
    assert tt.basis_tab(np.zeros((0, sum(n))), "mfma").shape == (0,) and tt.basis_last()["flops"] == 0.0
    # unknown mode, null pointers, negative npts
    assert refused(L.ttx_basis_tab(tt._h, 4, E._dp(t4), E._dp(out), 3), "ttx_basis_tab:")
    assert refused(L.ttx_basis_tab(tt._h, 0, nul, nul, -1), "ttx_basis_tab:")
    assert refused(L.ttx_basis_tab(tt._h, 4, nul, E._dp(out), 0), "ttx_basis_tab:")
    assert refused(L.ttx_basis_tab(tt._h, 4, E._dp(t4), nul, 0), "ttx_basis_tab:")
    assert refused(L.ttx_basis_tab(tt._h, -1, E._dp(t4), E._dp(out), 0), "ttx_basis_tab:")
    assert refused(L.ttx_basis_tab_dev(tt._h, 4, None, None, 0), "ttx_basis_tab_dev:")
    assert refused(L.ttx_basis_batch(tt._h, 4, E._dp(x), None, E._dp(out), 0), "ttx_basis_batch:")
    assert refused(L.ttx_basis_batch(tt._h, 4, nul, arr, E._dp(out), 0), "ttx_basis_batch:")
    assert refused(L.ttx_basis_batch(tt._h, 4, E._dp(x), arr, E._dp(out), 7), "ttx_basis_batch:")
    assert refused(L.ttx_basis_batch_dev(tt._h, 4, None, arr, None, 0), "ttx_basis_batch_dev:")
    # descriptors: unknown kind, b <= a, nodes out of order -- each before any launch
    for entry, match in ((E._Basis(9, 0, 0.0, 1.0, None), "unknown basis kind 9"), (E._Basis(E.TTX_BASIS_COS, 0, 1.0, 1.0, None), "a < b")):
        arr2 = (E._Basis * 5)(*([arr[0]] * 3 + [entry] + [arr[0]]))
        assert refused(L.ttx_basis_batch(tt._h, 4, E._dp(x), arr2, E._dp(out), 0), "ttx_basis_batch: mode 4")
        assert match in L.ttx_last_error().decode()
    with pytest.raises(E.TTXError, match="ttx_basis_batch: mode 2: the nodes are not strictly ascending"):
        tt.basis_batch(x, [("cos", 0.0, 1.0), ("linear", [1.0, 0.0])] + [("cos", 0.0, 1.0)] * 3, "exact")
    with pytest.raises(ValueError):
        tt.basis_batch(x, [("cos", 0.0, 1.0)] * 4)
    with pytest.raises(ValueError):
        tt.basis_tab(tab[:, :-1])
    # an engine of a two-process job (test_gpu_tijk_batch.py builds the same one): refused by every entry, which names itself
    s = D.ising_setup("c", 6, 9)
    mp = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"], nproc=2, world_rank=0, world_size=2)
    i5, v = np.ones((1, 5), np.int32), ctypes.c_double()
    want = L.ttx_ijk(mp._h, E._ip(i5), ctypes.byref(v))
    assert want != 0
    x5 = np.full((1, 5), 0.5)
    assert L.ttx_basis_batch(mp._h, 1, E._dp(x5), arr, E._dp(out), 0) == want and "ttx_basis_batch:" in L.ttx_last_error().decode()
    assert L.ttx_basis_tab(mp._h, 1, E._dp(np.ones((1, 45))), E._dp(out), 0) == want and "ttx_basis_tab:" in L.ttx_last_error().decode()
    assert L.ttx_basis_tab_dev(mp._h, 1, None, None, 0) == want and L.ttx_basis_batch_dev(mp._h, 1, None, arr, None, 0) == want
    # the figures of the last call; auto is one of the two modes
    r = [1, 3, 17, 5, 4, 1]
    w = sum(r[k] * n[k] * r[k + 1] for k in range(5))
    vals = {m: tt.basis_tab(tab, m) for m in MODES}
    for m in MODES:
        tt.basis_tab(tab[:257], m)
        last = tt.basis_last()
        assert last["mode"] == m and last["flops"] == 2.0 * 257 * w and last["ms_chain"] > 0.0 and last["ms_table"] == 0.0
    tt.basis_batch(np.full((300, 5), 0.5), ("cos", 0.0, 1.0), "exact")
    assert tt.basis_last()["ms_table"] > 0.0
    auto = tt.basis_tab(tab, "auto")
    ran = tt.basis_last()["mode"]
    assert ran in MODES and np.array_equal(_bits(auto), _bits(vals[ran]))
    assert np.array_equal(_bits(tt.basis_tab(tab, "exact")), _bits(vals["exact"]))      # the train and the earlier results are untouched
    for k, core in enumerate(c["cores"]):
        assert np.array_equal(tt.core(k + 1), core)


def test_fortran_basisval_at_nodes_and_against_its_own_sum():
    """the drop-in tt_lib: basisval(tt, x, kind, a, b, res, mode) (one ttx_basis_batch call) on a host train of rank 3.  With hat
    functions at their own nodes it equals the batched tijk, the device's chain, exactly, and the host's element to 1e-12 of the
    element scale (the tolerance of test_fortran_tijk_of_many_indices_equals_its_own_loop).  With the cosine basis both modes are
    held against the program's plain sum over all 360 multi-indices at 1e-12 of S = the sum of the terms' absolute values: a term
    there is a product of four run-time-library cosines whose arguments (at most 5 pi) carry about 7 |arg| u each, some 500 u per
    term, the summation adds 360 u, and the device's own 2 N u B is of the same order: 1e-13 S in all, a factor 10 in hand."""
    from conftest import fortran_exe
    exe = fortran_exe("test_tt_basis")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("done"), p.stdout[-2000:] + p.stderr[-2000:]
    rows = {tag: np.array([[float(v) for v in ln.split()[1:]] for ln in p.stdout.splitlines() if ln.split() and ln.split()[0] == tag])
            for tag in ("node", "cos")}
    node, cos = rows["node"], rows["cos"]
    assert node.shape == (24, 4) and cos.shape == (24, 5)
    scale = np.abs(node[:, 3]).max()
    assert scale > 0.1 and len(set(node[:, 3])) > 12
    assert np.array_equal(node[:, 1], node[:, 2])
    assert np.all(np.abs(node[:, 1] - node[:, 3]) <= 1e-12 * scale)
    assert np.abs(cos[:, 3]).max() > 1e-3 * cos[:, 4].max()
    for col in (1, 2):
        assert np.all(np.abs(cos[:, col] - cos[:, 3]) <= 1e-12 * cos[:, 4]), col


def test_host_route_of_the_driver_agrees_within_the_bound():
    """drivers.basis_host (every core pulled, one numpy product per mode: yet another summation order) against both device modes"""
    c = _case("mixed", True)
    tt, n = c["tt"], c["n"]
    rng = np.random.default_rng(3)
    basis = [("linear", np.linspace(0.0, 1.0, nk)) if nk > 1 and k % 2 else ("cos", 0.0, 1.0, True) for k, nk in enumerate(n)]
    x = rng.uniform(0.0, 1.0, (64, len(n)))
    phis = [E.basis_table(e, nk, x[:, k]) for k, (e, nk) in enumerate(zip(basis, n))]
    host, bnd = D.basis_host(tt, x, basis), B.bound(c["cores"], phis)
    for mode in MODES:
        assert np.all(np.abs(tt.basis_batch(x, basis, mode) - host) <= bnd), mode
    assert np.abs(host).max() > 0.0
