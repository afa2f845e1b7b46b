"""The derivative of the resident train along a direction in core space on the device: ttx_basis_jvp_batch / ttx_basis_jvp_tab, and the
vector operations on packed core-space buffers ttx_cores_dot, ttx_cores_axpby_dev, ttx_cores_get / ttx_cores_set
(ttcross_amd/csrc/ttx_basis_jvp.h).

The checker is tests/basis_jvp_ref.py: jvp_chain restates the definition of include/ttx.h in numpy, and exact mode must equal it bit
for bit, val and dval.  val must equal basis_tab's bit for bit in both modes.  MFMA mode sums dval in another order; its bound is the
one derived in basis_jvp_ref's docstring, |mfma - jvp_chain| <= 2 N_J u B_J with N_J = sum_m (2 n_m r_m + 2) and B_J the same sums on
absolute values -- 2 N_J u relative for cores, directions and tables without negative entries, where a dropped tile or a missing MFMA
of the three shows.  The shapes and point counts are test_gpu_basis_core_grad.py's.  Each shape's references are computed once."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import basis_core_grad_ref as C
import basis_jvp_ref as J
import basis_ref as B
import tt_ref as R
from test_gpu_basis_core_grad import NPTS, SHAPES
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

HERE = os.path.dirname(os.path.abspath(__file__))
PMAX = max(NPTS)
MODES = ("exact", "mfma")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


@functools.lru_cache(maxsize=None)
def _case(name, nonneg):
    """cores, a direction, the engine and the tables of PMAX points: computed once, never changed"""
    n, r = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)) + 1000 * nonneg + 11)
    if nonneg:
        cores = [rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1])) / (0.5 * r[k + 1]) for k in range(len(n))]
        V = [rng.uniform(0.0, 1.0, u.shape) / (0.5 * u.shape[2]) for u in cores]
        phis = [rng.uniform(0.0, 1.0, (PMAX, nk)) for nk in n]
    else:
        cores = R.rand_train(sum(map(ord, name)), n, r)
        V = [rng.standard_normal(u.shape) for u in cores]
        phis = [rng.standard_normal((PMAX, nk)) for nk in n]
    tab = B.hstack(phis)
    tab.setflags(write=False)
    val, dval = J.jvp_chain(cores, phis, V)
    return dict(n=n, r=r, d=len(n), cores=cores, V=V, phis=phis, tab=tab, tt=E.TTCross.from_cores(cores), val=val, dval=dval, bound=J.bound(cores, phis, V))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_exact_is_the_numpy_restatement_and_val_is_basis_tabs_bit_for_bit(name, monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    for nonneg in (False, True):
        cs = _case(name, nonneg)
        tt = cs["tt"]
        for p in NPTS:                                                          # a point's results depend on its own rows only: the first p of the reference
            val, dval = tt.basis_jvp_tab(cs["tab"][:p], cs["V"], "exact")
            assert _eq(val, cs["val"][:p]) and _eq(dval, cs["dval"][:p]), (nonneg, p)
        for mode in MODES:
            for p in (17, 300):
                val, _ = tt.basis_jvp_tab(cs["tab"][:p], cs["V"], mode)
                assert _eq(val, tt.basis_tab(cs["tab"][:p], mode)), (nonneg, mode, p)
    assert tt.basis_jvp_last()["mode"] == "mfma"


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_mfma_is_within_the_derived_bound(name, monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    for nonneg in (False, True):
        cs = _case(name, nonneg)
        for p in NPTS:
            _, dval = cs["tt"].basis_jvp_tab(cs["tab"][:p], cs["V"], "mfma")
            err, bnd = np.abs(dval - cs["dval"][:p]), cs["bound"][:p]
            print(name, "nonneg" if nonneg else "signed", p, "max err / bound", float(np.max(err / bnd)))
            assert np.all(err <= bnd), (nonneg, p)
            if nonneg:                                                          # relative: a dropped tile or the missing third MFMA shows
                assert np.all(cs["dval"][:p] > 0.0) and np.all(err <= 2 * J.count(cs["cores"]) * B.U * cs["dval"][:p]), p
    last = cs["tt"].basis_jvp_last()
    w = sum(cs["r"][k] * cs["n"][k] * cs["r"][k + 1] for k in range(cs["d"]))
    assert last["mode"] == "mfma" and last["ms_chain"] > 0.0 and last["ms_table"] == 0.0 and last["flops"] == 6.0 * PMAX * w


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_chunks_positions_and_repetition_change_no_bit(name, monkeypatch):
    cs = _case(name, False)
    tt, tab, V = cs["tt"], cs["tab"], cs["V"]
    perm = np.random.default_rng(5).permutation(PMAX)
    for mode in MODES:
        monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
        val, dval = tt.basis_jvp_tab(tab, V, mode)
        again = tt.basis_jvp_tab(tab, V, mode)
        assert _eq(again[0], val) and _eq(again[1], dval), mode                 # a call repeats bit for bit
        pv, pd = tt.basis_jvp_tab(np.ascontiguousarray(tab[perm]), V, mode)     # every point at another position of the batch
        assert _eq(pv, val[perm]) and _eq(pd, dval[perm]), mode
        one = tt.basis_jvp_tab(np.ascontiguousarray(tab[[257]]), V, mode)       # and alone
        assert _eq(one[0], val[[257]]) and _eq(one[1], dval[[257]]), mode
        monkeypatch.setenv("TTX_BASIS_CHUNK", "256")
        cv, cd = tt.basis_jvp_tab(tab, V, mode)
        assert _eq(cv, val) and _eq(cd, dval), mode


@pytest.mark.parametrize("name", ["mixed", "ragged", "mr6_mr8"])
def test_a_block_direction_is_basis_tab_of_the_replaced_train(name, monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    cs = _case(name, True)
    for mode in MODES:
        for i in range(cs["d"]):
            Vi = [v if k == i else np.zeros(v.shape) for k, v in enumerate(cs["V"])]
            _, dval = cs["tt"].basis_jvp_tab(cs["tab"], Vi, mode)
            rep = C.replaced(cs["cores"], i, cs["V"][i])
            want = E.TTCross.from_cores(rep).basis_tab(cs["tab"], mode)
            allow = J.bound(cs["cores"], cs["phis"], Vi) + B.bound(rep, cs["phis"])
            assert np.all(np.abs(dval - want) <= allow), (mode, i)
            assert np.all(want > 0.0) and np.all(allow < 1e-10 * want)


@pytest.mark.parametrize("name", ["mixed", "two_rows_mr5", "bond128"])
def test_adjoint_identity_against_the_devices_own_core_gradient(name, monkeypatch):
    """sum_p c_p dval_p = sum_i <G_i, V_i>, G from basis_core_grad_tab on the same engine"""
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    monkeypatch.delenv("TTX_BASIS_GRAD_STORE", raising=False)
    for nonneg in (False, True):
        cs = _case(name, nonneg)
        rng = np.random.default_rng(77)
        c = rng.uniform(0.0, 1.0, PMAX) if nonneg else rng.standard_normal(PMAX)
        allow = J.adjoint_allowance(cs["cores"], cs["phis"], c, cs["V"], C.abs_core_grad(cs["cores"], cs["phis"], c))
        for mode in MODES:
            _, dval = cs["tt"].basis_jvp_tab(cs["tab"], cs["V"], mode)
            _, G = cs["tt"].basis_core_grad_tab(cs["tab"], c, mode)
            left, right = float(np.sum(c * dval)), float(sum(np.sum(g * v) for g, v in zip(G, cs["V"])))
            print(name, mode, "adjoint", left, right, abs(left - right) / allow)
            assert abs(left - right) <= allow, (nonneg, mode)
            if nonneg:
                assert left > 0.0 and allow < 1e-9 * left


def _bases(n, rng):
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
        cols.append(x)
    return basis, np.ascontiguousarray(np.stack(cols, axis=1))


@pytest.mark.parametrize("name", ["mixed", "two_rows_mr5"])
def test_coordinates_give_what_the_host_tables_give_bit_for_bit(name, monkeypatch):
    cs = _case(name, False)
    tt, n, V = cs["tt"], cs["n"], cs["V"]
    basis, x = _bases(n, np.random.default_rng(41))
    tab = B.hstack([E.basis_table(e, nk, x[:, k]) for k, (e, nk) in enumerate(zip(basis, n))])
    for mode in MODES:
        for chunk in (None, "256"):
            monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
            if chunk:
                monkeypatch.setenv("TTX_BASIS_CHUNK", chunk)
            wv, wd = tt.basis_jvp_tab(tab, V, mode)
            val, dval = tt.basis_jvp(x, basis, J.pack(V), mode)               # a flat direction as well as a list of blocks
            assert _eq(val, wv) and _eq(dval, wd), (mode, chunk)
            assert tt.basis_jvp_last()["ms_table"] > 0.0


def test_device_pointer_entries_nan_coordinates_and_the_fit_on_device_tensors():
    """torch tensors by data_ptr() through the _dev entries, in a child process (basis_jvp_dev_worker.py says why)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "basis_jvp_dev_worker.py")], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in MODES:
        assert res[mode] == dict(batch_is_cuda=True, batch_equal=True, tab_equal=True, chunked_equal=True, nan_point_is_nan=True, nan_others_equal=True,
                                 fit_tab_equal=True, fit_batch_equal=True), (mode, res[mode])
    for key in ("dot_equal", "axpby_equal", "get_equal", "set_equal", "float32_refused", "host_v_refused", "short_v_refused"):
        assert res[key] is True, (key, res)


# ---- the vector operations -------------------------------------------------------------------------------------------------------
DOT_TRAINS = {                                                                  # tot = 59; one segment boundary (L goes from 256 to 512 past 65536) and its neighbours
    59: ([29, 30], [1, 1, 1]),
    65535: ([385, 386], [1, 85, 1]),
    65536: ([256, 256], [1, 128, 1]),
    65537: ([2767, 10000, 1], [1, 2, 3, 1]),
}


@pytest.mark.parametrize("tot", sorted(DOT_TRAINS) + ["bond128"])
def test_cores_dot_is_the_numpy_restatement_bit_for_bit(tot):
    n, r = SHAPES["bond128"] if tot == "bond128" else DOT_TRAINS[tot]
    rng = np.random.default_rng(len(n) + r[1])
    tt = E.TTCross.from_cores([rng.standard_normal((r[k], n[k], r[k + 1])) for k in range(len(n))])
    total = int(tt.core_offsets()[-1])
    assert tot == "bond128" or total == tot
    a, b = rng.standard_normal(total) * np.exp(rng.uniform(-20, 20, total)), rng.standard_normal(total)
    want = J.dot(a, b)
    got = tt.cores_dot(a, b)
    assert _bits(got) == _bits(want), (got, want)
    assert _bits(tt.cores_dot(a, b)) == _bits(want)                             # a call repeats bit for bit
    assert _bits(tt.cores_dot(tt._core_blocks(a), tt._core_blocks(b))) == _bits(want)        # lists of blocks
    assert abs(want - float(np.dot(a, b))) <= 2.0 * (total + 1) * B.U * float(np.dot(np.abs(a), np.abs(b)))
    ones = np.ones(total)
    assert tt.cores_dot(ones, ones) == float(total)                             # no element dropped or counted twice


def test_cores_get_and_set_are_bit_for_bit_and_nothing_stale_survives():
    cs = _case("mixed", False)
    cores, tab, n = cs["cores"], cs["tab"], cs["n"]
    tt = E.TTCross.from_cores(cores)                                            # an engine of its own: this test changes the cores
    flat = tt.cores_get()
    assert _eq(flat, J.pack(cores))
    tt.cores_set(flat)
    for k in range(5):
        assert _eq(tt.core(k + 1), cores[k]), k
    w = [np.cos(np.arange(nk) + 1.0) for nk in n]
    before = (tt.basis_tab(tab, "exact"), tt.norm(), tt.quad(w))               # whatever these calls leave behind is now on the engine
    other = R.rand_train(991, cs["n"], cs["r"])
    other[1][0, 0, 0] = -0.0                                                    # bits, not values
    tt.cores_set(other)                                                         # a list of blocks
    for k in range(5):
        assert _eq(tt.core(k + 1), other[k]), k
    fresh = E.TTCross.from_cores(other)
    after = (tt.basis_tab(tab, "exact"), tt.norm(), tt.quad(w))
    assert _eq(after[0], fresh.basis_tab(tab, "exact")) and _eq(after[0], B.chain(other, cs["phis"]))
    assert _bits(after[1]) == _bits(fresh.norm()) and _bits(after[2]) == _bits(fresh.quad(w))
    assert not _eq(after[0], before[0]) and after[1] != before[1] and after[2] != before[2]
    assert _eq(tt.cores_get(), J.pack(other))
    # the host form of axpby is the three operations of the device kernel
    x, y = J.pack(cores), J.pack(other)
    assert _eq(tt.cores_axpby(0.3, x, -1.7, y), J.axpby(0.3, x, -1.7, y))
    with pytest.raises(ValueError):
        tt.cores_set(flat[:-1])


def test_empty_calls_refusals_and_figures(monkeypatch):
    monkeypatch.delenv("TTX_BASIS_CHUNK", raising=False)
    L = E.load_library()
    cs = _case("mixed", False)
    tt, n, r = cs["tt"], cs["n"], cs["r"]
    EINVAL, ESTATE, nul = 1, 4, ctypes.POINTER(ctypes.c_double)()
    total = int(tt.core_offsets()[-1])
    x, v, val, dval = np.full((4, 5), 0.5), np.ones(total), np.full(4, 7.0), np.full(4, 7.0)
    arr = (E._Basis * 5)(*[E._Basis(E.TTX_BASIS_COS, 0, 0.0, 1.0, None) for _ in range(5)])
    t4 = np.ascontiguousarray(cs["tab"][:4])

    def refused(rc, entry):
        return rc == EINVAL and entry in L.ttx_last_error().decode() and np.all(val == 7.0) and np.all(dval == 7.0)

    # npts = 0 launches nothing and touches nothing
    assert L.ttx_basis_jvp_tab(tt._h, 0, nul, nul, nul, nul, 0) == 0
    assert L.ttx_basis_jvp_batch(tt._h, 0, nul, None, nul, E._dp(val), E._dp(dval), 1) == 0 and np.all(val == 7.0) and np.all(dval == 7.0)
    last = tt.basis_jvp_last()
    assert last["flops"] == 0.0 and last["ms_chain"] == 0.0 and last["ms_table"] == 0.0 and last["mode"] == "mfma"
    v0, d0 = tt.basis_jvp_tab(np.zeros((0, sum(n))), cs["V"], "mfma")
    assert v0.shape == (0,) and d0.shape == (0,)
    # a null v, dval or table, an unknown mode, negative npts
    tab_ = "ttx_basis_jvp_tab:"
    assert refused(L.ttx_basis_jvp_tab(tt._h, 4, E._dp(t4), nul, E._dp(val), E._dp(dval), 0), tab_)
    assert refused(L.ttx_basis_jvp_tab(tt._h, 4, E._dp(t4), E._dp(v), E._dp(val), nul, 0), tab_)
    assert refused(L.ttx_basis_jvp_tab(tt._h, 4, nul, E._dp(v), E._dp(val), E._dp(dval), 0), tab_)
    assert refused(L.ttx_basis_jvp_tab(tt._h, 4, E._dp(t4), E._dp(v), E._dp(val), E._dp(dval), 3), tab_)
    assert refused(L.ttx_basis_jvp_tab(tt._h, -1, E._dp(t4), E._dp(v), E._dp(val), E._dp(dval), 0), tab_)
    assert refused(L.ttx_basis_jvp_tab_dev(tt._h, 4, None, None, None, None, 0), "ttx_basis_jvp_tab_dev:")
    bat = "ttx_basis_jvp_batch:"
    assert refused(L.ttx_basis_jvp_batch(tt._h, 4, E._dp(x), None, E._dp(v), E._dp(val), E._dp(dval), 0), bat)
    assert refused(L.ttx_basis_jvp_batch(tt._h, 4, E._dp(x), arr, nul, E._dp(val), E._dp(dval), 0), bat)
    assert refused(L.ttx_basis_jvp_batch(tt._h, 4, E._dp(x), arr, E._dp(v), E._dp(val), E._dp(dval), 7), bat)
    assert refused(L.ttx_basis_jvp_batch_dev(tt._h, 4, None, arr, None, None, None, 0), "ttx_basis_jvp_batch_dev:")
    arr2 = (E._Basis * 5)(*([arr[0]] * 3 + [E._Basis(9, 0, 0.0, 1.0, None)] + [arr[0]]))       # an unknown kind, before any launch
    assert refused(L.ttx_basis_jvp_batch(tt._h, 4, E._dp(x), arr2, E._dp(v), E._dp(val), E._dp(dval), 0), bat + " mode 4")
    out = ctypes.c_double(7.0)
    assert L.ttx_cores_dot(tt._h, nul, E._dp(v), ctypes.byref(out)) == EINVAL and L.ttx_cores_dot(tt._h, E._dp(v), E._dp(v), None) == EINVAL and out.value == 7.0
    assert L.ttx_cores_dot_dev(tt._h, None, None, ctypes.byref(out)) == EINVAL and "ttx_cores_dot_dev:" in L.ttx_last_error().decode()
    assert L.ttx_cores_axpby_dev(tt._h, 1.0, None, 1.0, None) == EINVAL and "ttx_cores_axpby_dev:" in L.ttx_last_error().decode()
    assert L.ttx_cores_get_dev(tt._h, None) == EINVAL and L.ttx_cores_set_dev(tt._h, None) == EINVAL
    assert L.ttx_cores_get(tt._h, nul) == EINVAL and L.ttx_cores_set(tt._h, nul) == EINVAL
    with pytest.raises(ValueError):
        tt.basis_jvp(x, [("cos", 0.0, 1.0)] * 4, v)
    with pytest.raises(ValueError):
        tt.basis_jvp_tab(cs["tab"][:4], v[:-1])
    with pytest.raises(ValueError):
        tt.cores_dot(v, v[:-1])
    # an engine without a train (five modes, as the tables here): TTX_ESTATE
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    assert L.ttx_basis_jvp_tab(fresh._h, 4, E._dp(t4), E._dp(v), E._dp(val), E._dp(dval), 0) == ESTATE and np.all(dval == 7.0)
    assert L.ttx_basis_jvp_batch(fresh._h, 4, E._dp(x), arr, E._dp(v), E._dp(val), E._dp(dval), 0) == ESTATE
    assert L.ttx_cores_dot(fresh._h, E._dp(v), E._dp(v), ctypes.byref(out)) == ESTATE and L.ttx_cores_get(fresh._h, E._dp(v)) == ESTATE
    # val may be null; the figures of the last call; auto is one of the two modes
    w = sum(r[k] * n[k] * r[k + 1] for k in range(5))
    tab, vf = np.ascontiguousarray(cs["tab"]), J.pack(cs["V"])
    res = {m: tt.basis_jvp_tab(tab, vf, m) for m in MODES}
    for m in MODES:
        d2 = np.full(PMAX, 7.0)
        assert L.ttx_basis_jvp_tab(tt._h, PMAX, E._dp(tab), E._dp(vf), nul, E._dp(d2), E.EVAL_MODES[m]) == 0
        assert _eq(d2, res[m][1]), m
        tt.basis_jvp_tab(tab[:257], vf, m)
        last = tt.basis_jvp_last()
        assert last["mode"] == m and last["flops"] == 6.0 * 257 * w and last["ms_chain"] > 0.0 and last["ms_table"] == 0.0
    av, ad = tt.basis_jvp_tab(tab, vf, "auto")
    ran = tt.basis_jvp_last()["mode"]
    assert ran in MODES and _eq(av, res[ran][0]) and _eq(ad, res[ran][1])
    for k, core in enumerate(cs["cores"]):                                      # the train is untouched
        assert np.array_equal(tt.core(k + 1), core)
