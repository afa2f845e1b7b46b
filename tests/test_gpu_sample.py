"""Samples drawn from the resident train on the device: ttx_sample / ttx_sample_dev (ttcross_amd/csrc/ttx_sample.h).

The checker is tests/sample_ref.py (numpy float64): verify walks every sample along the device's own indices and allows another
index than the reference's only where t lies within 4 N u Bc(n_k) of an edge (the derivation is in its docstring); at most
0.1 % of a test's samples may have such a mode.  val must be tijk_batch(ind, "exact") bit for bit.  logq is compared with the
reference's along the same indices: per drawn mode the ratio p / c(n) carries the 4 N u of the two sums, and the allowance
8 u (1 + |log term|) covers the division (1 u), a device log within 4 ulp of the correctly rounded one, numpy's log (1 ulp)
and the addition into the running sum (1 u of a partial sum bounded by d max |log term|, spread over the d terms)."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sample_ref as S
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

U = S.U
HERE = os.path.dirname(os.path.abspath(__file__))
ALL = [(k, False) for k in S.CASES] + [(k, True) for k in S.SIGNED]
IDS = [k + ("_signed" if s else "") for k, s in ALL]


@functools.lru_cache(maxsize=None)
def _run(name, signed=False):
    """(engine, cores, u, w, device result) of a case: drawn once, shared, never modified"""
    cores, u, w = S.case(name, signed)
    tt = E.TTCross.from_cores(cores)
    res = tt.sample(u, w)
    for v in res.values():
        v.setflags(write=False)
    return tt, cores, u, w, res


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("ind", "logq", "val"))


def _logq_bound(d, N, maxlog):
    return d * (4.0 * N * U + 8.0 * U * (1.0 + maxlog))


@pytest.mark.parametrize("name,signed", ALL, ids=IDS)
def test_indices_are_the_definitions_and_val_is_the_element_bit_for_bit(name, signed):
    tt, cores, u, w, res = _run(name, signed)
    chk = S.verify(cores, u, w, None, res["ind"])
    print(name, "signed" if signed else "non-negative", "N", chk["N"], "undecided", chk["undecided"], "of", S.NPTS)
    assert chk["undecided"] <= S.NPTS // 1000
    assert res["val"].tobytes() == tt.tijk_batch(res["ind"], "exact").tobytes()
    assert np.all(np.isfinite(res["logq"])) and np.all(res["logq"] <= 0.0)


@pytest.mark.parametrize("name", list(S.CASES))
def test_logq_is_the_references_along_the_devices_indices(name):
    tt, cores, u, w, res = _run(name)
    chk = S.verify(cores, u, w, None, res["ind"])
    bound = _logq_bound(len(cores), chk["N"], chk["maxlog"])
    diff = np.abs(res["logq"] - chk["logq"])
    print(name, "max |logq - ref| / bound", float((diff / bound).max()))
    assert np.all(diff <= bound)
    if name == "d3":                                                   # and the dense density; its own sums carry 2 N u each
        rho = S.dense_density(cores, w)[tuple((res["ind"] - 1).T)]
        assert np.all(np.abs(np.exp(res["logq"]) - rho) <= rho * (bound + 4.0 * chk["N"] * U))


def test_a_sample_does_not_depend_on_its_neighbours_or_on_the_call():
    tt, cores, u, w, res = _run("d8_unequal")
    assert _same(tt.sample(u, w), res)                                 # repetition
    perm = np.random.default_rng(1).permutation(u.shape[0])
    got = tt.sample(u[perm], w)
    assert all(got[k].tobytes() == res[k][perm].tobytes() for k in res)
    dup = tt.sample(np.repeat(u[:300], 3, axis=0), w)
    assert all(dup[k].tobytes() == np.repeat(res[k][:300], 3, axis=0).tobytes() for k in res)
    for m in (1, 3, 4, 5):                                             # npts mod 4: the waves of the last workgroup
        part = tt.sample(u[:m], w)
        assert all(part[k].tobytes() == res[k][:m].tobytes() for k in res)
    t2 = E.TTCross.from_cores(cores)
    assert _same(t2.sample(u, w), res)
    only = tt.sample(u, w, want=("ind",))
    assert sorted(only) == ["ind"] and only["ind"].tobytes() == res["ind"].tobytes()
    byseed = tt.sample(50, w, seed=5)
    assert _same(byseed, tt.sample(np.random.default_rng(5).random((50, len(cores))), w))


def test_the_chunk_size_does_not_enter():
    """TTX_SAMPLE_CHUNK = 64 and 1000 against the default, each in a fresh child process"""
    base = dict(os.environ)
    base.pop("TTX_SAMPLE_CHUNK", None)
    out = []
    for chunk in (None, "64", "1000"):
        env = base if chunk is None else dict(base, TTX_SAMPLE_CHUNK=chunk)
        p = subprocess.run([sys.executable, os.path.join(HERE, "sample_worker.py"), "chunk", "long_modes"], capture_output=True, text=True, timeout=240, env=env)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        out.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert out[0]["digest"] == out[1]["digest"] == out[2]["digest"] and all(o["failed"] == 0 for o in out)
    res = _run("long_modes")[4]
    import hashlib
    assert out[0]["digest"] == hashlib.sha256(res["ind"].tobytes() + res["logq"].tobytes() + res["val"].tobytes()).hexdigest()


def test_device_entry_equals_the_host_entry():
    """torch tensors by data_ptr() through ttx_sample_dev, in a child process (sample_worker.py says why)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "sample_worker.py"), "dev"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["is_cuda"] and r["dtypes"] == ["torch.int32", "torch.float64", "torch.float64"]
    assert r["equal"] and r["failed"] == 1 and r["only_ind"] == ["ind"] and r["chain"] and r["empty"] == [0, 8] and r["float32_refused"]


def test_fixed_modes():
    tt, cores, u, w, _ = _run("d6_size1_rank1")
    fixed = [0, 1, 0, 0, 3, 0]
    res = tt.sample(u, w, fixed)
    assert np.all(res["ind"][:, 1] == 1) and np.all(res["ind"][:, 4] == 3)
    chk = S.verify(cores, u, w, fixed, res["ind"])
    assert chk["undecided"] <= S.NPTS // 1000
    assert res["val"].tobytes() == tt.tijk_batch(res["ind"], "exact").tobytes()
    assert np.all(np.abs(res["logq"] - chk["logq"]) <= _logq_bound(6, chk["N"], chk["maxlog"]))
    # logq has no contribution from a fixed mode: the dense conditional density on d3 with mode 2 held
    t3, c3, u3, w3, _ = _run("d3")
    f3 = [0, 4, 0]
    r3 = t3.sample(u3, w3, f3)
    k3 = S.verify(c3, u3, w3, f3, r3["ind"])
    rho = S.dense_density(c3, w3, f3)[r3["ind"][:, 0] - 1, 0, r3["ind"][:, 2] - 1]
    assert np.all(r3["ind"][:, 1] == 4)
    assert np.all(np.abs(np.exp(r3["logq"]) - rho) <= rho * (_logq_bound(3, k3["N"], k3["maxlog"]) + 4.0 * k3["N"] * U))
    u_nan = u3.copy()
    u_nan[:, 1] = np.nan                                               # the u of a fixed mode is not looked at
    assert _same(t3.sample(u_nan, w3, f3), r3)


def test_edges_of_u():
    tt, cores, u, w, base = _run("d3")
    n = [c.shape[1] for c in cores]
    v = u[:40].copy()
    v[3], v[11], v[17] = 0.0, np.nextafter(1.0, 0.0), 1.0
    v[23, 1], v[29, 2] = np.nan, -0.5
    v[31, 0] = -0.0                                                    # counts as 0
    res = tt.sample(v, w)
    assert tt.sample_last()["failed"] == 2
    assert res["ind"][3].tolist() == [1, 1, 1] and res["ind"][11].tolist() == n and res["ind"][17].tolist() == n
    for s in (23, 29):
        assert np.all(res["ind"][s] == 0) and np.isnan(res["logq"][s]) and res["val"][s] == 0.0
    assert res["ind"][31, 0] == 1
    ref = S.draw(cores, v, w)
    touched = np.zeros(40, bool)
    touched[[3, 11, 17, 23, 29, 31]] = True
    assert np.array_equal(res["ind"][[3, 11, 17, 23, 29]], ref[0][[3, 11, 17, 23, 29]]) and np.array_equal(np.isnan(res["logq"]), ref[3])
    assert all(res[k][~touched].tobytes() == base[k][:40][~touched].tobytes() for k in res)
    assert res["val"].tobytes() == np.where(ref[3], 0.0, tt.tijk_batch(np.where(ref[3][:, None], 1, res["ind"]).astype(np.int32), "exact")).tobytes()


def test_degenerate_trains():
    cores, u, w = S.case("d3")
    u = u[:500]
    zero = E.TTCross.from_cores([np.zeros_like(c) for c in cores])
    res = zero.sample(u, w)
    assert zero.sample_last()["failed"] == 500
    assert np.all(res["ind"] == 0) and np.all(np.isnan(res["logq"])) and np.all(res["val"] == 0.0)
    hole = [c.copy() for c in cores]
    hole[1][:, 2, :] = 0.0                                             # G_2(:, 3, :) = 0: index 3 is never drawn at mode 2
    th = E.TTCross.from_cores(hole)
    res = th.sample(u, w)
    assert th.sample_last()["failed"] == 0 and not np.any(res["ind"][:, 1] == 3) and set(res["ind"][:, 1]) == {1, 2, 4, 5, 6, 7}
    assert S.verify(hole, u, w, None, res["ind"])["undecided"] == 0
    nan = [c.copy() for c in cores]
    nan[1][1, 4, 0] = np.nan                                           # an input with a defined result: the call returns
    tn = E.TTCross.from_cores(nan)
    res = tn.sample(u, w)
    n = np.array([c.shape[1] for c in cores])
    assert np.all(res["ind"] >= 0) and np.all(res["ind"] <= n[None, :])
    failed = np.all(res["ind"] == 0, axis=1)
    assert np.all((res["ind"] > 0)[~failed]) and tn.sample_last()["failed"] == int(failed.sum()) > 0
    assert np.all(np.isnan(res["logq"][failed])) and np.all(res["val"][failed] == 0.0)


def test_refusals():
    L = E.load_library()
    tt, cores, u, w, _ = _run("d3")
    EINVAL, ESTATE = 1, 4
    empty = tt.sample(np.zeros((0, 3)), w)
    assert empty["ind"].shape == (0, 3) and empty["logq"].shape == (0,) and tt.sample(0)["val"].shape == (0,)
    for bad in ([0, 8, 0], [-1, 0, 0], [0, 0, 5]):
        with pytest.raises(E.TTXError):
            tt.sample(u[:4], w, bad)
    with pytest.raises(ValueError):
        tt.sample(u[:4], w, [0, 0])
    with pytest.raises(ValueError):
        tt.sample(u[:4, :2], w)
    ind, nul_d, nul_i = np.zeros((4, 3), np.int32), ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_int32)()
    fx = np.array([0, 8, 0], np.int32)
    assert L.ttx_sample(tt._h, 4, E._dp(u), nul_d, E._ip(fx), E._ip(ind), nul_d, nul_d) == EINVAL
    assert L.ttx_sample(tt._h, 4, nul_d, nul_d, nul_i, E._ip(ind), nul_d, nul_d) == EINVAL
    assert L.ttx_sample(tt._h, -1, E._dp(u), nul_d, nul_i, E._ip(ind), nul_d, nul_d) == EINVAL
    assert L.ttx_sample(tt._h, 4, E._dp(u), nul_d, nul_i, E._ip(ind), nul_d, nul_d) == 0       # logq and val may be NULL
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    u5, i5 = np.full((1, 5), 0.5), np.zeros((1, 5), np.int32)
    assert L.ttx_sample(fresh._h, 1, E._dp(u5), nul_d, nul_i, E._ip(i5), nul_d, nul_d) == ESTATE
    # a multi-process engine gets the answer ttx_ijk gives it (test_gpu_tijk_batch.py)
    mp = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"], nproc=2, world_rank=0, world_size=2)
    v = ctypes.c_double()
    want = L.ttx_ijk(mp._h, E._ip(np.ones((1, 5), np.int32)), ctypes.byref(v))
    assert want != 0 and L.ttx_sample(mp._h, 1, E._dp(u5), nul_d, nul_i, E._ip(i5), nul_d, nul_d) == want


def test_fortran_sample_val_is_tijk_of_its_indices():
    """the drop-in tt_lib: sample(tt, u, ind, logq=, val=) on a positive host train of rank 3, free and with mode 2 held at 3; val
    against the program's own tijk(tt, ind(:,p)) at 1e-12 of the element scale, the tolerance test_gpu_boundary.py uses for tijk"""
    from conftest import fortran_exe
    exe = fortran_exe("test_tt_sample")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("done"), p.stdout[-2000:] + p.stderr[-2000:]
    n = np.array([4, 5, 3, 6, 4])
    for tag in ("free", "held"):
        rows = np.array([[float(x) for x in ln.split()[1:]] for ln in p.stdout.splitlines() if ln.split() and ln.split()[0] == tag])
        assert rows.shape == (40, 9)
        ind = rows[:, 4:].astype(int)
        assert np.all(ind >= 1) and np.all(ind <= n[None, :]) and len({tuple(r) for r in ind}) > 10
        assert np.all(np.abs(rows[:, 1] - rows[:, 2]) <= 1e-12 * np.abs(rows[:, 2]).max())
        assert np.all(np.isfinite(rows[:, 3])) and np.all(rows[:, 3] < 0.0)
        if tag == "held":
            assert np.all(ind[:, 1] == 3)
