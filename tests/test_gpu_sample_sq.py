"""Samples drawn from the square of the resident train on the device: ttx_sample_sq / ttx_sample_sq_dev
(ttcross_amd/csrc/ttx_sample_sq.h).

The checker is tests/sample_sq_ref.py: verify walks every sample along the device's own indices and allows another index than the
reference's only where t lies within the derived allowance of an edge (its docstring has the derivation; tests/
test_sample_sq_cpu.py shows on the reference alone that the cap below is fair); at most 0.1 % of a test's samples may have such a
mode.  val must be tijk_batch(ind, "exact") bit for bit in both modes.  logq is compared with the reference's along the same
indices, within verify's logq_tol."""
import ctypes
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sample_ref as S
import sample_sq_ref as Q
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

U = S.U
HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("exact", "mfma")
ALL = [(k, s) for k in S.CASES for s in (False, True)] + [("edge_ranks", True)]
IDS = [k + ("_signed" if s else "") for k, s in ALL]
KEYS = ("ind", "logq", "val")


@functools.lru_cache(maxsize=None)
def _case(name, signed):
    return Q.edge_case() if name == "edge_ranks" else Q.case(name, signed)


@functools.lru_cache(maxsize=None)
def _engine(name, signed):
    return E.TTCross.from_cores(_case(name, signed)[0])


@functools.lru_cache(maxsize=None)
def _run(name, signed, mode, gamma=0.0):
    """the device result of a case: drawn once, shared, never modified"""
    cores, u, w = _case(name, signed)
    res = _engine(name, signed).sample_sq(u, w, gamma=gamma, mode=mode)
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _check(name, signed, mode, gamma=0.0):
    cores, u, w = _case(name, signed)
    return Q.verify(cores, u, w, None, gamma, _run(name, signed, mode, gamma)["ind"])


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in KEYS)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,signed", ALL, ids=IDS)
def test_indices_val_and_logq(name, signed, mode):
    """ranks 1, 3, 4, 5, 15, 16, 17, 64, 65 and 128 lie on the bonds of d8_unequal and edge_ranks, d6_size1_rank1 and edge_ranks have
    a mode of one index, above_lds_cap a mode above TTX_SM_LDSROW"""
    tt, res, chk = _engine(name, signed), _run(name, signed, mode), _check(name, signed, mode)
    print(name, "signed" if signed else "non-negative", mode, "N", chk["N"], "undecided", chk["undecided"], "of", S.NPTS)
    assert tt.sample_sq_last()["mode"] in MODES
    assert chk["undecided"] <= S.NPTS // 1000
    assert res["val"].tobytes() == tt.tijk_batch(res["ind"], "exact").tobytes()
    assert np.all(np.isfinite(res["logq"])) and np.all(res["logq"] <= 0.0)
    diff = np.abs(res["logq"] - chk["logq"])
    print("   max |logq - ref| / bound", float((diff / chk["logq_tol"]).max()))
    assert np.all(diff <= chk["logq_tol"])


@pytest.mark.parametrize("name,signed", ALL, ids=IDS)
def test_exact_and_mfma_agree_except_where_undecided(name, signed):
    cores, u, w = _case(name, signed)
    a, b = _run(name, signed, "exact"), _run(name, signed, "mfma")
    differ = np.any(a["ind"] != b["ind"], axis=1)
    assert not np.any(differ & ~(_check(name, signed, "exact")["mask"] | _check(name, signed, "mfma")["mask"]))
    same = ~differ
    assert a["val"][same].tobytes() == b["val"][same].tobytes()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gamma", [0.0, Q.CHI_GAMMA])
def test_dense_identity_and_chi_square_on_d3_signed(gamma, mode):
    cores, _, w = _case("d3", True)
    tt = _engine("d3", True)
    u = np.random.default_rng(Q.CHI_SEED).random((Q.CHI_NPTS, 3))
    res = tt.sample_sq(u, w, gamma=gamma, mode=mode)
    assert tt.sample_sq_last()["failed"] == 0 and tt.sample_sq_last()["mode"] == mode
    chk = Q.verify(cores, u, w, None, gamma, res["ind"])
    assert chk["undecided"] <= Q.CHI_NPTS // 1000
    full = Q.dense_density(cores, w, None, gamma)
    rho = full[tuple((res["ind"] - 1).T)].astype(np.float64)
    rel = np.abs(np.exp(res["logq"]) - rho) / rho
    print("gamma", gamma, mode, "max rel / bound", float((rel / (chk["logq_tol"] + 4.0 * U)).max()))
    assert np.all(rel <= chk["logq_tol"] + 4.0 * U)
    # exp(logq) (Z + gamma prod W) = (val^2 + gamma) prod w: the importance weight is bounded by Z + gamma prod W
    stat, q = Q.chi2(res["ind"], full.astype(np.float64)), Q.chi2_quantile(139)
    print("   chi-square", stat, "quantile", q)
    assert stat <= q


@pytest.mark.parametrize("mode", MODES)
def test_sample_counts_at_the_tile_edges(mode):
    cores, u, w = _case("d8_unequal", True)
    tt, res = _engine("d8_unequal", True), _run("d8_unequal", True, mode)
    for m in (1, 15, 16, 17, 63, 64, 65):
        part = tt.sample_sq(u[:m], w, mode=mode)
        assert all(part[k].tobytes() == res[k][:m].tobytes() for k in KEYS), m


@pytest.mark.parametrize("mode", MODES)
def test_fixed_modes(mode):
    cores, u, w = _case("d6_size1_rank1", True)
    tt = _engine("d6_size1_rank1", True)
    fixed = [0, 1, 0, 0, 3, 0]
    res = tt.sample_sq(u, w, fixed, 0.5, mode)
    assert np.all(res["ind"][:, 1] == 1) and np.all(res["ind"][:, 4] == 3)
    chk = Q.verify(cores, u, w, fixed, 0.5, res["ind"])
    assert chk["undecided"] <= S.NPTS // 1000
    assert res["val"].tobytes() == tt.tijk_batch(res["ind"], "exact").tobytes()
    assert np.all(np.abs(res["logq"] - chk["logq"]) <= chk["logq_tol"])
    # logq has no contribution from a fixed mode: the dense conditional density on d3 with mode 2 held
    c3, u3, w3 = _case("d3", True)
    t3, f3 = _engine("d3", True), [0, 4, 0]
    r3 = t3.sample_sq(u3, w3, f3, 0.0, mode)
    k3 = Q.verify(c3, u3, w3, f3, 0.0, r3["ind"])
    rho = Q.dense_density(c3, w3, f3)[r3["ind"][:, 0] - 1, 0, r3["ind"][:, 2] - 1].astype(np.float64)
    assert np.all(r3["ind"][:, 1] == 4)
    assert np.all(np.abs(np.exp(r3["logq"]) - rho) <= rho * (k3["logq_tol"] + 4.0 * U))
    u_nan = u3.copy()
    u_nan[:, 1] = np.nan                                               # the u of a fixed mode is not looked at
    assert _same(t3.sample_sq(u_nan, w3, f3, 0.0, mode), r3)


@pytest.mark.parametrize("mode", MODES)
def test_zero_weights_are_never_drawn(mode):
    cores, u, w = _case("long_modes", True)
    w = [q.copy() for q in w]
    w[0][::2] = 0.0
    w[1][5:100] = 0.0
    w[2][-1] = 0.0
    res = _engine("long_modes", True).sample_sq(u, w, mode=mode)
    assert np.all(res["ind"] > 0)
    assert np.all((res["ind"][:, 0] - 1) % 2 == 1) and not np.any((res["ind"][:, 1] >= 6) & (res["ind"][:, 1] <= 100)) and np.all(res["ind"][:, 2] < 64)
    assert Q.verify(cores, u, w, None, 0.0, res["ind"])["undecided"] <= S.NPTS // 1000


@pytest.mark.parametrize("mode", MODES)
def test_edges_of_u(mode):
    cores, u, w = _case("d3", True)
    tt, base = _engine("d3", True), _run("d3", True, mode)
    n = [c.shape[1] for c in cores]
    v = u[:40].copy()
    v[3], v[11], v[17] = 0.0, np.nextafter(1.0, 0.0), 1.0
    v[23, 1], v[29, 2] = np.nan, -0.5
    v[31, 0] = -0.0                                                    # counts as 0
    res = tt.sample_sq(v, w, mode=mode)
    assert tt.sample_sq_last()["failed"] == 2
    assert res["ind"][3].tolist() == [1, 1, 1] and res["ind"][11].tolist() == n and res["ind"][17].tolist() == n
    for s in (23, 29):
        assert np.all(res["ind"][s] == 0) and np.isnan(res["logq"][s]) and res["val"][s] == 0.0
    assert res["ind"][31, 0] == 1
    touched = np.zeros(40, bool)
    touched[[3, 11, 17, 23, 29, 31]] = True
    assert all(res[k][~touched].tobytes() == base[k][:40][~touched].tobytes() for k in KEYS)
    Q.verify(cores, v, w, None, 0.0, res["ind"])


def test_an_all_zero_train_fails_every_sample():
    cores, u, w = _case("d3", True)
    zero = E.TTCross.from_cores([np.zeros_like(c) for c in cores])
    for mode in MODES:
        res = zero.sample_sq(u[:500], w, mode=mode)
        assert zero.sample_sq_last()["failed"] == 500
        assert np.all(res["ind"] == 0) and np.all(np.isnan(res["logq"])) and np.all(res["val"] == 0.0)


def test_nan_and_inf_in_a_core_stay_in_range():
    """range safety, in a child process: every index written lies in 0 .. n_k, whole rows fail, the failed samples are counted"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "sample_sq_worker.py"), "nan"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert sorted(r) == ["inf_exact", "inf_mfma", "nan_exact", "nan_mfma"]
    for v in r.values():
        assert v["in_range"] and v["whole_rows"] and v["marked"] and v["failed"] == v["counted"] > 0


@pytest.mark.parametrize("mode", MODES)
def test_a_sample_does_not_depend_on_its_neighbours_or_on_the_call(mode):
    cores, u, w = _case("d8_unequal", True)
    tt, res = _engine("d8_unequal", True), _run("d8_unequal", True, mode)
    assert _same(tt.sample_sq(u, w, mode=mode), res)                   # repetition
    perm = np.random.default_rng(1).permutation(u.shape[0])
    got = tt.sample_sq(u[perm], w, mode=mode)
    assert all(got[k].tobytes() == res[k][perm].tobytes() for k in KEYS)
    t2 = E.TTCross.from_cores(cores)
    assert _same(t2.sample_sq(u, w, mode=mode), res)
    only = tt.sample_sq(u, w, mode=mode, want=("ind",))
    assert sorted(only) == ["ind"] and only["ind"].tobytes() == res["ind"].tobytes()
    byseed = tt.sample_sq(50, w, seed=5, mode=mode)
    assert _same(byseed, tt.sample_sq(np.random.default_rng(5).random((50, len(cores))), w, mode=mode))


@pytest.mark.parametrize("mode", MODES)
def test_the_chunk_size_does_not_enter(mode):
    """TTX_SAMPLE_CHUNK = 64 and 1000 against the default, each in a fresh child process"""
    base = dict(os.environ)
    base.pop("TTX_SAMPLE_CHUNK", None)
    out = []
    for chunk in (None, "64", "1000"):
        env = base if chunk is None else dict(base, TTX_SAMPLE_CHUNK=chunk)
        p = subprocess.run([sys.executable, os.path.join(HERE, "sample_sq_worker.py"), "chunk", "long_modes", mode], capture_output=True, text=True, timeout=240, env=env)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        out.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert out[0]["digest"] == out[1]["digest"] == out[2]["digest"] and all(o["failed"] == 0 for o in out)
    res = _run("long_modes", True, mode, 0.125)
    assert out[0]["digest"] == hashlib.sha256(res["ind"].tobytes() + res["logq"].tobytes() + res["val"].tobytes()).hexdigest()


def test_device_entry_equals_the_host_entry():
    """torch tensors by data_ptr() through ttx_sample_sq_dev, in a child process (sample_sq_worker.py says why)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "sample_sq_worker.py"), "dev"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in MODES:
        m = r[mode]
        assert m["is_cuda"] and m["dtypes"] == ["torch.int32", "torch.float64", "torch.float64"]
        assert m["equal"] and m["failed"] == 1 and m["only_ind"] == ["ind"] and m["chain"] and m["empty"] == [0, 8]
    assert r["float32_refused"]


@pytest.mark.parametrize("mode", MODES)
def test_a_long_train_stays_finite(mode):
    """d = 255: without the power-of-two scaling of the factors F overflows (the reference's exponents pass 1024)"""
    cores, u, w = Q.long_case()
    tt = E.TTCross.from_cores(cores)
    res = tt.sample_sq(u, w, mode=mode)
    assert tt.sample_sq_last()["failed"] == 0
    assert np.all(res["ind"] > 0) and np.all(np.isfinite(res["logq"])) and np.all(np.isfinite(res["val"])) and np.all(res["val"] != 0.0)
    assert max(Q.tables(cores, w, gram=False)["cum"]) > 1024
    chk = Q.verify(cores, u, w, None, 0.0, res["ind"], routes=True)    # routes: the float64 reference against long double
    assert chk["undecided"] <= 1 and chk["gap"] <= 0.25
    assert res["val"].tobytes() == tt.tijk_batch(res["ind"], "exact").tobytes()
    assert np.all(np.abs(res["logq"] - chk["logq"]) <= chk["logq_tol"])


def test_refused_by_hadamard_still_samplable():
    """rank 12 with sign changes: the square has rank 144 > 128 and hadamard refuses it; sample_sq draws from it all the same"""
    rng = np.random.default_rng(12)
    n, r = [6, 5, 7, 4], [1, 12, 12, 12, 1]
    cores = [rng.standard_normal((r[k], n[k], r[k + 1])) for k in range(4)]
    assert any((c < 0).any() and (c > 0).any() for c in cores)
    tt = E.TTCross.from_cores(cores)
    with pytest.raises(E.TTXError):
        tt.hadamard(tt)
    u = rng.random((S.NPTS, 4))
    for mode in MODES:
        res = tt.sample_sq(u, None, mode=mode)
        chk = Q.verify(cores, u, None, None, 0.0, res["ind"])
        assert tt.sample_sq_last()["failed"] == 0 and chk["undecided"] <= S.NPTS // 1000
        rho = Q.dense_density(cores)[tuple((res["ind"] - 1).T)].astype(np.float64)
        assert np.all(np.abs(np.exp(res["logq"]) - rho) <= rho * (chk["logq_tol"] + 4.0 * U))


def test_refusals():
    L = E.load_library()
    cores, u, w = _case("d3", True)
    tt = _engine("d3", True)
    EINVAL, ESTATE = 1, 4
    empty = tt.sample_sq(np.zeros((0, 3)), w)
    assert empty["ind"].shape == (0, 3) and empty["logq"].shape == (0,) and tt.sample_sq(0)["val"].shape == (0,)
    for bad in ([0, 8, 0], [-1, 0, 0], [0, 0, 5]):
        with pytest.raises(E.TTXError):
            tt.sample_sq(u[:4], w, bad)
    for j, v in ((0, -1e-300), (7, -1.0), (15, np.nan), (3, np.inf)):
        wb = np.concatenate(w)
        wb[j] = v
        with pytest.raises(E.TTXError, match="weight"):
            tt.sample_sq(u[:4], np.split(wb, [5, 12]))
    with pytest.raises(E.TTXError, match="gamma"):
        tt.sample_sq(u[:4], w, gamma=-1.0)
    with pytest.raises(ValueError):
        tt.sample_sq(u[:4], w, mode="fast")
    with pytest.raises(ValueError):
        tt.sample_sq(u[:4], w, [0, 0])
    with pytest.raises(ValueError):
        tt.sample_sq(u[:4, :2], w)
    ind, nul_d, nul_i = np.zeros((4, 3), np.int32), ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_int32)()
    au = E.EVAL_MODES["auto"]
    assert L.ttx_sample_sq(tt._h, 4, E._dp(u), nul_d, nul_i, 0.0, au, E._ip(ind), nul_d, nul_d) == 0       # logq and val may be NULL
    with pytest.raises(E.TTXError):                                    # ranks above 128, at creation or at the call
        big = [np.ones((1, 2, 129)), np.ones((129, 2, 1))]
        E.TTCross.from_cores(big).sample_sq(np.full((1, 2), 0.5))
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    u5, i5 = np.full((1, 5), 0.5), np.zeros((1, 5), np.int32)
    assert L.ttx_sample_sq(fresh._h, 1, E._dp(u5), nul_d, nul_i, 0.0, au, E._ip(i5), nul_d, nul_d) == ESTATE
    # a multi-process engine gets the answer ttx_ijk gives it (test_gpu_tijk_batch.py)
    mp = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"], nproc=2, world_rank=0, world_size=2)
    v = ctypes.c_double()
    want = L.ttx_ijk(mp._h, E._ip(np.ones((1, 5), np.int32)), ctypes.byref(v))
    assert want != 0 and L.ttx_sample_sq(mp._h, 1, E._dp(u5), nul_d, nul_i, 0.0, au, E._ip(i5), nul_d, nul_d) == want


def test_fortran_sample_sq_val_is_tijk_of_its_indices():
    """the drop-in tt_lib: sample_sq(tt, u, ind, logq=, val=) on a signed host train of rank 3, free and with mode 2 held at 3 (with a
    defensive term, exact mode); val against the program's own tijk(tt, ind(:,p)) at 1e-12 of the element scale, the tolerance
    test_gpu_boundary.py uses for tijk"""
    from conftest import fortran_exe
    exe = fortran_exe("test_tt_sample_sq")
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
    assert any(ln.split()[0] == "free" and float(ln.split()[2]) < 0.0 for ln in p.stdout.splitlines() if ln.split()) # the train is signed
