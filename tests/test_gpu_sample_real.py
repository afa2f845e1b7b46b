"""Real-valued samples from the interpolant of the resident train on the device: ttx_sample_real / ttx_sample_real_dev
(ttcross_amd/csrc/ttx_sample_real.h).

The checker is tests/sample_real_ref.py (numpy float64): verify walks every sample along the device's own x and checks, per drawn
mode, that x lies in its cell, that the cell has mass and that the reference's conditional CDF at x meets u C(n-2) within tol_k
(derived in its docstring; no allowance for undecided samples is needed in the CDF's domain).  val must equal basis_batch(x,
linear, "exact") element for element; logq is compared with the reference's along the same x within the bound of the same
docstring, and on trains without sign changes exp(logq) quad(trapezoid weights) with val."""
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

import sample_real_ref as SR
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

U = SR.U
HERE = os.path.dirname(os.path.abspath(__file__))
ALL = [(k, False) for k in SR.CASES] + [(k, True) for k in SR.SIGNED]
IDS = [k + ("_signed" if s else "") for k, s in ALL]
NAMES = ("x", "cell", "logq", "val")


@functools.lru_cache(maxsize=None)
def _run(name, signed=False):
    """(engine, cores, u, nodes, device result, the reference's check along the device's x) of a case: drawn once, shared, never modified"""
    cores, u, nodes = SR.case(name, signed)
    tt = E.TTCross.from_cores(cores)
    res = tt.sample_real(u, nodes)
    for v in res.values():
        v.setflags(write=False)
    return tt, cores, u, nodes, res


@functools.lru_cache(maxsize=None)
def _chk(name, signed=False):
    tt, cores, u, nodes, res = _run(name, signed)
    return SR.verify(cores, nodes, u, None, res["x"], res["cell"])


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in NAMES)


def _linear(nodes):
    return [("linear", t) for t in nodes]


@pytest.mark.parametrize("name,signed", ALL, ids=IDS)
def test_samples_invert_the_references_cdf_and_val_is_the_interpolant(name, signed):
    tt, cores, u, nodes, res = _run(name, signed)
    chk = _chk(name, signed)
    print(name, "signed" if signed else "non-negative", "N", chk["N"], "worst |CDF - T| / tol", chk["worst"])
    assert np.all(np.isfinite(res["val"]))
    assert np.all(res["val"] == tt.basis_batch(res["x"], _linear(nodes), "exact"))
    for k, t in enumerate(nodes):
        if t.size > 1:
            assert len(np.unique(res["x"][:, k])) > SR.NPTS // 2        # real points, not a lattice


@pytest.mark.parametrize("name,signed", ALL, ids=IDS)
def test_logq_is_the_references_along_the_devices_x(name, signed):
    tt, cores, u, nodes, res = _run(name, signed)
    chk = _chk(name, signed)
    with np.errstate(invalid="ignore"):
        diff = np.where(res["logq"] == chk["logq"], 0.0, np.abs(res["logq"] - chk["logq"]))     # -inf on both sides agrees
    print(name, "max |logq - ref| / bound", float(np.max(diff / chk["logq_bound"])))
    assert np.all(diff <= chk["logq_bound"])


@pytest.mark.parametrize("name", list(SR.CASES))
def test_exp_logq_times_quad_is_val_on_trains_without_sign_changes(name):
    tt, cores, u, nodes, res = _run(name)
    chk = _chk(name)
    z = tt.quad(E.trapezoid_weights(nodes))
    bound = chk["logq_bound"] + 4.0 * chk["N"] * U
    rel = np.abs(np.exp(res["logq"]) * z - res["val"]) / res["val"]
    print(name, "Z", z, "max |exp(logq) Z - val| / val", float(rel.max()), "bound", float(bound.min()))
    assert abs(z - chk["Z"]) <= 2.0 * chk["N"] * U * chk["Z"]
    assert np.all(res["val"] > 0.0) and np.all(rel <= bound)


def test_a_sample_does_not_depend_on_its_neighbours_or_on_the_call():
    tt, cores, u, nodes, res = _run("d8_unequal")
    assert _same(tt.sample_real(u, nodes), res)                        # repetition
    perm = np.random.default_rng(1).permutation(u.shape[0])
    got = tt.sample_real(u[perm], nodes)
    assert all(got[k].tobytes() == res[k][perm].tobytes() for k in res)
    dup = tt.sample_real(np.repeat(u[:300], 3, axis=0), nodes)
    assert all(dup[k].tobytes() == np.repeat(res[k][:300], 3, axis=0).tobytes() for k in res)
    for m in (1, 3, 4, 5):                                             # alone, and npts mod 4: the waves of the last workgroup
        part = tt.sample_real(u[:m], nodes)
        assert all(part[k].tobytes() == res[k][:m].tobytes() for k in res)
    alone = tt.sample_real(u[977:978], nodes)
    assert all(alone[k].tobytes() == res[k][977:978].tobytes() for k in res)
    t2 = E.TTCross.from_cores(cores)
    assert _same(t2.sample_real(u, nodes), res)
    only = tt.sample_real(u, nodes, want=("x",))
    assert sorted(only) == ["x"] and only["x"].tobytes() == res["x"].tobytes()
    byseed = tt.sample_real(50, nodes, seed=5)
    assert _same(byseed, tt.sample_real(np.random.default_rng(5).random((50, len(cores))), nodes))


def test_the_chunk_size_does_not_enter():
    """TTX_SAMPLE_CHUNK = 64 against the default, each in a fresh child process, and against this process"""
    base = dict(os.environ)
    base.pop("TTX_SAMPLE_CHUNK", None)
    out = []
    for chunk in (None, "64"):
        env = base if chunk is None else dict(base, TTX_SAMPLE_CHUNK=chunk)
        p = subprocess.run([sys.executable, os.path.join(HERE, "sample_real_worker.py"), "chunk", "long_modes"], capture_output=True, text=True, timeout=240, env=env)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        out.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert out[0]["digest"] == out[1]["digest"] and all(o["failed"] == 0 for o in out)
    res = _run("long_modes")[4]
    assert out[0]["digest"] == hashlib.sha256(b"".join(res[k].tobytes() for k in NAMES)).hexdigest()


def test_device_entry_equals_the_host_entry():
    """torch tensors by data_ptr() through ttx_sample_real_dev, in a child process (sample_real_worker.py says why)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "sample_real_worker.py"), "dev"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["is_cuda"] and r["dtypes"] == ["torch.float64", "torch.int32", "torch.float64", "torch.float64"]
    assert r["equal"] and r["failed"] == 1 and r["only_x"] == ["x"] and r["chain"] and r["empty"] == [0, 8] and r["float32_refused"]


def test_held_modes():
    tt, cores, u, nodes, _ = _run("d6_size1_rank1")
    # on a node, between nodes and outside the node range all count as held; modes 2 and 4 have one node
    cond = [np.nan, np.nan, float(nodes[2][3]), np.nan, 0.25 * float(nodes[4][1]) + 0.75 * float(nodes[4][2]), float(nodes[5][-1]) + 2.0]
    res = tt.sample_real(u, nodes, cond)
    for k in (2, 4, 5):
        assert np.all(res["x"][:, k] == cond[k]) and np.all(res["cell"][:, k] == 0)
    for k in (1, 3):
        assert np.all(res["x"][:, k] == nodes[k][0]) and np.all(res["cell"][:, k] == 0)
    assert np.all(res["cell"][:, 0] >= 1) and tt.sample_real_last()["failed"] == 0
    chk = SR.verify(cores, nodes, u, cond, res["x"], res["cell"])      # the reference with phi(cond) as weights
    assert np.all(res["val"] == tt.basis_batch(res["x"], _linear(nodes), "exact"))
    assert np.all(np.abs(res["logq"] - chk["logq"]) <= chk["logq_bound"])
    u_nan = u.copy()
    u_nan[:, [1, 2, 3, 4, 5]] = np.nan                                 # the u of a held mode is not looked at
    assert _same(tt.sample_real(u_nan, nodes, cond), res)
    # a held mode of one node may be given its coordinate: the hat row is (1) wherever it lies
    c1 = list(cond)
    c1[1] = 123.0
    r1 = tt.sample_real(u, nodes, c1)
    assert np.all(r1["x"][:, 1] == 123.0) and all(r1[k].tobytes() == res[k].tobytes() for k in ("cell", "logq", "val"))
    # every mode held: no draw, val is the interpolant at cond
    t3, c3, u3, n3, _ = _run("d3")
    allheld = [0.5 * float(n3[0][0] + n3[0][1]), float(n3[1][0]) - 1.0, float(n3[2][2])]
    r3 = t3.sample_real(u3[:5], n3, allheld)
    want = t3.basis_batch(np.array([allheld]), _linear(n3), "exact")[0]
    assert np.all(r3["val"] == want) and np.all(r3["logq"] == 0.0) and np.all(r3["cell"] == 0) and np.all(r3["x"] == np.array(allheld)[None, :])
    last = t3.sample_real_last()
    assert last["ms_head"] == 0.0 and last["bytes_head"] == 0.0 and last["failed"] == 0     # no head table was formed


def test_edges_of_u():
    tt, cores, u, nodes, base = _run("d3")
    lo, hi = [float(t[0]) for t in nodes], [float(t[-1]) for t in nodes]
    ncell = [t.size - 1 for t in nodes]
    v = u[:40].copy()
    v[3], v[11], v[17] = 0.0, np.nextafter(1.0, 0.0), 1.0
    v[23, 1], v[29, 2] = np.nan, -0.5
    v[31, 0] = -0.0                                                    # counts as 0
    res = tt.sample_real(v, nodes)
    assert tt.sample_real_last()["failed"] == 2
    assert res["x"][3].tolist() == lo and res["cell"][3].tolist() == [1, 1, 1]                 # the left end of the first cell with mass
    assert res["x"][17].tolist() == hi and res["cell"][17].tolist() == ncell                   # the right end of the last
    assert res["cell"][11].tolist() == ncell and np.all(res["x"][11] <= hi)
    for s in (23, 29):
        assert np.all(np.isnan(res["x"][s])) and np.all(res["cell"][s] == 0) and np.isnan(res["logq"][s]) and res["val"][s] == 0.0
    assert res["x"][31, 0] == lo[0] and res["cell"][31, 0] == 1
    touched = np.zeros(40, bool)
    touched[[3, 11, 17, 23, 29, 31]] = True
    assert all(res[k][~touched].tobytes() == base[k][:40][~touched].tobytes() for k in res)
    chk = SR.verify(cores, nodes, v, None, res["x"], res["cell"])
    # u = 1 - 2^-53: T = u C(n-2) is C(n-2) or the number before it, so x is the right end up to rounding.  In the last cell the density
    # is linear between its ends, at least pmin = min(p(n-2), p(n-1)) (positive on this train), so the mass to the right of x is at
    # least (t_end - x) pmin; it is also C(n-2) - CDF(x) <= |CDF(x) - T| + (C(n-2) - T) <= tol_k + 2 u C(n-2) (2^-53 C and T's rounding)
    pmin = chk["pend"][11].min(axis=1)
    assert np.all(pmin > 0.0) and np.all(np.array(hi) - res["x"][11] <= (chk["tol"][11] + 2.0 * U * chk["total"][11]) / pmin)
    print("u = 1 - 2^-53: (t_end - x) / bound", ((np.array(hi) - res["x"][11]) * pmin / (chk["tol"][11] + 2.0 * U * chk["total"][11])).tolist())
    fin = ~np.isnan(res["x"][:, 0])
    assert np.all(res["val"][fin] == tt.basis_batch(res["x"][fin], _linear(nodes), "exact"))


def test_degenerate_trains():
    cores, u, nodes = SR.case("d3")
    u = u[:500]
    zero = E.TTCross.from_cores([np.zeros_like(c) for c in cores])
    res = zero.sample_real(u, nodes)
    assert zero.sample_real_last()["failed"] == 500
    assert np.all(np.isnan(res["x"])) and np.all(res["cell"] == 0) and np.all(np.isnan(res["logq"])) and np.all(res["val"] == 0.0)
    hole = [c.copy() for c in cores]
    hole[1][:, 2:4, :] = 0.0                                           # G_2(:, 3, :) = G_2(:, 4, :) = 0: cell 3 of mode 2 has no mass and is never chosen
    th = E.TTCross.from_cores(hole)
    res = th.sample_real(u, nodes)
    assert th.sample_real_last()["failed"] == 0 and not np.any(res["cell"][:, 1] == 3) and set(res["cell"][:, 1]) == {1, 2, 4, 5, 6}
    SR.verify(hole, nodes, u, None, res["x"], res["cell"])
    edge = u.copy()
    edge[:, 0] = np.linspace(0.0, 1.0, 500)                            # u = 0 and u = 1 with the first and last cells empty, in the mode drawn last
    ends = [c.copy() for c in cores]
    ends[0][:, :2, :] = 0.0
    ends[0][:, -2:, :] = 0.0                                           # only node 3 of 5 is left: cells 2 and 3 have mass
    te = E.TTCross.from_cores(ends)
    res = te.sample_real(edge, nodes)
    assert te.sample_real_last()["failed"] == 0 and set(res["cell"][:, 0]) == {2, 3}
    assert res["x"][0, 0] == nodes[0][1] and res["x"][-1, 0] == nodes[0][3]
    assert res["val"][0] == 0.0 and res["logq"][0] == -np.inf          # the density vanishes at the end of its support
    SR.verify(ends, nodes, edge, None, res["x"], res["cell"])


def test_nan_and_inf_cores_return_with_cells_in_range():
    """in one child process, as sample_worker.py's"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "sample_real_worker.py"), "nonfinite"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    for tag in ("nan", "inf"):
        assert r[tag]["cells_in_range"] and r[tag]["failed_rows"] and r[tag]["others_drawn"] and r[tag]["nfailed"] == r[tag]["counted"] > 0


def test_refusals():
    L = E.load_library()
    tt, cores, u, nodes, _ = _run("d3")
    EINVAL, ESTATE = 1, 4
    empty = tt.sample_real(np.zeros((0, 3)), nodes)
    assert empty["x"].shape == (0, 3) and empty["cell"].shape == (0, 3) and empty["logq"].shape == (0,) and tt.sample_real(0, nodes)["val"].shape == (0,)
    desc, nanf, dup = [t.copy() for t in nodes], [t.copy() for t in nodes], [t.copy() for t in nodes]
    desc[1][3] = desc[1][2] - 0.1
    nanf[2][1] = np.nan
    dup[0][1] = dup[0][0]
    for bad in (desc, nanf, dup):
        with pytest.raises(E.TTXError):
            tt.sample_real(u[:4], bad)
    for bad in ([np.nan, np.inf, np.nan], [-np.inf, np.nan, np.nan]):
        with pytest.raises(E.TTXError):
            tt.sample_real(u[:4], nodes, bad)
    with pytest.raises(ValueError):
        tt.sample_real(u[:4], nodes[:2])
    with pytest.raises(ValueError):
        tt.sample_real(u[:4], [nodes[0], nodes[1], nodes[2][:-1]])
    with pytest.raises(ValueError):
        tt.sample_real(u[:4], nodes, [0.0, 0.0])
    with pytest.raises(ValueError):
        tt.sample_real(u[:4, :2], nodes)
    with pytest.raises(ValueError):
        tt.sample_real(u[:4], nodes, want=("ind",))
    x, cell = np.zeros((4, 3)), np.zeros((4, 3), np.int32)
    nul_d, nul_i, nul_r = ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.POINTER(ctypes.c_double))()
    rows = (ctypes.POINTER(ctypes.c_double) * 3)(*[E._dp(t) for t in nodes])
    norow = (ctypes.POINTER(ctypes.c_double) * 3)(E._dp(nodes[0]), nul_d, E._dp(nodes[2]))
    before = tt.sample_real_last()
    assert L.ttx_sample_real(tt._h, 4, nul_d, rows, nul_d, E._dp(x), E._ip(cell), nul_d, nul_d) == EINVAL
    assert L.ttx_sample_real(tt._h, 4, E._dp(u), rows, nul_d, nul_d, E._ip(cell), nul_d, nul_d) == EINVAL
    assert L.ttx_sample_real(tt._h, 4, E._dp(u), nul_r, nul_d, E._dp(x), E._ip(cell), nul_d, nul_d) == EINVAL
    assert L.ttx_sample_real(tt._h, -1, E._dp(u), rows, nul_d, E._dp(x), E._ip(cell), nul_d, nul_d) == EINVAL
    assert L.ttx_sample_real(tt._h, 4, E._dp(u), norow, nul_d, E._dp(x), E._ip(cell), nul_d, nul_d) == EINVAL
    assert tt.sample_real_last() == before                             # refused before the engine's figures were touched
    assert L.ttx_sample_real(tt._h, 4, E._dp(u), rows, nul_d, E._dp(x), nul_i, nul_d, nul_d) == 0      # cell, logq and val may be NULL
    assert x.tobytes() == _run("d3")[4]["x"][:4].tobytes()
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    u5, x5 = np.full((1, 5), 0.5), np.zeros((1, 5))
    t9 = np.linspace(0.0, 1.0, 9)
    rows5 = (ctypes.POINTER(ctypes.c_double) * 5)(*[E._dp(t9)] * 5)
    assert L.ttx_sample_real(fresh._h, 1, E._dp(u5), rows5, nul_d, E._dp(x5), nul_i, nul_d, nul_d) == ESTATE
    # a multi-process engine gets the answer ttx_ijk gives it (test_gpu_tijk_batch.py)
    mp = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"], nproc=2, world_rank=0, world_size=2)
    v = ctypes.c_double()
    want = L.ttx_ijk(mp._h, E._ip(np.ones((1, 5), np.int32)), ctypes.byref(v))
    assert want != 0 and L.ttx_sample_real(mp._h, 1, E._dp(u5), rows5, nul_d, E._dp(x5), nul_i, nul_d, nul_d) == want


def test_fortran_sample_real_val_is_the_basis_value_of_its_x():
    """the drop-in tt_lib: sample_real(tt, u, nodes, x, logq=, val=) on a positive host train of rank 3, free and with mode 2 held
    between two nodes; val must EQUAL the program's own basisval(tt, x, 2, 0, 1, .., mode = 0) -- ttx_basis_batch's exact chain on the
    same equidistant nodes, formed by the expression dtt_basisval uses; both are printed with 17 digits, which round-trip"""
    from conftest import fortran_exe
    exe = fortran_exe("test_tt_sample_real")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("done"), p.stdout[-2000:] + p.stderr[-2000:]
    for tag in ("free", "held"):
        rows = np.array([[float(v) for v in ln.split()[1:]] for ln in p.stdout.splitlines() if ln.split() and ln.split()[0] == tag])
        assert rows.shape == (40, 9)
        xs = rows[:, 4:]
        assert np.all(xs >= 0.0) and np.all(xs <= 1.0) and len({tuple(r) for r in xs}) == 40
        assert np.all(np.isfinite(rows[:, 1])) and np.all(rows[:, 1] > 0.0) and np.all(rows[:, 1] == rows[:, 2])
        assert np.all(np.isfinite(rows[:, 3]))
        if tag == "held":
            assert np.all(xs[:, 1] == 0.3)
