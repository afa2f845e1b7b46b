"""The forward Rosenblatt map of the squared interpolant on the device: ttx_rosenblatt_sq_real / ttx_rosenblatt_sq_real_dev (k_sqr_cdf,
ttcross_amd/csrc/ttx_sample_sq_real.h).

The sharpest check needs no reference: the sampler forms cell, hat values and log term from its rounded x, so the forward map at the
sampler's own x, in the same mode, must repeat logq and val byte for byte.  u is compared with tests/rosenblatt_ref.py along the same
x within the allowance derived in its docstring (tol_fwd over the total, plus 4 u), and with the uniforms the points were drawn from
within the sum of the sampler's allowance and that one; tests/test_rosenblatt_cpu.py shows that the reference alone meets both.
logq at points the sampler did not draw is compared within sample_sq_real_ref.verify's logq_bound.  Every case has 500 points."""
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

import rosenblatt_cases as RC
import rosenblatt_ref as F
import sample_sq_real_ref as Q
import sample_sq_ref as SQ
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

U = F.U
HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("exact", "mfma")
NAMES = ("u", "cell", "logq", "val")


@functools.lru_cache(maxsize=None)
def _engine(name, signed):
    return E.TTCross.from_cores(RC.case(name, signed)[0])


def _frozen(res):
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _drawn(name, signed, mode, gamma=0.0):
    """the sampler's result of a case: drawn once, shared, never modified"""
    cores, u, nodes = RC.case(name, signed)
    return _frozen(_engine(name, signed).sample_sq_real(u, nodes, gamma=gamma, mode=mode))


@functools.lru_cache(maxsize=None)
def _back(name, signed, mode, gamma=0.0):
    """the forward map at the sampler's own points, same mode"""
    cores, u, nodes = RC.case(name, signed)
    return _frozen(_engine(name, signed).rosenblatt_sq_real(_drawn(name, signed, mode, gamma)["x"], nodes, gamma=gamma, mode=mode))


@functools.lru_cache(maxsize=None)
def _walk(name, signed, mode, gamma=0.0):
    """the reference along the same points"""
    cores, u, nodes = RC.case(name, signed)
    return F.walk(cores, nodes, _drawn(name, signed, mode, gamma)["x"], None, gamma)


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in NAMES)


def _linear(nodes):
    return [("linear", t) for t in nodes]


def _against_reference(res, w, tag):
    """u, cell, logq of the device against walk's result w, within the bounds; the failed rows alike"""
    assert np.array_equal(np.isnan(res["u"][:, 0]), w["failed"]), tag
    ok = ~w["failed"]
    assert np.array_equal(res["cell"], w["cell"]), tag
    err, bound = np.abs(res["u"] - w["u"])[ok], F.u_bound(w)[ok]
    with np.errstate(invalid="ignore"):
        diff = np.where(res["logq"] == w["logq"], 0.0, np.abs(res["logq"] - w["logq"]))[ok]
    print(tag, "max |u - ref| / bound", float((err / bound).max()) if ok.any() else 0.0, "max |logq - ref| / bound",
          float((diff[diff > 0] / w["logq_bound"][ok][diff > 0]).max()) if (diff > 0).any() else 0.0)
    assert np.all(err <= bound), tag
    assert np.all(diff <= w["logq_bound"][ok]), tag
    assert np.array_equal(res["val"], w["val"]), tag


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,signed", RC.ALL, ids=RC.IDS)
def test_at_the_samplers_own_points(name, signed, mode):
    """ranks 1, 3, 4, 5, 15, 16, 17, 64, 65 and 128 and modes of 1, 2, 15, 16, 17, 31, 32, 64, 65, 130 and 1025 nodes (rosenblatt_cases.py)"""
    cores, u, nodes = RC.case(name, signed)
    tt, s, f, w = _engine(name, signed), _drawn(name, signed, mode), _back(name, signed, mode), _walk(name, signed, mode)
    assert not np.isnan(s["x"]).any()
    assert f["logq"].tobytes() == s["logq"].tobytes() and f["val"].tobytes() == s["val"].tobytes()
    for k, t in enumerate(nodes):
        if t.size == 1:
            assert np.all(f["u"][:, k] == 0.0) and np.all(f["cell"][:, k] == 0) and np.all(s["cell"][:, k] == 0)
            continue
        # on the right node of its cell x belongs to the next one, unless that cell is the last
        up = (s["x"][:, k] == t[np.minimum(s["cell"][:, k], t.size - 1)]) & (s["cell"][:, k] < t.size - 1)
        assert np.array_equal(f["cell"][:, k], s["cell"][:, k] + up)
    assert np.all(f["val"] == tt.basis_batch(s["x"], _linear(nodes), "exact"))
    _against_reference(f, w, f"{name} {mode}")
    drawn = np.array([t.size > 1 for t in nodes])
    err, bound = np.abs(f["u"] - np.minimum(u, 1.0))[:, drawn], F.u_bound(w, w["tol_inv"])[:, drawn]
    print("   max |u' - u|", float(err.max()), "in units of the combined allowance", float((err / bound).max()))
    assert np.all(err <= bound)


@functools.lru_cache(maxsize=None)
def _other_points(name, signed):
    """a seeded cloud in the box, every node itself, both ends of the box"""
    nodes = RC.case(name, signed)[2]
    nmax = max(t.size for t in nodes)
    x = np.concatenate([RC.cloud(nodes, 200, 23), np.array([[t[min(i, t.size - 1)] for t in nodes] for i in range(nmax)]),
                        np.array([[t[0] for t in nodes], [t[-1] for t in nodes]])])
    x.setflags(write=False)
    return x


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,signed", RC.ALL, ids=RC.IDS)
def test_at_points_the_sampler_did_not_draw(name, signed, mode):
    cores, _, nodes = RC.case(name, signed)
    tt, x = _engine(name, signed), _other_points(name, signed)
    res = tt.rosenblatt_sq_real(x, nodes, mode=mode)
    last = tt.rosenblatt_sq_real_last()
    assert last["failed"] == 0 and last["mode"] == mode
    w = F.walk(cores, nodes, x)
    _against_reference(res, w, f"{name} {mode}")
    assert np.all(res["val"] == tt.basis_batch(x, _linear(nodes), "exact"))
    drawn = np.array([t.size > 1 for t in nodes])
    # the ends of the box: nothing before the left one and nothing inside, so u = 0; at the right one the reference has u = 1, the device
    # C(n-3) + A(n-2) over C(n-2), which its wave scan associates otherwise
    assert np.all(res["u"][-2] == 0.0) and np.all(w["u"][-1, drawn] == 1.0)
    assert np.all(res["u"][-1, drawn] >= 1.0 - F.u_bound(w)[-1, drawn]) and np.all(res["u"][-1, drawn] <= 1.0)
    assert np.all(res["cell"][-2, drawn] == 1) and np.array_equal(res["cell"][-1, drawn], np.array([t.size - 1 for t in nodes])[drawn])


@pytest.mark.parametrize("mode", MODES)
def test_cells_without_mass(mode):
    """In the mode walked last a cell without mass is no failure: logq = -inf, u the running sum before it.  The trains are those of
    test_gpu_sample_sq_real.py's test_a_sign_change_inside_a_cell (also: the zeros of g inside a cell) and test_degenerate_trains."""
    a, b = np.array([-1.0, 1.0, 3.0, -3.0]), np.array([2.0, -2.0, 1.0])
    cores = [a.reshape(1, 4, 1), b.reshape(1, 3, 1)]
    nodes = [np.array([0.0, 1.0, 2.0, 4.0]), np.array([-1.0, 0.0, 2.0])]
    tt = E.TTCross.from_cores(cores)
    x = RC.cloud(nodes, 64, 3)
    x[0], x[1], x[2] = [0.5, 0.25], [3.0, 1.0], [0.75, -0.5]           # zeros of a at 0.5 and 3, of b at -0.5 and 2/3
    res = tt.rosenblatt_sq_real(x, nodes, mode=mode)
    assert tt.rosenblatt_sq_real_last()["failed"] == 1 and np.all(np.isnan(res["u"][2]))   # a zero of b in the mode walked first: no mass is left for mode 1
    _against_reference(res, F.walk(cores, nodes, x), "sign change " + mode)
    assert res["logq"][0] == -np.inf and res["logq"][1] == -np.inf and np.all(res["val"][:2] == 0.0)
    assert abs(res["u"][0, 0] - 1.0 / 64.0) <= 8.0 * U                  # int_0^0.5 (2x - 1)^2 dx = 1/6 of Z_1 = 32/3
    c3, _, n3 = RC.case("d3", False)
    ends = [c.copy() for c in c3]
    ends[0][:, :2, :] = 0.0
    ends[0][:, -2:, :] = 0.0                                            # only node 3 of 5 is left: cells 1 and 4 of mode 1 have no mass
    te = E.TTCross.from_cores(ends)
    xe = RC.cloud(n3, 40, 4)
    xe[:10, 0] = np.linspace(n3[0][0], n3[0][1], 10)
    xe[10:20, 0] = np.linspace(n3[0][3], n3[0][4], 10)
    xe[20:, 0] = np.linspace(n3[0][1], n3[0][3], 22)[1:-1]               # inside the two cells with mass
    res = te.rosenblatt_sq_real(xe, n3, mode=mode)
    assert te.rosenblatt_sq_real_last()["failed"] == 0
    _against_reference(res, F.walk(ends, n3, xe), "empty ends " + mode)
    assert np.all(res["logq"][:9] == -np.inf) and np.all(res["u"][:10, 0] == 0.0) and np.all(res["cell"][:9, 0] == 1)
    assert np.all(res["logq"][11:20] == -np.inf) and np.all(res["u"][10:20, 0] == 1.0) and np.all(res["cell"][10:20, 0] == 4)
    assert np.all(np.isfinite(res["logq"][20:]))
    # a massless cell in a mode walked before the last leaves a state of zeros: the next total is 0 and the point fails
    hole = [c.copy() for c in c3]
    hole[1][:, 2:4, :] = 0.0
    th = E.TTCross.from_cores(hole)
    xh = RC.cloud(n3, 20, 5)
    xh[:5, 1] = 0.5 * (n3[1][2] + n3[1][3])
    res = th.rosenblatt_sq_real(xh, n3, mode=mode)
    wh = F.walk(hole, n3, xh)                                           # the points of the cloud that fell into that cell fail too
    assert wh["failed"][:5].all() and not wh["failed"].all() and th.rosenblatt_sq_real_last()["failed"] == int(wh["failed"].sum())
    _against_reference(res, wh, "hole " + mode)
    zero = E.TTCross.from_cores([np.zeros_like(c) for c in c3])
    res = zero.rosenblatt_sq_real(xh, n3, mode=mode)
    assert zero.rosenblatt_sq_real_last()["failed"] == 20 and np.all(np.isnan(res["u"])) and np.all(res["cell"] == 0) and np.all(np.isnan(res["logq"])) and np.all(res["val"] == 0.0)
    res = zero.rosenblatt_sq_real(xh, n3, gamma=1.0, mode=mode)        # the defensive term alone: the uniform density, u = (x - t_0) / (t_(n-1) - t_0)
    assert zero.rosenblatt_sq_real_last()["failed"] == 0
    lin = np.stack([(xh[:, k] - t[0]) / (t[-1] - t[0]) for k, t in enumerate(n3)], axis=1)
    assert np.all(np.abs(res["u"] - lin) <= max(t.size for t in n3) * 8.0 * U)      # the n_k - 1 additions of the running sum, five operations per mass


@pytest.mark.parametrize("mode", MODES)
def test_u_is_monotone_along_a_coordinate(mode):
    """257 ascending points across every cell of the 17-node mode of tile_edges, the modes walked before it fixed"""
    cores, _, nodes = RC.case("tile_edges", True)
    tt = _engine("tile_edges", True)
    k = 3
    assert nodes[k].size == 17
    x = np.repeat(RC.cloud(nodes, 1, 9), 257, axis=0)
    x[:, k] = np.sort(np.concatenate([nodes[k], RC.cloud([nodes[k]], 240, 10)[:, 0]]))
    x[:, :k] = RC.cloud(nodes[:k], 257, 12)                             # the modes walked after it do not enter u_k
    res = tt.rosenblatt_sq_real(x, nodes, mode=mode)
    uk = res["u"][:, k]
    assert tt.rosenblatt_sq_real_last()["failed"] == 0 and len(set(res["cell"][:, k])) == 16
    assert uk[0] == 0.0 and uk[-1] <= 1.0 and np.all(np.diff(uk) >= 0.0)
    assert np.all(res["u"][:, k + 1:] == res["u"][0, k + 1:])


@pytest.mark.parametrize("mode", MODES)
def test_held_modes_and_a_defensive_term(mode):
    cores, u, nodes = RC.case("d6_size1_rank1", True)
    tt = _engine("d6_size1_rank1", True)
    cond = [np.nan, np.nan, float(nodes[2][3]), np.nan, 0.25 * float(nodes[4][1]) + 0.75 * float(nodes[4][2]), float(nodes[5][-1]) + 2.0]
    s = tt.sample_sq_real(u, nodes, cond, 0.125, mode)
    f = tt.rosenblatt_sq_real(s["x"], nodes, cond, 0.125, mode)
    assert tt.rosenblatt_sq_real_last()["failed"] == 0
    assert np.all(f["u"][:, 1:] == 0.0) and np.all(f["cell"][:, 1:] == 0) and np.all(f["cell"][:, 0] >= 1)
    assert f["logq"].tobytes() == s["logq"].tobytes() and f["val"].tobytes() == s["val"].tobytes()
    xn = s["x"].copy()
    xn[:, 1:] = np.nan                                                  # the x of a held mode is not looked at
    assert _same(tt.rosenblatt_sq_real(xn, nodes, cond, 0.125, mode), f)
    w = F.walk(cores, nodes, xn, cond, 0.125)
    _against_reference(f, w, "held " + mode)
    assert np.all(np.abs(f["u"][:, 0] - u[:, 0]) <= F.u_bound(w, w["tol_inv"])[:, 0])
    # exp(logq) (Z + gamma V) = val^2 + gamma with the device's own Z, at points the sampler did not draw
    c4, _, n4 = RC.case("tile_edges", True)
    t4 = _engine("tile_edges", True)
    mats = []
    for t in n4:
        dg, sp = E.mass_cholesky(t)
        mats.append(np.diag(dg) + np.diag(sp[:-1], 1))
    Z = t4.mode_apply(mats, "exact").norm() ** 2
    x4 = RC.cloud(n4, 300, 13)
    for gamma in (0.0, 0.125):
        res = t4.rosenblatt_sq_real(x4, n4, gamma=gamma, mode=mode)
        w4 = F.walk(c4, n4, x4, None, gamma)
        want = res["val"] * res["val"] + gamma
        rel = np.abs(np.exp(res["logq"]) * (Z + gamma * Q.volume(n4)) - want) / want
        bound = w4["logq_bound"] + 8.0 * w4["N"] * U                    # Z and V carry N u each against their true values, val^2 twice that
        print(mode, "gamma", gamma, "max rel / bound", float((rel / bound).max()))
        assert np.all(rel <= bound)
    # every mode held: nothing is walked, val is the interpolant at cond
    c3, _, n3 = RC.case("d3", True)
    t3 = _engine("d3", True)
    allheld = [0.5 * float(n3[0][0] + n3[0][1]), float(n3[1][0]) - 1.0, float(n3[2][2])]
    r = t3.rosenblatt_sq_real(np.full((5, 3), np.nan), n3, allheld, 0.25, mode)
    assert np.all(r["val"] == t3.basis_batch(np.array([allheld]), _linear(n3), "exact")[0]) and np.all(r["logq"] == 0.0) and np.all(r["cell"] == 0) and np.all(r["u"] == 0.0)


@pytest.mark.parametrize("mode", MODES)
def test_failed_points(mode):
    cores, _, nodes = RC.case("d3", True)
    tt = _engine("d3", True)
    x = RC.cloud(nodes, 40, 19)
    base = tt.rosenblatt_sq_real(x, nodes, mode=mode)
    assert tt.rosenblatt_sq_real_last()["failed"] == 0
    v = x.copy()
    v[3, 0], v[11, 1], v[17, 2], v[23, 1] = np.nan, np.inf, -np.inf, np.nextafter(nodes[1][-1], np.inf)
    v[29, 0], v[31, 2] = np.nextafter(nodes[0][0], -np.inf), np.nextafter(nodes[2][0], -np.inf)
    v[35, 0], v[36, 2] = nodes[0][-1], nodes[2][0]                      # on the ends of the box: inside
    bad = [3, 11, 17, 23, 29, 31]
    res = tt.rosenblatt_sq_real(v, nodes, mode=mode)
    assert tt.rosenblatt_sq_real_last()["failed"] == 6
    for s in bad:
        assert np.all(np.isnan(res["u"][s])) and np.all(res["cell"][s] == 0) and np.isnan(res["logq"][s]) and res["val"][s] == 0.0
    touched = np.zeros(40, bool)
    touched[bad + [35, 36]] = True
    assert all(res[k][~touched].tobytes() == base[k][~touched].tobytes() for k in NAMES)
    assert not np.isnan(res["u"][[35, 36]]).any() and res["cell"][35, 0] == nodes[0].size - 1 and res["cell"][36, 2] == 1 and res["u"][36, 2] == 0.0
    _against_reference(res, F.walk(cores, nodes, v), "failed " + mode)


def test_nan_and_inf_in_a_core_fail_every_row():
    """in a child process: the entry G_2(2, 5, 1) enters the factor F_2 and with it every row of mode 3, the mode walked first, so all
    200 points fail: whole rows of NaN, cell 0 (nothing outside 0 .. n_k - 1 is ever written), logq NaN, val 0, all counted"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "rosenblatt_worker.py"), "nan"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert sorted(r) == ["inf_exact", "inf_mfma", "nan_exact", "nan_mfma"]
    for v in r.values():
        assert v["in_range"] and v["whole_rows"] and v["marked"] and v["failed"] == v["counted"] == 200


@pytest.mark.parametrize("mode", MODES)
def test_point_counts_from_1_to_65_and_repetition(mode):
    cores, u, nodes = RC.case("tile_edges", True)
    tt, s, f = _engine("tile_edges", True), _drawn("tile_edges", True, mode), _back("tile_edges", True, mode)
    for m in range(1, 66):
        part = tt.rosenblatt_sq_real(s["x"][:m], nodes, mode=mode)
        assert all(part[k].tobytes() == f[k][:m].tobytes() for k in NAMES), m
    assert _same(tt.rosenblatt_sq_real(s["x"], nodes, mode=mode), f)
    perm = np.random.default_rng(1).permutation(u.shape[0])
    got = tt.rosenblatt_sq_real(s["x"][perm], nodes, mode=mode)
    assert all(got[k].tobytes() == f[k][perm].tobytes() for k in NAMES)
    only = tt.rosenblatt_sq_real(s["x"], nodes, mode=mode, want=("u", "logq"))
    assert sorted(only) == ["logq", "u"] and only["u"].tobytes() == f["u"].tobytes() and only["logq"].tobytes() == f["logq"].tobytes()
    assert _same(E.TTCross.from_cores(cores).rosenblatt_sq_real(s["x"], nodes, mode=mode), f)


@pytest.mark.parametrize("mode", MODES)
def test_the_chunk_size_does_not_enter(mode):
    """TTX_SAMPLE_CHUNK = 7 against the default, each in a fresh child process, and against this process"""
    base = dict(os.environ)
    base.pop("TTX_SAMPLE_CHUNK", None)
    out = []
    for chunk in (None, "7"):
        env = base if chunk is None else dict(base, TTX_SAMPLE_CHUNK=chunk)
        p = subprocess.run([sys.executable, os.path.join(HERE, "rosenblatt_worker.py"), "chunk", "long_modes", mode], capture_output=True, text=True, timeout=240, env=env)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        out.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert out[0]["digest"] == out[1]["digest"] and all(o["failed"] == 0 for o in out)
    res = _back("long_modes", True, mode, 0.125)
    assert out[0]["digest"] == hashlib.sha256(b"".join(res[k].tobytes() for k in NAMES)).hexdigest()


def test_device_entry_equals_the_host_entry():
    """torch tensors by data_ptr() through ttx_rosenblatt_sq_real_dev, in a child process (rosenblatt_worker.py says why)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "rosenblatt_worker.py"), "dev"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in MODES:
        m = r[mode]
        assert m["is_cuda"] and m["dtypes"] == ["torch.float64", "torch.int32", "torch.float64", "torch.float64"]
        assert m["equal"] and m["failed"] == 1 and m["only_u"] == ["u"] and m["empty"] == [0, 8]
    assert r["float32_refused"]


@pytest.mark.parametrize("mode", MODES)
def test_the_samplers_on_the_same_engine_are_unchanged_before_and_after(mode):
    cores, u, w = SQ.case("d8_unequal", True)
    u = u[:RC.NPTS]
    nodes = RC.case("d8_unequal", True)[2]
    tt = E.TTCross.from_cores(cores)
    sq0 = tt.sample_sq(u, w, gamma=0.125, mode=mode)
    re0 = tt.sample_sq_real(u, nodes, gamma=0.125, mode=mode)
    last0 = tt.sample_sq_real_last()
    f = tt.rosenblatt_sq_real(re0["x"], nodes, gamma=0.125, mode=mode)
    assert tt.sample_sq_real_last() == last0                            # a slot of its own
    assert f["logq"].tobytes() == re0["logq"].tobytes() and f["val"].tobytes() == re0["val"].tobytes()
    sq1 = tt.sample_sq(u, w, gamma=0.125, mode=mode)
    re1 = tt.sample_sq_real(u, nodes, gamma=0.125, mode=mode)
    assert all(sq0[k].tobytes() == sq1[k].tobytes() for k in ("ind", "logq", "val"))
    assert all(re0[k].tobytes() == re1[k].tobytes() for k in ("x", "cell", "logq", "val"))
    assert all(re0[k].tobytes() == _drawn("d8_unequal", True, mode, 0.125)[k].tobytes() for k in ("x", "cell", "logq", "val"))


def test_auto_and_last():
    cores, u, nodes = RC.case("d3", True)
    tt = _engine("d3", True)
    x = _drawn("d3", True, "exact")["x"]
    res = tt.rosenblatt_sq_real(x, nodes)                               # auto: 500 points of d3 lie far below the threshold
    last = tt.rosenblatt_sq_real_last()
    assert sorted(last) == ["failed", "flops", "mode", "ms_cdf", "ms_head", "ms_rows"]
    assert last["mode"] == "exact" and last["failed"] == 0 and last["flops"] == 500.0 * 2.0 * (5 * 1 * 3 + 7 * 3 * 2 + 4 * 2 * 1)
    assert last["ms_head"] > 0.0 and last["ms_rows"] > 0.0 and last["ms_cdf"] > 0.0
    assert _same(res, _back("d3", True, "exact"))
    assert E.TTCross.from_cores(cores).rosenblatt_sq_real_last()["mode"] is None


def test_refusals():
    L = E.load_library()
    cores, u, nodes = RC.case("d3", True)
    tt = _engine("d3", True)
    x = np.array(_drawn("d3", True, "exact")["x"])
    EINVAL, ESTATE = 1, 4
    empty = tt.rosenblatt_sq_real(np.zeros((0, 3)), nodes)
    assert empty["u"].shape == (0, 3) and empty["logq"].shape == (0,) and empty["cell"].shape == (0, 3)
    for k, bad in ((0, np.nan), (1, np.inf)):
        nb = [t.copy() for t in nodes]
        nb[k][2] = bad
        with pytest.raises(E.TTXError):
            tt.rosenblatt_sq_real(x[:4], nb)
    nb = [t.copy() for t in nodes]
    nb[2][1] = nb[2][0]                                                # not strictly ascending
    with pytest.raises(E.TTXError, match="ascending"):
        tt.rosenblatt_sq_real(x[:4], nb)
    with pytest.raises(E.TTXError, match="infinite"):
        tt.rosenblatt_sq_real(x[:4], nodes, [np.nan, np.inf, np.nan])
    with pytest.raises(E.TTXError, match="gamma"):
        tt.rosenblatt_sq_real(x[:4], nodes, gamma=-1.0)
    with pytest.raises(ValueError):
        tt.rosenblatt_sq_real(x[:4], nodes, mode="fast")
    with pytest.raises(ValueError):
        tt.rosenblatt_sq_real(x[:4], nodes, [0.0, 0.0])
    with pytest.raises(ValueError):
        tt.rosenblatt_sq_real(x[:4, :2], nodes)
    with pytest.raises(ValueError):
        tt.rosenblatt_sq_real(x[:4], nodes[:2])
    with pytest.raises(ValueError):
        tt.rosenblatt_sq_real(4, nodes)                                 # points, not a count
    with pytest.raises(ValueError):
        tt.rosenblatt_sq_real(x[:4], nodes, want=("x",))
    uo, nul_d, nul_i = np.zeros((4, 3)), ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_int32)()
    rowp = (ctypes.POINTER(ctypes.c_double) * 3)(*[E._dp(t) for t in nodes])
    au = E.EVAL_MODES["auto"]
    assert L.ttx_rosenblatt_sq_real(tt._h, 4, E._dp(x), rowp, nul_d, 0.0, au, E._dp(uo), nul_i, nul_d, nul_d) == 0     # cell, logq and val may be NULL
    assert np.array_equal(uo, _back("d3", True, "exact")["u"][:4])
    with pytest.raises(E.TTXError):                                    # ranks above 128, at creation or at the call
        big = [np.ones((1, 2, 129)), np.ones((129, 2, 1))]
        E.TTCross.from_cores(big).rosenblatt_sq_real(np.full((1, 2), 0.5), [np.arange(2.0)] * 2)
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    x5, u5 = np.full((1, 5), 0.5), np.zeros((1, 5))
    row5 = (ctypes.POINTER(ctypes.c_double) * 5)(*[E._dp(np.arange(9.0)) for _ in range(5)])
    assert L.ttx_rosenblatt_sq_real(fresh._h, 1, E._dp(x5), row5, nul_d, 0.0, au, E._dp(u5), nul_i, nul_d, nul_d) == ESTATE
    # a multi-process engine gets the answer ttx_ijk gives it (test_gpu_tijk_batch.py)
    mp = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"], nproc=2, world_rank=0, world_size=2)
    v = ctypes.c_double()
    want = L.ttx_ijk(mp._h, E._ip(np.ones((1, 5), np.int32)), ctypes.byref(v))
    assert want != 0 and L.ttx_rosenblatt_sq_real(mp._h, 1, E._dp(x5), row5, nul_d, 0.0, au, E._dp(u5), nul_i, nul_d, nul_d) == want


def test_fortran_rosenblatt_sq_real_maps_the_samplers_points_back():
    """the drop-in tt_lib: sample_sq_real, then rosenblatt_sq_real at its x, free and with mode 2 held at 0.3 (with a defensive term, exact
    mode).  The program prints whether logq and val repeated and the largest |u' - u|; its u' and x, printed with 17 digits, which
    round-trip, are checked here against the reference on the same train: the sum of three rank-1 trains"""
    from conftest import fortran_exe
    exe = fortran_exe("test_tt_rosenblatt_sq_real")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("done"), p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.split()]
    n, d, npts = [4, 5, 3, 6, 4], 5, 40
    parts = [[np.array([f(j, k) for j in range(1, n[k - 1] + 1)]) for k in range(1, d + 1)]
             for f in (lambda j, k: 0.25 * j - 0.1 * k - 0.4, lambda j, k: np.cos(0.7 * j + k), lambda j, k: np.sin(1.3 * j * k))]
    cores = []
    for k in range(d):
        c = np.zeros((1 if k == 0 else 3, n[k], 1 if k == d - 1 else 3))
        for q in range(3):
            c[0 if k == 0 else q, :, 0 if k == d - 1 else q] = parts[q][k]
        cores.append(c)
    nodes = [np.array([0.0 + (1.0 - 0.0) * float(j) / float(nk - 1) for j in range(nk)]) for nk in n]
    u = np.array([[(0.6180339887498949 * (pp + 7 * k) + 0.37 * pp * k) % 1.0 for k in range(1, d + 1)] for pp in range(1, npts + 1)])
    for tag, rows, cond, gamma in (("free", "fx", None, 0.0), ("held", "hx", [np.nan, 0.3, np.nan, np.nan, np.nan], 0.5)):
        v = [ln[1:] for ln in lines if ln[0] == tag]
        assert len(v) == 1 and v[0][1] == "T" and v[0][2] == "T" and int(v[0][3]) == 0, (tag, v)
        got = np.array([[float(t) for t in ln[2:]] for ln in lines if ln[0] == rows])
        assert got.shape == (npts, 2 * d)
        w = F.walk(cores, nodes, got[:, d:], cond, gamma)
        drawn = np.ones(d, bool) if cond is None else np.isnan(cond)
        assert not w["failed"].any() and np.all(got[:, :d][:, ~drawn] == 0.0)
        # the program's cores come from its own cos and sin and its u from its own mod: entries within an ulp of those here, which moves
        # every sum of products by less than d u B, far inside another N u Bc: the same allowance once more
        assert np.all(np.abs(got[:, :d] - w["u"])[:, drawn] <= 2.0 * F.u_bound(w)[:, drawn])
        err = np.abs(got[:, :d] - np.minimum(u, 1.0))[:, drawn]
        assert np.all(err <= 2.0 * F.u_bound(w, w["tol_inv"])[:, drawn])
        assert float(v[0][0]) <= float((2.0 * F.u_bound(w, w["tol_inv"])[:, drawn]).max())
