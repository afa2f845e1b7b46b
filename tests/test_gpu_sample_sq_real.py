"""Real-valued samples drawn from the square of the interpolant of the resident train on the device: ttx_sample_sq_real /
ttx_sample_sq_real_dev (ttcross_amd/csrc/ttx_sample_sq_real.h).

The checker is tests/sample_sq_real_ref.py: verify walks every sample along the device's own x in the domain of the conditional CDF,
within the allowance derived in its docstring (tests/test_sample_sq_real_cpu.py shows on the reference alone that its two routes
agree within a quarter of it); there is no undecided allowance.  val must equal basis_batch(x, linear, "exact") element for element
in both modes.  logq is compared with the reference's along the same x within verify's logq_bound, and the identity
exp(logq) (Z + gamma V) = val^2 + gamma is checked with Z formed on the device and, on d3, from the dense tensor."""
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
import sample_sq_real_ref as Q
import sample_sq_ref as SQ
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

U = S.U
HERE = os.path.dirname(os.path.abspath(__file__))
MODES = ("exact", "mfma")
NAMES = ("x", "cell", "logq", "val")
ALL = [(k, s) for k in S.CASES for s in (False, True)] + [("edge_ranks", True), ("tile_edges", True)]
IDS = [k + ("_signed" if s else "") for k, s in ALL]
# modes of 2 (one cell), 15, 16, 17, 31 and 32 nodes: one tile of 15 cells exactly, one cell more, two tiles exactly, one more; bonds 4, 5, 16, 17
TILE_EDGES = ([2, 15, 16, 17, 31, 32], [1, 4, 5, 16, 17, 3, 1])


def _nodes(n, seed):
    rng = np.random.default_rng(seed)
    return [np.cumsum(rng.uniform(0.2, 1.0, nk)) - rng.uniform(0.0, 3.0) for nk in n]


@functools.lru_cache(maxsize=None)
def _case(name, signed):
    if name == "edge_ranks":                                            # sample_sq_ref's train with the bonds 4, 5, 15, 16 and a mode of one node
        cores, u, _ = SQ.edge_case()
        return cores, u, _nodes(SQ.EDGE_RANKS[0], 4517)
    if name == "tile_edges":
        n, r = TILE_EDGES
        rng = np.random.default_rng(1516)
        return [rng.standard_normal((r[k], n[k], r[k + 1])) for k in range(len(n))], rng.random((S.NPTS, len(n))), _nodes(n, 1517)
    return Q.case(name, signed)


@functools.lru_cache(maxsize=None)
def _engine(name, signed):
    return E.TTCross.from_cores(_case(name, signed)[0])


@functools.lru_cache(maxsize=None)
def _run(name, signed, mode, gamma=0.0):
    """the device result of a case: drawn once, shared, never modified"""
    cores, u, nodes = _case(name, signed)
    res = _engine(name, signed).sample_sq_real(u, nodes, gamma=gamma, mode=mode)
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _check(name, signed, mode, gamma=0.0):
    cores, u, nodes = _case(name, signed)
    res = _run(name, signed, mode, gamma)
    return Q.verify(cores, nodes, u, None, gamma, res["x"], res["cell"])


def _same(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in NAMES)


def _linear(nodes):
    return [("linear", t) for t in nodes]


def _device_Z(tt, nodes):
    """||mode_apply(U_k) train||^2 on the device: the integral of the squared interpolant over the box"""
    mats = []
    for t in nodes:
        dg, sp = E.mass_cholesky(t)
        mats.append(np.diag(dg) + np.diag(sp[:-1], 1))
    return tt.mode_apply(mats, "exact").norm() ** 2


def _identity(res, chk, ZV, gamma):
    want = res["val"] * res["val"] + gamma
    rel = np.abs(np.exp(res["logq"]) * ZV - want) / want
    bound = chk["logq_bound"] + 8.0 * chk["N"] * U                      # Z and V carry N u each against their true values, val^2 twice that
    return rel, bound


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,signed", ALL, ids=IDS)
def test_samples_val_and_logq(name, signed, mode):
    """ranks 1, 3, 4, 5, 15, 16, 17, 64, 65 and 128 lie on the bonds of d8_unequal, edge_ranks and tile_edges; modes of 1, 2, 15, 16, 17,
    31, 32, 64, 65, 130 and 1025 nodes in tile_edges, long_modes, above_lds_cap and d6_size1_rank1"""
    cores, u, nodes = _case(name, signed)
    tt, res, chk = _engine(name, signed), _run(name, signed, mode), _check(name, signed, mode)
    print(name, "signed" if signed else "non-negative", mode, "N", chk["N"], "worst |CDF - T| / tol", chk["worst"])
    assert tt.sample_sq_real_last()["mode"] in MODES
    assert np.all(np.isfinite(res["val"]))
    assert np.all(res["val"] == tt.basis_batch(res["x"], _linear(nodes), "exact"))
    assert np.array_equal(res["val"], chk["val"])
    for k, t in enumerate(nodes):
        if t.size > 1:
            assert len(np.unique(res["x"][:, k])) > S.NPTS // 2         # real points, not a lattice
    with np.errstate(invalid="ignore"):
        diff = np.where(res["logq"] == chk["logq"], 0.0, np.abs(res["logq"] - chk["logq"]))
    print("   max |logq - ref| / bound", float((diff / chk["logq_bound"]).max()))
    assert np.all(diff <= chk["logq_bound"])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,signed", [("d3", True), ("d8_unequal", True), ("long_modes", False), ("tile_edges", True)])
def test_identity_with_the_devices_own_Z(name, signed, mode):
    cores, u, nodes = _case(name, signed)
    tt = _engine(name, signed)
    Z = _device_Z(tt, nodes)
    for gamma in (0.0, 0.125):
        res, chk = _run(name, signed, mode, gamma), _check(name, signed, mode, gamma)
        rel, bound = _identity(res, chk, Z + gamma * Q.volume(nodes), gamma)
        print(name, mode, "gamma", gamma, "Z", Z, "max rel / bound", float((rel / bound).max()))
        assert np.all(rel <= bound)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gamma", [0.0, Q.CHI_GAMMA])
def test_dense_identity_and_chi_square_on_d3_signed(gamma, mode):
    cores, _, nodes = _case("d3", True)
    tt = _engine("d3", True)
    u = np.random.default_rng(Q.CHI_SEED).random((Q.CHI_NPTS, 3))
    res = tt.sample_sq_real(u, nodes, gamma=gamma, mode=mode)
    assert tt.sample_sq_real_last()["failed"] == 0 and tt.sample_sq_real_last()["mode"] == mode
    chk = Q.verify(cores, nodes, u, None, gamma, res["x"], res["cell"])
    Zd = float(Q.dense_Z(cores, nodes))
    assert abs(_device_Z(tt, nodes) - Zd) <= 4.0 * chk["N"] * U * Zd
    rel, bound = _identity(res, chk, Zd + gamma * Q.volume(nodes), gamma)
    print("gamma", gamma, mode, "max rel / bound", float((rel / bound).max()))
    assert np.all(rel <= bound)
    rho = Q.dense_cell_masses(cores, nodes, gamma).astype(np.float64)
    stat, q = Q.chi2(res["cell"], rho), Q.chi2_quantile(71)
    print("   chi-square", stat, "quantile", q)
    assert stat <= q


@pytest.mark.parametrize("mode", MODES)
def test_sample_counts_from_1_to_65(mode):
    cores, u, nodes = _case("tile_edges", True)
    tt, res = _engine("tile_edges", True), _run("tile_edges", True, mode)
    for m in range(1, 66):
        part = tt.sample_sq_real(u[:m], nodes, mode=mode)
        assert all(part[k].tobytes() == res[k][:m].tobytes() for k in NAMES), m


@pytest.mark.parametrize("mode", MODES)
def test_held_modes_with_a_defensive_term(mode):
    cores, u, nodes = _case("d6_size1_rank1", True)
    tt = _engine("d6_size1_rank1", True)
    # on a node, between nodes and outside the node range all count as held; modes 2 and 4 have one node
    cond = [np.nan, np.nan, float(nodes[2][3]), np.nan, 0.25 * float(nodes[4][1]) + 0.75 * float(nodes[4][2]), float(nodes[5][-1]) + 2.0]
    res = tt.sample_sq_real(u, nodes, cond, 0.5, mode)
    for k in (2, 4, 5):
        assert np.all(res["x"][:, k] == cond[k]) and np.all(res["cell"][:, k] == 0)
    for k in (1, 3):
        assert np.all(res["x"][:, k] == nodes[k][0]) and np.all(res["cell"][:, k] == 0)
    assert np.all(res["cell"][:, 0] >= 1) and tt.sample_sq_real_last()["failed"] == 0
    chk = Q.verify(cores, nodes, u, cond, 0.5, res["x"], res["cell"])
    assert np.all(res["val"] == tt.basis_batch(res["x"], _linear(nodes), "exact"))
    assert np.all(np.abs(res["logq"] - chk["logq"]) <= chk["logq_bound"])
    u_nan = u.copy()
    u_nan[:, [1, 2, 3, 4, 5]] = np.nan                                 # the u of a held mode is not looked at
    assert _same(tt.sample_sq_real(u_nan, nodes, cond, 0.5, mode), res)
    c1 = list(cond)
    c1[1] = 123.0                                                      # a mode of one node may be given its coordinate: the hat row is (1)
    r1 = tt.sample_sq_real(u, nodes, c1, 0.5, mode)
    assert np.all(r1["x"][:, 1] == 123.0) and all(r1[k].tobytes() == res[k].tobytes() for k in ("cell", "logq", "val"))
    # the conditional density of mode 1 alone, given the others: its integral over the box of mode 1 is 1 (the identity with Z + gamma V
    # of the held train, here from the reference's dense route: d3 with mode 2 held between two nodes)
    c3, u3, n3 = _case("d3", True)
    t3 = _engine("d3", True)
    cd = [np.nan, 0.3 * float(n3[1][2]) + 0.7 * float(n3[1][3]), np.nan]
    r3 = t3.sample_sq_real(u3, n3, cd, 0.25, mode)
    k3 = Q.verify(c3, n3, u3, cd, 0.25, r3["x"], r3["cell"])
    row = Q.R.hat_row(n3[1], cd[1])
    held = [c3[0], np.einsum("i,aib->ab", row, c3[1])[:, None, :], c3[2]]
    dense = S.dense(held)[:, 0, :].astype(np.longdouble)
    Z = float(np.einsum("ij,ik,jl,kl->", dense, Q.mass_matrix(n3[0]), Q.mass_matrix(n3[2]), dense))
    rel, bound = _identity(r3, k3, Z + 0.25 * float((n3[0][-1] - n3[0][0]) * (n3[2][-1] - n3[2][0])), 0.25)
    assert np.all(rel <= bound)
    # every mode held: no draw, val is the interpolant at cond
    allheld = [0.5 * float(n3[0][0] + n3[0][1]), float(n3[1][0]) - 1.0, float(n3[2][2])]
    r4 = t3.sample_sq_real(u3[:5], n3, allheld, 0.25, mode)
    want = t3.basis_batch(np.array([allheld]), _linear(n3), "exact")[0]
    assert np.all(r4["val"] == want) and np.all(r4["logq"] == 0.0) and np.all(r4["cell"] == 0) and np.all(r4["x"] == np.array(allheld)[None, :])


@pytest.mark.parametrize("mode", MODES)
def test_a_sign_change_inside_a_cell(mode):
    """rank 1, d = 2: g(x, y) = a(x) b(y) with a = (-1, 1, 3, -3) on the nodes 0, 1, 2, 4: a changes sign at x = 0.5 and x = 3 exactly,
    inside cells 1 and 3, where the conditional touches zero and its CDF is flat.  b = (2, -2, 1) likewise."""
    a, b = np.array([-1.0, 1.0, 3.0, -3.0]), np.array([2.0, -2.0, 1.0])
    cores = [a.reshape(1, 4, 1), b.reshape(1, 3, 1)]
    nodes = [np.array([0.0, 1.0, 2.0, 4.0]), np.array([-1.0, 0.0, 2.0])]
    tt = E.TTCross.from_cores(cores)
    u = np.random.default_rng(31).random((S.NPTS, 2))
    u[:64, 0] = np.linspace(0.0, 1.0, 64)
    # the zero of the conditional of mode 1 at x = 0.5 carries the mass of half the first cell: int_0^0.5 (2x - 1)^2 dx = 1/6, and Z_1 = 32/3: u = 1/64
    Z1 = 1.0 / 3.0 + (1.0 + 3.0 + 9.0) / 3.0 + 2.0 * (9.0 - 9.0 + 9.0) / 3.0
    u[64, 0], u[65, 0] = (1.0 / 6.0) / Z1, np.nextafter((1.0 / 6.0) / Z1, 1.0)
    res = tt.sample_sq_real(u, nodes, mode=mode)
    assert tt.sample_sq_real_last()["failed"] == 0
    chk = Q.verify(cores, nodes, u, None, 0.0, res["x"], res["cell"])
    print(mode, "worst |CDF - T| / tol", chk["worst"], "x at the zero", res["x"][64, 0], res["x"][65, 0])
    assert np.all(res["val"] == tt.basis_batch(res["x"], _linear(nodes), "exact"))
    with np.errstate(invalid="ignore"):
        diff = np.where(res["logq"] == chk["logq"], 0.0, np.abs(res["logq"] - chk["logq"]))
    assert np.all(diff <= chk["logq_bound"])
    Z = float(Q.dense_Z(cores, nodes))
    fin = np.isfinite(res["logq"])                                     # logq = -inf exactly on a zero of g
    rel, bound = _identity({k: res[k][fin] for k in NAMES}, {"logq_bound": chk["logq_bound"][fin], "N": chk["N"]}, Z, 0.0)
    assert fin.sum() >= S.NPTS - 2 and np.all(rel <= bound)
    assert abs(Z1 - 32.0 / 3.0) < 1e-14 and res["cell"][64, 0] in (1, 2) and 0.0 <= res["x"][64, 0] <= 1.0


@pytest.mark.parametrize("mode", MODES)
def test_edges_of_u(mode):
    cores, u, nodes = _case("d3", True)
    tt, base = _engine("d3", True), _run("d3", True, mode)
    lo, hi = [float(t[0]) for t in nodes], [float(t[-1]) for t in nodes]
    ncell = [t.size - 1 for t in nodes]
    v = u[:40].copy()
    v[3], v[11], v[17] = 0.0, np.nextafter(1.0, 0.0), 1.0
    v[23, 1], v[29, 2] = np.nan, -0.5
    v[31, 0] = -0.0                                                    # counts as 0
    res = tt.sample_sq_real(v, nodes, mode=mode)
    assert tt.sample_sq_real_last()["failed"] == 2
    assert res["x"][3].tolist() == lo and res["cell"][3].tolist() == [1, 1, 1]                 # the left end of the first cell with mass
    assert res["x"][17].tolist() == hi and res["cell"][17].tolist() == ncell                   # the right end of the last
    assert res["cell"][11].tolist() == ncell and np.all(res["x"][11] <= hi)
    for s in (23, 29):
        assert np.all(np.isnan(res["x"][s])) and np.all(res["cell"][s] == 0) and np.isnan(res["logq"][s]) and res["val"][s] == 0.0
    assert res["x"][31, 0] == lo[0] and res["cell"][31, 0] == 1
    touched = np.zeros(40, bool)
    touched[[3, 11, 17, 23, 29, 31]] = True
    assert all(res[k][~touched].tobytes() == base[k][:40][~touched].tobytes() for k in NAMES)
    Q.verify(cores, nodes, v, None, 0.0, res["x"], res["cell"])
    fin = ~np.isnan(res["x"][:, 0])
    assert np.all(res["val"][fin] == tt.basis_batch(res["x"][fin], _linear(nodes), "exact"))


@pytest.mark.parametrize("mode", MODES)
def test_degenerate_trains(mode):
    cores, u, nodes = _case("d3", False)
    u = u[:500]
    zero = E.TTCross.from_cores([np.zeros_like(c) for c in cores])
    res = zero.sample_sq_real(u, nodes, mode=mode)
    assert zero.sample_sq_real_last()["failed"] == 500
    assert np.all(np.isnan(res["x"])) and np.all(res["cell"] == 0) and np.all(np.isnan(res["logq"])) and np.all(res["val"] == 0.0)
    res = zero.sample_sq_real(u, nodes, gamma=1.0, mode=mode)          # the defensive term alone: the uniform density on the box
    assert zero.sample_sq_real_last()["failed"] == 0 and np.all(res["val"] == 0.0)
    # per mode the ratio g / C(n-2) carries the n_k - 1 additions of the running sum and the five operations of a cell mass, the
    # division and the log four more relative to 1 + |term|
    logL = [abs(np.log(t[-1] - t[0])) for t in nodes]
    assert np.all(np.abs(res["logq"] + np.log(Q.volume(nodes))) <= sum((t.size + 8) * U + 8.0 * U * (1.0 + l) for t, l in zip(nodes, logL)))
    hole = [c.copy() for c in cores]
    hole[1][:, 2:4, :] = 0.0                                           # G_2(:, 3, :) = G_2(:, 4, :) = 0: cell 3 of mode 2 has no mass and is never chosen
    th = E.TTCross.from_cores(hole)
    res = th.sample_sq_real(u, nodes, mode=mode)
    assert th.sample_sq_real_last()["failed"] == 0 and not np.any(res["cell"][:, 1] == 3) and set(res["cell"][:, 1]) == {1, 2, 4, 5, 6}
    Q.verify(hole, nodes, u, None, 0.0, res["x"], res["cell"])
    edge = u.copy()
    edge[:, 0] = np.linspace(0.0, 1.0, 500)                            # u = 0 and u = 1 with the first and last cells empty, in the mode drawn last
    ends = [c.copy() for c in cores]
    ends[0][:, :2, :] = 0.0
    ends[0][:, -2:, :] = 0.0                                           # only node 3 of 5 is left: cells 2 and 3 have mass
    te = E.TTCross.from_cores(ends)
    res = te.sample_sq_real(edge, nodes, mode=mode)
    assert te.sample_sq_real_last()["failed"] == 0 and set(res["cell"][:, 0]) == {2, 3}
    assert res["x"][0, 0] == nodes[0][1] and res["x"][-1, 0] == nodes[0][3]


def test_nan_and_inf_in_a_core_stay_in_range():
    """range safety, in a child process: every cell written lies in 0 .. n_k - 1 and every x in its box, whole rows fail, the failed
    samples are counted"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "sample_sq_real_worker.py"), "nan"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert sorted(r) == ["inf_exact", "inf_mfma", "nan_exact", "nan_mfma"]
    for v in r.values():
        assert v["in_range"] and v["whole_rows"] and v["marked"] and v["failed"] == v["counted"] > 0


@pytest.mark.parametrize("mode", MODES)
def test_a_sample_does_not_depend_on_its_neighbours_or_on_the_call(mode):
    cores, u, nodes = _case("d8_unequal", True)
    tt, res = _engine("d8_unequal", True), _run("d8_unequal", True, mode)
    assert _same(tt.sample_sq_real(u, nodes, mode=mode), res)          # repetition
    perm = np.random.default_rng(1).permutation(u.shape[0])
    got = tt.sample_sq_real(u[perm], nodes, mode=mode)
    assert all(got[k].tobytes() == res[k][perm].tobytes() for k in NAMES)
    dup = tt.sample_sq_real(np.repeat(u[:300], 3, axis=0), nodes, mode=mode)
    assert all(dup[k].tobytes() == np.repeat(res[k][:300], 3, axis=0).tobytes() for k in NAMES)
    alone = tt.sample_sq_real(u[977:978], nodes, mode=mode)
    assert all(alone[k].tobytes() == res[k][977:978].tobytes() for k in NAMES)
    t2 = E.TTCross.from_cores(cores)
    assert _same(t2.sample_sq_real(u, nodes, mode=mode), res)
    only = tt.sample_sq_real(u, nodes, mode=mode, want=("x",))
    assert sorted(only) == ["x"] and only["x"].tobytes() == res["x"].tobytes()
    byseed = tt.sample_sq_real(50, nodes, seed=5, mode=mode)
    assert _same(byseed, tt.sample_sq_real(np.random.default_rng(5).random((50, len(cores))), nodes, mode=mode))


@pytest.mark.parametrize("mode", MODES)
def test_the_chunk_size_does_not_enter(mode):
    """TTX_SAMPLE_CHUNK = 64 against the default, each in a fresh child process, and against this process"""
    base = dict(os.environ)
    base.pop("TTX_SAMPLE_CHUNK", None)
    out = []
    for chunk in (None, "64"):
        env = base if chunk is None else dict(base, TTX_SAMPLE_CHUNK=chunk)
        p = subprocess.run([sys.executable, os.path.join(HERE, "sample_sq_real_worker.py"), "chunk", "long_modes", mode], capture_output=True, text=True, timeout=240, env=env)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
        out.append(json.loads(p.stdout.strip().splitlines()[-1]))
    assert out[0]["digest"] == out[1]["digest"] and all(o["failed"] == 0 for o in out)
    res = _run("long_modes", True, mode, 0.125)
    assert out[0]["digest"] == hashlib.sha256(b"".join(res[k].tobytes() for k in NAMES)).hexdigest()


def test_device_entry_equals_the_host_entry():
    """torch tensors by data_ptr() through ttx_sample_sq_real_dev, in a child process (sample_sq_real_worker.py says why)"""
    p = subprocess.run([sys.executable, os.path.join(HERE, "sample_sq_real_worker.py"), "dev"], capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    for mode in MODES:
        m = r[mode]
        assert m["is_cuda"] and m["dtypes"] == ["torch.float64", "torch.int32", "torch.float64", "torch.float64"]
        assert m["equal"] and m["failed"] == 1 and m["only_x"] == ["x"] and m["chain"] and m["empty"] == [0, 8]
    assert r["float32_refused"]


LONG_H = 3.0e4


@functools.lru_cache(maxsize=None)
def _long_case():
    """sample_sq_ref.long_case's d = 255 train; the weights of size 1e4 of its first 60 modes become node spacings of 3e4 (the mass
    matrix's entries are h / 3 and h / 6), so an unscaled factor would pass 1e308 as it does there"""
    cores, u, _ = SQ.long_case()
    rng = np.random.default_rng(256)
    nodes = [np.cumsum(rng.uniform(0.5, 1.5, 3)) * (LONG_H if k < SQ.LONG_BIG else 1.0) for k in range(len(cores))]
    return cores, u, nodes


@pytest.mark.parametrize("mode", MODES)
def test_a_long_train_stays_finite(mode):
    cores, u, nodes = _long_case()
    tt = E.TTCross.from_cores(cores)
    res = tt.sample_sq_real(u, nodes, mode=mode)
    assert tt.sample_sq_real_last()["failed"] == 0
    assert np.all(res["cell"] > 0) and np.all(np.isfinite(res["x"])) and np.all(np.isfinite(res["logq"])) and np.all(np.isfinite(res["val"])) and np.all(res["val"] != 0.0)
    assert max(Q.tables(cores, nodes, gram=False)["cum"]) > 1024
    chk = Q.verify(cores, nodes, u, None, 0.0, res["x"], res["cell"])
    assert np.all(res["val"] == tt.basis_batch(res["x"], _linear(nodes), "exact"))
    assert np.all(np.abs(res["logq"] - chk["logq"]) <= chk["logq_bound"])


@pytest.mark.parametrize("mode", MODES)
def test_sample_sq_on_the_same_engine_is_unchanged_before_and_after(mode):
    """the generalised split and head pass change nothing for the grid sampler: bit for bit the same before and after a real-valued call,
    and the same as on an engine that never made one"""
    cores, u, w = SQ.case("d8_unequal", True)
    nodes = _case("d8_unequal", True)[2]
    tt = E.TTCross.from_cores(cores)
    before = tt.sample_sq(u, w, gamma=0.125, mode=mode)
    real = tt.sample_sq_real(u, nodes, gamma=0.125, mode=mode)
    after = tt.sample_sq(u, w, gamma=0.125, mode=mode)
    assert all(before[k].tobytes() == after[k].tobytes() for k in ("ind", "logq", "val"))
    assert _same(real, _run("d8_unequal", True, mode, 0.125))
    assert SQ.verify(cores, u, w, None, 0.125, after["ind"])["undecided"] <= S.NPTS // 1000
    fresh = E.TTCross.from_cores(cores).sample_sq(u, w, gamma=0.125, mode=mode)
    assert all(fresh[k].tobytes() == after[k].tobytes() for k in ("ind", "logq", "val"))


def test_auto_and_last():
    cores, u, nodes = _case("d3", True)
    tt = _engine("d3", True)
    res = tt.sample_sq_real(u, nodes)                                   # auto: 2000 samples of d3 lie far below the threshold
    last = tt.sample_sq_real_last()
    assert last["mode"] == "exact" and last["failed"] == 0 and last["flops"] == 2000.0 * 2.0 * (5 * 1 * 3 + 7 * 3 * 2 + 4 * 2 * 1)
    assert last["ms_head"] > 0.0 and last["ms_rows"] > 0.0 and last["ms_pick"] > 0.0
    assert _same(res, _run("d3", True, "exact"))


def test_refusals():
    L = E.load_library()
    cores, u, nodes = _case("d3", True)
    tt = _engine("d3", True)
    EINVAL, ESTATE = 1, 4
    empty = tt.sample_sq_real(np.zeros((0, 3)), nodes)
    assert empty["x"].shape == (0, 3) and empty["logq"].shape == (0,) and tt.sample_sq_real(0, nodes)["val"].shape == (0,)
    for k, bad in ((0, np.nan), (1, np.inf)):
        nb = [t.copy() for t in nodes]
        nb[k][2] = bad
        with pytest.raises(E.TTXError):
            tt.sample_sq_real(u[:4], nb)
    nb = [t.copy() for t in nodes]
    nb[2][1] = nb[2][0]                                                # not strictly ascending
    with pytest.raises(E.TTXError, match="ascending"):
        tt.sample_sq_real(u[:4], nb)
    with pytest.raises(E.TTXError, match="infinite"):
        tt.sample_sq_real(u[:4], nodes, [np.nan, np.inf, np.nan])
    with pytest.raises(E.TTXError, match="gamma"):
        tt.sample_sq_real(u[:4], nodes, gamma=-1.0)
    with pytest.raises(ValueError):
        tt.sample_sq_real(u[:4], nodes, mode="fast")
    with pytest.raises(ValueError):
        tt.sample_sq_real(u[:4], nodes, [0.0, 0.0])
    with pytest.raises(ValueError):
        tt.sample_sq_real(u[:4, :2], nodes)
    with pytest.raises(ValueError):
        tt.sample_sq_real(u[:4], nodes[:2])
    x, nul_d, nul_i = np.zeros((4, 3)), ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_int32)()
    rowp = (ctypes.POINTER(ctypes.c_double) * 3)(*[E._dp(t) for t in nodes])
    au = E.EVAL_MODES["auto"]
    assert L.ttx_sample_sq_real(tt._h, 4, E._dp(u), rowp, nul_d, 0.0, au, E._dp(x), nul_i, nul_d, nul_d) == 0     # cell, logq and val may be NULL
    assert np.array_equal(x, _run("d3", True, "exact")["x"][:4])
    with pytest.raises(E.TTXError):                                    # ranks above 128, at creation or at the call
        big = [np.ones((1, 2, 129)), np.ones((129, 2, 1))]
        E.TTCross.from_cores(big).sample_sq_real(np.full((1, 2), 0.5), [np.arange(2.0)] * 2)
    s = D.ising_setup("c", 6, 9)
    fresh = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"])
    u5, x5 = np.full((1, 5), 0.5), np.zeros((1, 5))
    row5 = (ctypes.POINTER(ctypes.c_double) * 5)(*[E._dp(np.arange(9.0)) for _ in range(5)])
    assert L.ttx_sample_sq_real(fresh._h, 1, E._dp(u5), row5, nul_d, 0.0, au, E._dp(x5), nul_i, nul_d, nul_d) == ESTATE
    # a multi-process engine gets the answer ttx_ijk gives it (test_gpu_tijk_batch.py)
    mp = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"], nproc=2, world_rank=0, world_size=2)
    v = ctypes.c_double()
    want = L.ttx_ijk(mp._h, E._ip(np.ones((1, 5), np.int32)), ctypes.byref(v))
    assert want != 0 and L.ttx_sample_sq_real(mp._h, 1, E._dp(u5), row5, nul_d, 0.0, au, E._dp(x5), nul_i, nul_d, nul_d) == want


def test_fortran_sample_sq_real_val_is_the_basis_value_of_its_x():
    """the drop-in tt_lib: sample_sq_real(tt, u, nodes, x, logq=, val=) on a signed host train of rank 3, free and with mode 2 held
    between two nodes (with a defensive term, exact mode); val must EQUAL the program's own basisval(tt, x, 2, 0, 1, .., mode = 0) --
    ttx_basis_batch's exact chain on the same equidistant nodes; both are printed with 17 digits, which round-trip"""
    from conftest import fortran_exe
    exe = fortran_exe("test_tt_sample_sq_real")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("done"), p.stdout[-2000:] + p.stderr[-2000:]
    for tag in ("free", "held"):
        rows = np.array([[float(v) for v in ln.split()[1:]] for ln in p.stdout.splitlines() if ln.split() and ln.split()[0] == tag])
        assert rows.shape == (40, 9)
        xs = rows[:, 4:]
        assert np.all(xs >= 0.0) and np.all(xs <= 1.0) and len({tuple(r) for r in xs}) == 40
        assert np.all(np.isfinite(rows[:, 1])) and np.all(rows[:, 1] == rows[:, 2])
        assert np.all(np.isfinite(rows[:, 3]))
        if tag == "held":
            assert np.all(xs[:, 1] == 0.3)
    assert any(ln.split()[0] == "free" and float(ln.split()[2]) < 0.0 for ln in p.stdout.splitlines() if ln.split())  # the train is signed
