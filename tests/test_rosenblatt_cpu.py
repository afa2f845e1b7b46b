"""ttx_rosenblatt_sq_real without a GPU: the numpy reference (tests/rosenblatt_ref.py) checked against the sampler's reference and
against the dense tensor, sqr_cdf as a stand-alone program (plain and under the address and undefined-behaviour sanitizers), and
the refusals of the C entry that precede any look at the engine.

The round trip is the proof that the GPU test's bound is met by the reference alone: forward(draw(u)) must return min(u, 1) within
the sum of the sampler's allowance (sample_sq_real_ref.verify's tol_k) and the forward map's (tol_fwd), both over the total and
with 4 u for the divisions (rosenblatt_ref's docstring)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import rosenblatt_cases as RC
import rosenblatt_ref as F
import sample_sq_real_ref as Q
from ttcross_amd import engine as E

EINVAL, ESTATE = 1, 4
U_ = F.U


@pytest.mark.parametrize("name,signed", RC.ALL, ids=RC.IDS)
def test_forward_of_the_references_draw_returns_u(name, signed):
    cores, u, nodes = RC.case(name, signed)
    x, cell, logq, val, failed = Q.draw(cores, nodes, u)
    assert not failed.any()
    w = F.walk(cores, nodes, x)
    assert not w["failed"].any()
    assert np.array_equal(w["logq"], logq) and np.array_equal(w["val"], val)         # the same operations along the same x
    assert np.all((w["cell"] == cell) | ((w["cell"] == cell + 1) & (x == np.stack([t[np.minimum(cell[:, k], t.size - 1)] for k, t in enumerate(nodes)], axis=1))))
    drawn = np.array([t.size > 1 for t in nodes])
    assert np.all(w["u"][:, ~drawn] == 0.0) and np.all(w["cell"][:, ~drawn] == 0)
    err, bound = np.abs(w["u"] - np.minimum(u, 1.0))[:, drawn], F.u_bound(w, w["tol_inv"])[:, drawn]
    print(name, "signed" if signed else "non-negative", "N", w["N"], "max |u' - u|", float(err.max()), "in units of the bound", float((err / bound).max()))
    assert np.all(err <= bound)


def test_forward_with_held_modes_and_a_defensive_term():
    cores, u, nodes = RC.case("d6_size1_rank1", True)
    cond = [np.nan, np.nan, float(nodes[2][3]), np.nan, 0.5 * (nodes[4][1] + nodes[4][2]), float(nodes[5][-1]) + 2.0]
    x, cell, logq, val, failed = Q.draw(cores, nodes, u, cond, 0.5)
    xn = x.copy()
    xn[:, [1, 2, 3, 4, 5]] = np.nan                                     # the x of a held mode is not looked at
    w = F.walk(cores, nodes, xn, cond, 0.5)
    assert not w["failed"].any() and np.array_equal(w["logq"], logq) and np.array_equal(w["val"], val)
    assert np.all(w["u"][:, 1:] == 0.0) and np.all(w["cell"][:, 1:] == 0)
    assert np.all(np.abs(w["u"][:, 0] - u[:, 0]) <= F.u_bound(w, w["tol_inv"])[:, 0])


@pytest.mark.parametrize("gamma", [0.0, 0.25])
def test_u_is_the_dense_conditional_cdf_on_d3_and_logq_the_dense_density(gamma):
    """points the sampler did not draw: a seeded cloud in the box, every node of every mode, both ends of the box"""
    cores, _, nodes = RC.case("d3", True)
    x = np.concatenate([RC.cloud(nodes, 300, 11), np.array([[t[min(i, t.size - 1)] for t in nodes] for i in range(7)]),
                        np.array([[t[0] for t in nodes], [t[-1] for t in nodes]])])
    w = F.walk(cores, nodes, x, None, gamma)
    assert not w["failed"].any()
    assert np.all(w["u"][-2] == 0.0) and np.all(w["u"][-1] == 1.0)
    dense = F.dense_u(cores, nodes, x, gamma)
    err = np.abs(w["u"].astype(np.longdouble) - dense).astype(np.float64)
    bound = F.u_bound(w)
    print("gamma", gamma, "max |u - dense| in units of the bound", float((err / bound).max()))
    assert np.all(err <= bound)
    ZV = float(Q.dense_Z(cores, nodes)) + gamma * Q.volume(nodes)
    want = w["val"] * w["val"] + gamma
    rel = np.abs(np.exp(w["logq"]) * ZV - want) / want
    lim = w["logq_bound"] + 4.0 * w["N"] * U_
    print("   max |exp(logq) (Z + gamma V) - (val^2 + gamma)| / (val^2 + gamma) / bound", float((rel / lim).max()))
    assert np.all(rel <= lim)
    assert np.all(np.abs(w["val"] - Q.R.dense_interpolant(cores, nodes, x)) <= 4.0 * w["N"] * U_ * np.abs(Q.R.dense_interpolant([np.abs(c) for c in cores], nodes, x)))


def test_failed_points_and_a_cell_without_mass():
    cores, _, nodes = RC.case("d3", False)
    x = RC.cloud(nodes, 12, 5)
    x[1, 0], x[3, 2], x[5, 1], x[7, 0] = np.nan, np.inf, np.nextafter(nodes[1][-1], np.inf), np.nextafter(nodes[0][0], -np.inf)
    u, cell, logq, val, failed = F.forward(cores, nodes, x)
    assert np.flatnonzero(failed).tolist() == [1, 3, 5, 7]
    assert np.all(np.isnan(u[failed])) and np.all(cell[failed] == 0) and np.all(np.isnan(logq[failed])) and np.all(val[failed] == 0.0)
    assert np.all(np.isfinite(u[~failed])) and np.all(cell[~failed] >= 1)
    # a cell without mass in the mode walked LAST (after a massless cell of another mode the state is 0 and the next total with it)
    hole = [c.copy() for c in cores]
    hole[0][:, 2:4, :] = 0.0                                            # cell 3 of mode 1 has no mass
    xm = RC.cloud(nodes, 8, 6)
    xm[:, 0] = np.minimum(nodes[0][2] + (nodes[0][3] - nodes[0][2]) * np.linspace(0.0, 1.0, 8), np.nextafter(nodes[0][3], -np.inf))
    xm[7, 0] = nodes[0][3]                                              # on the right node: the next cell, at its massless end
    u, cell, logq, val, failed = F.forward(hole, nodes, xm)
    assert not failed.any() and np.all(cell[:, 0] == np.array([3] * 7 + [4])) and np.all(logq == -np.inf) and np.all(val == 0.0)
    assert np.all((u[:, 0] > 0.0) & (u[:, 0] < 1.0)) and np.all(np.isfinite(u))
    xh = xm.copy()
    xh[:, 1] = nodes[1][2]                                              # the same in mode 2: the state is 0 from there on, mode 1 has no mass
    hole2 = [c.copy() for c in cores]
    hole2[1][:, 2, :] = 0.0
    assert F.forward(hole2, nodes, xh)[4].all()
    zero = [np.zeros_like(c) for c in cores]
    assert F.forward(zero, nodes, xm)[4].all() and not F.forward(zero, nodes, xm, None, 1.0)[4].any()


def test_the_three_symbols_and_the_wrappers_exist():
    L = E.load_library()
    for name in ("ttx_rosenblatt_sq_real", "ttx_rosenblatt_sq_real_dev", "ttx_rosenblatt_sq_real_last"):
        assert hasattr(L, name)
    assert callable(E.TTCross.rosenblatt_sq_real) and callable(E.TTCross.rosenblatt_sq_real_last)


def test_refusals_before_the_engine_is_looked_at():
    L = E.load_library()
    x, u = np.zeros((2, 3)), np.zeros((2, 3))
    rows = [np.arange(4.0)] * 3
    rowp = (ctypes.POINTER(ctypes.c_double) * 3)(*[E._dp(t) for t in rows])
    nul_d, nul_i, nul_r = ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.POINTER(ctypes.c_double))()
    ex, au = E.EVAL_MODES["exact"], E.EVAL_MODES["auto"]
    assert L.ttx_rosenblatt_sq_real(None, -1, E._dp(x), rowp, nul_d, 0.0, ex, E._dp(u), nul_i, nul_d, nul_d) == EINVAL
    assert L.ttx_rosenblatt_sq_real(None, 2, nul_d, rowp, nul_d, 0.0, ex, E._dp(u), nul_i, nul_d, nul_d) == EINVAL
    assert L.ttx_rosenblatt_sq_real(None, 2, E._dp(x), rowp, nul_d, 0.0, ex, nul_d, nul_i, nul_d, nul_d) == EINVAL
    assert L.ttx_rosenblatt_sq_real(None, 2, E._dp(x), nul_r, nul_d, 0.0, ex, E._dp(u), nul_i, nul_d, nul_d) == EINVAL
    assert L.ttx_rosenblatt_sq_real(None, 2, E._dp(x), rowp, nul_d, 0.0, 77, E._dp(u), nul_i, nul_d, nul_d) == EINVAL
    assert b"unknown mode" in L.ttx_last_error()
    for g in (-1e-300, -1.0, float("inf"), float("-inf"), float("nan")):
        assert L.ttx_rosenblatt_sq_real(None, 2, E._dp(x), rowp, nul_d, g, au, E._dp(u), nul_i, nul_d, nul_d) == EINVAL
        assert b"gamma" in L.ttx_last_error()
    assert L.ttx_rosenblatt_sq_real_dev(None, -1, None, rowp, nul_d, 0.0, ex, None, None, None, None) == EINVAL
    assert L.ttx_rosenblatt_sq_real_dev(None, 2, None, rowp, nul_d, 0.0, ex, None, None, None, None) == EINVAL
    assert b"ttx_rosenblatt_sq_real_dev" in L.ttx_last_error()
    assert L.ttx_rosenblatt_sq_real_last(None, None, None, None, None, None, None) == EINVAL
    # sound arguments and no engine: the state error, still without a device
    assert L.ttx_rosenblatt_sq_real(None, 2, E._dp(x), rowp, nul_d, 0.0, au, E._dp(u), nul_i, nul_d, nul_d) == ESTATE
    assert L.ttx_rosenblatt_sq_real(None, 0, nul_d, nul_r, nul_d, 0.5, au, nul_d, nul_i, nul_d, nul_d) == ESTATE


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "ttcross_amd", "csrc"),
                    os.path.join(ROOT, "tests", "rosenblatt_main.cpp"), "-o", str(exe)], check=True)
    return exe


def _check_main(out):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad, cases, worst = out.stdout.strip().splitlines()[-1].split()
    print("worst |sqr_cdf(sqr_invert(s')) - s'| in units of the bound", worst)
    assert int(bad) == 0 and int(cases) > 240000 and float(worst) <= 1.0


def test_the_cubic_and_its_inversion_round_trip_as_a_host_program(tmp_path):
    _check_main(subprocess.run([str(_build(tmp_path, "rosenblatt", []))], capture_output=True, text=True))


def test_the_round_trip_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path, "rosenblatt_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    _check_main(subprocess.run([str(exe)], capture_output=True, text=True, env=env))
