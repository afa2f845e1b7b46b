"""ttx_sample_sq_real without a GPU: the numpy reference (tests/sample_sq_real_ref.py) checked against itself and against the dense
tensor, the host-side code as a stand-alone program (plain and under the address and undefined-behaviour sanitizers), and the
refusals of the C entry that precede any look at the engine.

The reference carries two independent evaluations of the conditional rows: the float64 factor route of the definition (QR of the
rows built from the mass matrix's Cholesky factor) and prefix Gram matrices in long double built from the mass matrices themselves.
The factor route's verify walks along the points the Gram route drew: the two must agree within a quarter of the allowance
everywhere.  The cases are sample_ref.CASES with sample_real_ref.case's nodes, non-negative and signed, 2000 samples."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import sample_ref as S
import sample_sq_real_ref as Q
from ttcross_amd import engine as E

EINVAL, ESTATE = 1, 4
ALL = [(k, s) for k in S.CASES for s in (False, True)]
IDS = [k + ("_signed" if s else "") for k, s in ALL]
U_ = S.U


@pytest.mark.parametrize("name,signed", ALL, ids=IDS)
def test_the_two_routes_agree_within_a_quarter_of_the_allowance(name, signed):
    cores, u, nodes = Q.case(name, signed)
    x, cell = Q.draw(cores, nodes, u, route="gram")[:2]
    chk = Q.verify(cores, nodes, u, None, 0.0, x, cell, routes=True)
    print(name, "signed" if signed else "non-negative", "N", chk["N"], "worst CDF miss", chk["worst"], "routes differ by", chk["gap"], "of the allowance")
    assert chk["gap"] <= 0.25


def test_the_routes_agree_with_a_defensive_term_and_held_modes():
    cores, u, nodes = Q.case("d6_size1_rank1", True)
    cond = [np.nan, np.nan, float(nodes[2][3]), np.nan, 0.5 * (nodes[4][1] + nodes[4][2]), float(nodes[5][-1]) + 2.0]
    x, cell = Q.draw(cores, nodes, u, cond, 0.5, route="gram")[:2]
    chk = Q.verify(cores, nodes, u, cond, 0.5, x, cell, routes=True)
    assert chk["gap"] <= 0.25
    assert np.all(cell[:, [1, 2, 3, 4, 5]] == 0) and np.all(x[:, 2] == cond[2]) and np.all(x[:, 5] == cond[5])


def test_mass_cholesky_of_the_package_is_the_references_bit_for_bit():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 16, 257):
        t = np.cumsum(rng.uniform(1e-3, 2.0, n)) - 4.0
        dg, sp = E.mass_cholesky(t)
        rdg, rsp = Q.mass_cholesky(t)
        assert np.array_equal(dg, rdg) and np.array_equal(sp, rsp)
        Uf = np.diag(dg) + np.diag(sp[:-1], 1)
        assert np.abs(Uf.T @ Uf - Q.mass_matrix(t).astype(np.float64)).max() <= 8.0 * U_ * np.diff(t).max() if n > 1 else True
    pairs = E.mass_cholesky([np.arange(3.0), np.arange(4.0)])
    assert len(pairs) == 2 and pairs[1][0].size == 4


@functools.lru_cache(maxsize=None)
def _chi_draw(gamma):
    cores, _, nodes = Q.case("d3", True)
    u = np.random.default_rng(Q.CHI_SEED).random((Q.CHI_NPTS, 3))
    return cores, nodes, u, Q.draw(cores, nodes, u, None, gamma)


@pytest.mark.parametrize("gamma", [0.0, Q.CHI_GAMMA])
def test_dense_identity_on_d3_signed(gamma):
    """exp(logq) (Z + gamma V) = val^2 + gamma with Z from the dense tensor and the mass matrices, within the derived logq bound"""
    cores, nodes, u, (x, cell, logq, val, failed) = _chi_draw(gamma)
    assert not failed.any()
    chk = Q.verify(cores, nodes, u, None, gamma, x, cell)
    assert np.array_equal(logq, chk["logq"]) and np.array_equal(val, chk["val"])
    dense = Q.R.dense_interpolant(cores, nodes, x[:500])
    assert np.all(np.abs(val[:500] - dense) <= 4.0 * chk["N"] * U_ * np.abs(Q.R.dense_interpolant([np.abs(c) for c in cores], nodes, x[:500])))
    ZV = float(Q.dense_Z(cores, nodes)) + gamma * Q.volume(nodes)
    want = val * val + gamma
    rel = np.abs(np.exp(logq) * ZV - want) / want
    bound = chk["logq_bound"] + 4.0 * chk["N"] * U_
    print("gamma", gamma, "max |exp(logq) (Z + gamma V) - (val^2 + gamma)| / (val^2 + gamma) / bound", float((rel / bound).max()))
    assert np.all(rel <= bound)


@pytest.mark.parametrize("gamma", [0.0, Q.CHI_GAMMA])
def test_the_reference_draws_cell_frequencies_pass_chi_square(gamma):
    cores, nodes, u, (x, cell, logq, val, failed) = _chi_draw(gamma)
    rho = Q.dense_cell_masses(cores, nodes, gamma).astype(np.float64)
    assert rho.size == 72 and abs(float(rho.sum()) - 1.0) < 1e-15
    stat, q = Q.chi2(cell, rho), Q.chi2_quantile(71)
    print("gamma", gamma, "chi-square", stat, "quantile at 1 - 1e-6", q)
    assert stat <= q


def test_the_numpy_inversion_meets_the_residual_bound():
    rng = np.random.default_rng(9)
    s0, s1 = rng.random(20000), rng.random(20000)
    lim = np.sqrt(s0) * np.sqrt(s1)
    c = np.where(rng.random(20000) < 0.3, -lim, (2.0 * rng.random(20000) - 1.0) * lim)
    g = np.where(rng.random(20000) < 0.5, 0.0, rng.random(20000) * 1e-3)
    q0, qm, q1 = s0 + g, c + g, s1 + g
    sp = rng.random(20000) * (((q0 + qm) + q1) / 3.0)
    lam = Q.invert(q0, qm, q1, sp)
    LD = np.longdouble
    l = lam.astype(LD)
    res = np.abs(q0.astype(LD) * l * (1 - l) ** 2 + (q0.astype(LD) + qm) * l * l * (1 - l) + (q0.astype(LD) + qm + q1) / 3 * l ** 3 - sp)
    assert np.all((lam >= 0.0) & (lam <= 1.0))
    assert np.all(res <= 32.0 * U_ * np.maximum(np.maximum(q0, q1), np.abs(qm)))
    assert np.array_equal(Q.invert([np.nan, 1.0, 0.0, 1.0], [1.0, np.inf, 0.0, 1.0], [1.0, 1.0, 0.0, 1.0], [0.1, 0.1, 0.0, 5.0]), [0.0, 0.0, 0.0, 1.0])


def test_the_three_symbols_exist():
    L = E.load_library()
    for name in ("ttx_sample_sq_real", "ttx_sample_sq_real_dev", "ttx_sample_sq_real_last"):
        assert hasattr(L, name)
    assert callable(E.TTCross.sample_sq_real) and callable(E.TTCross.sample_sq_real_last) and callable(E.mass_cholesky)


def test_refusals_before_the_engine_is_looked_at():
    L = E.load_library()
    u, x = np.zeros((2, 3)), np.zeros((2, 3))
    rows = [np.arange(4.0)] * 3
    rowp = (ctypes.POINTER(ctypes.c_double) * 3)(*[E._dp(t) for t in rows])
    nul_d, nul_i, nul_r = ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.POINTER(ctypes.c_double))()
    ex, au = E.EVAL_MODES["exact"], E.EVAL_MODES["auto"]
    assert L.ttx_sample_sq_real(None, -1, E._dp(u), rowp, nul_d, 0.0, ex, E._dp(x), nul_i, nul_d, nul_d) == EINVAL
    assert L.ttx_sample_sq_real(None, 2, nul_d, rowp, nul_d, 0.0, ex, E._dp(x), nul_i, nul_d, nul_d) == EINVAL
    assert L.ttx_sample_sq_real(None, 2, E._dp(u), rowp, nul_d, 0.0, ex, nul_d, nul_i, nul_d, nul_d) == EINVAL
    assert L.ttx_sample_sq_real(None, 2, E._dp(u), nul_r, nul_d, 0.0, ex, E._dp(x), nul_i, nul_d, nul_d) == EINVAL
    assert L.ttx_sample_sq_real(None, 2, E._dp(u), rowp, nul_d, 0.0, 77, E._dp(x), nul_i, nul_d, nul_d) == EINVAL
    assert b"unknown mode" in L.ttx_last_error()
    for g in (-1e-300, -1.0, float("inf"), float("-inf"), float("nan")):
        assert L.ttx_sample_sq_real(None, 2, E._dp(u), rowp, nul_d, g, au, E._dp(x), nul_i, nul_d, nul_d) == EINVAL
        assert b"gamma" in L.ttx_last_error()
    assert L.ttx_sample_sq_real_dev(None, -1, None, rowp, nul_d, 0.0, ex, None, None, None, None) == EINVAL
    assert L.ttx_sample_sq_real_dev(None, 2, None, rowp, nul_d, 0.0, ex, None, None, None, None) == EINVAL
    assert b"ttx_sample_sq_real_dev" in L.ttx_last_error()
    assert L.ttx_sample_sq_real_last(None, None, None, None, None, None, None) == EINVAL
    # sound arguments and no engine: the state error, still without a device
    assert L.ttx_sample_sq_real(None, 2, E._dp(u), rowp, nul_d, 0.0, au, E._dp(x), nul_i, nul_d, nul_d) == ESTATE
    assert L.ttx_sample_sq_real(None, 0, nul_d, nul_r, nul_d, 0.5, au, nul_d, nul_i, nul_d, nul_d) == ESTATE


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "ttcross_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sample_sq_real_main.cpp"), "-o", str(exe)], check=True)
    return exe


def _check_main(out):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad, factors, inversions, worst = out.stdout.strip().splitlines()[-1].split()
    print("worst residual of sqr_invert in units of the bound", worst)
    assert int(bad) == 0 and int(factors) == 2000 and int(inversions) > 200000 and float(worst) <= 1.0


def test_factor_and_inversion_checks_as_a_host_program(tmp_path):
    _check_main(subprocess.run([str(_build(tmp_path, "sample_sq_real", []))], capture_output=True, text=True))


def test_factor_and_inversion_checks_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path, "sample_sq_real_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    _check_main(subprocess.run([str(exe)], capture_output=True, text=True, env=env))
