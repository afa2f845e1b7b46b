"""ttx_sample_sq without a GPU: the numpy reference (tests/sample_sq_ref.py) checked against itself, and the refusals of the C entry
that precede any look at the engine.

The reference carries two independent evaluations of the conditional rows, the float64 factor route of the definition and prefix
Gram matrices in long double.  Here the factor route's verify walks along the indices the Gram route drew: the two must agree
within a quarter of the allowance everywhere, and at most 0.1 % of a case's samples may have an undecided mode -- the cap the GPU
test applies to the device, shown here to hold for the reference alone.  The cases are sample_ref.CASES with standard-normal cores
(signed) and uniform(0.1, 1) cores, |w| as weights, 2000 samples, the cases' own seeds."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import sample_ref as S
import sample_sq_ref as Q
from ttcross_amd import engine as E

EINVAL, ESTATE = 1, 4
ALL = [(k, s) for k in S.CASES for s in (False, True)]
IDS = [k + ("_signed" if s else "") for k, s in ALL]


@pytest.mark.parametrize("name,signed", ALL, ids=IDS)
def test_the_two_routes_agree_and_the_cap_holds_on_the_reference_alone(name, signed):
    cores, u, w = Q.case(name, signed)
    ind = Q.draw(cores, u, w, route="gram")[0]
    chk = Q.verify(cores, u, w, None, 0.0, ind, routes=True)
    print(name, "signed" if signed else "non-negative", "N", chk["N"], "undecided", chk["undecided"], "of", S.NPTS, "routes differ by", chk["gap"], "of the allowance")
    assert chk["undecided"] <= S.NPTS // 1000
    assert chk["gap"] <= 0.25


def test_the_routes_agree_with_a_defensive_term_and_fixed_modes():
    cores, u, w = Q.case("d6_size1_rank1", True)
    fixed = [0, 1, 0, 0, 3, 0]
    ind = Q.draw(cores, u, w, fixed, 0.5, route="gram")[0]
    chk = Q.verify(cores, u, w, fixed, 0.5, ind, routes=True)
    assert chk["undecided"] <= S.NPTS // 1000 and chk["gap"] <= 0.25
    assert np.all(ind[:, 1] == 1) and np.all(ind[:, 4] == 3)


@functools.lru_cache(maxsize=None)
def _chi_draw(gamma):
    cores, _, w = Q.case("d3", True)
    u = np.random.default_rng(Q.CHI_SEED).random((Q.CHI_NPTS, 3))
    return cores, u, w, Q.draw(cores, u, w, None, gamma)


@pytest.mark.parametrize("gamma", [0.0, Q.CHI_GAMMA])
def test_dense_identity_on_d3_signed(gamma):
    """exp(logq) = (T^2 + gamma) prod w / (Z + gamma prod W) from the dense tensor, within the derived logq bound"""
    cores, u, w, (ind, logq, val, failed) = _chi_draw(gamma)
    assert not failed.any()
    chk = Q.verify(cores, u, w, None, gamma, ind)
    rho = Q.dense_density(cores, w, None, gamma)[tuple((ind - 1).T)].astype(np.float64)
    assert abs(float(Q.dense_density(cores, w, None, gamma).sum()) - 1.0) < 1e-15
    assert np.array_equal(logq, chk["logq"])
    rel = np.abs(np.exp(logq) - rho) / rho
    print("gamma", gamma, "max |exp(logq) - rho| / rho / bound", float((rel / (chk["logq_tol"] + 4.0 * U_)).max()))
    assert np.all(rel <= chk["logq_tol"] + 4.0 * U_)


U_ = S.U


@pytest.mark.parametrize("gamma", [0.0, Q.CHI_GAMMA])
def test_the_reference_draws_frequencies_pass_chi_square(gamma):
    cores, u, w, (ind, logq, val, failed) = _chi_draw(gamma)
    rho = Q.dense_density(cores, w, None, gamma).astype(np.float64)
    assert rho.size == 140
    stat, q = Q.chi2(ind, rho), Q.chi2_quantile(139)
    print("gamma", gamma, "chi-square", stat, "quantile at 1 - 1e-6", q)
    assert stat <= q


def test_the_three_symbols_exist():
    L = E.load_library()
    for name in ("ttx_sample_sq", "ttx_sample_sq_dev", "ttx_sample_sq_last"):
        assert hasattr(L, name)


def test_refusals_before_the_engine_is_looked_at():
    L = E.load_library()
    u, ind = np.zeros((2, 3)), np.zeros((2, 3), np.int32)
    nul_d, nul_i = ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_int32)()
    ex, au = E.EVAL_MODES["exact"], E.EVAL_MODES["auto"]
    assert L.ttx_sample_sq(None, -1, E._dp(u), nul_d, nul_i, 0.0, ex, E._ip(ind), nul_d, nul_d) == EINVAL
    assert L.ttx_sample_sq(None, 2, nul_d, nul_d, nul_i, 0.0, ex, E._ip(ind), nul_d, nul_d) == EINVAL
    assert L.ttx_sample_sq(None, 2, E._dp(u), nul_d, nul_i, 0.0, ex, nul_i, nul_d, nul_d) == EINVAL
    assert L.ttx_sample_sq(None, 2, E._dp(u), nul_d, nul_i, 0.0, 77, E._ip(ind), nul_d, nul_d) == EINVAL
    assert b"unknown mode" in L.ttx_last_error()
    for g in (-1e-300, -1.0, float("inf"), float("-inf"), float("nan")):
        assert L.ttx_sample_sq(None, 2, E._dp(u), nul_d, nul_i, g, au, E._ip(ind), nul_d, nul_d) == EINVAL
        assert b"gamma" in L.ttx_last_error()
    assert L.ttx_sample_sq_dev(None, -1, None, nul_d, nul_i, 0.0, ex, None, None, None) == EINVAL
    assert L.ttx_sample_sq_dev(None, 2, None, nul_d, nul_i, 0.0, ex, None, None, None) == EINVAL
    assert b"ttx_sample_sq_dev" in L.ttx_last_error()
    assert L.ttx_sample_sq_last(None, None, None, None, None, None, None) == EINVAL
    # sound arguments and no engine: the state error, still without a device
    assert L.ttx_sample_sq(None, 2, E._dp(u), nul_d, nul_i, 0.0, au, E._ip(ind), nul_d, nul_d) == ESTATE
    assert L.ttx_sample_sq(None, 0, nul_d, nul_d, nul_i, 0.5, au, nul_i, nul_d, nul_d) == ESTATE


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "ttcross_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sample_sq_main.cpp"), "-o", str(exe)], check=True)
    return exe


def _check_main(out):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad, plans, checks = (int(v) for v in out.stdout.strip().splitlines()[-1].split())
    assert bad == 0 and plans == 4000 and checks > 100 * plans


def test_plan_and_weight_checks_as_a_host_program(tmp_path):
    _check_main(subprocess.run([str(_build(tmp_path, "sample_sq", []))], capture_output=True, text=True))


def test_plan_and_weight_checks_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path, "sample_sq_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    _check_main(subprocess.run([str(exe)], capture_output=True, text=True, env=env))

