"""Ranks grown from data (ttx_basis_enrich_batch / ttx_basis_enrich_tab): what can be checked without a GPU, so that the thresholds of
tests/test_gpu_enrich.py rest on something other than the code under test -- the numpy restatement (tests/enrich_ref.py) against a
dense long-double G2_i Omega_i^T, the plan of a call (tests/enrich_plan_main.cpp, plain and under the sanitizers) against
enrich_ref.plan, the enriched numpy train against its source bit for bit, and the recovery run that the GPU test repeats."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import basis_core_grad_ref as C
import basis_ref as B
import enrich_ref as N
import tt_ref as R
from ttcross_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ttx_basis_enrich_batch", "ttx_basis_enrich_batch_dev", "ttx_basis_enrich_tab", "ttx_basis_enrich_tab_dev", "ttx_basis_enrich_last")
# the shapes of test_gpu_enrich.py in the order tests/enrich_plan_main.cpp prints them, and the k the issue's table expects at add = 20
SHAPES = [("mixed", [7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1], [4, 0, 4, 1]), ("two_rows_mr5", [4, 5, 3, 2], [1, 16, 33, 65, 1], [0, 20, 2]),
          ("bond128", [2, 2, 2], [1, 128, 128, 1], [0, 0]), ("mr6_mr8", [3, 2, 3], [1, 96, 113, 1], [0, 3]),
          ("ragged", [3, 4, 2, 5], [1, 2, 70, 3, 1], [1, 0, 5]), ("d2", [5, 7], [1, 3, 1], [2]),
          ("tiles", [4, 6, 5, 6, 4], [1, 4, 15, 17, 4, 1], [0, 9, 20, 4])]
DENSE = [s for s in SHAPES if s[0] in ("mixed", "ragged", "d2", "tiles")]
NPTS, ADD = 23, 20


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _data(n, r, seed, nonneg, npts=NPTS):
    rng = np.random.default_rng(seed)
    if nonneg:
        cores = [rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1])) for k in range(len(n))]
        return cores, [rng.uniform(0.0, 1.0, (npts, nk)) for nk in n], rng.uniform(0.0, 1.0, npts)
    return R.rand_train(seed, n, r), [rng.standard_normal((npts, nk)) for nk in n], rng.standard_normal(npts)


def test_header_and_library_declare_the_entry_points():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        raw = f.read()
    h = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw, flags=re.S))
    tail = "uint64_t seed, int32_t mode, ttx_engine **out, int32_t *added , double *gain , double *ynorm2 , double *y);"
    assert "int ttx_basis_enrich_batch (ttx_engine *h, int64_t npts, const double *x , const ttx_basis *basis , const double *c , const int32_t *add , " + tail in h
    assert "int ttx_basis_enrich_tab (ttx_engine *h, int64_t npts, const double *phi , const double *c, const int32_t *add, uint64_t seed" in h
    assert "int ttx_basis_enrich_last (const ttx_engine *h, double *ms_table, double *ms_back, double *ms_sketch, double *ms_qr, double *ms_asm, double *flops, int32_t *mode_ran, int64_t *chunk_ran);" in h
    for word in ("TTX_ENRICH_AUTO_FLOPS", "PROVISIONAL", "stationary point", "never formed"):
        assert word in raw, word
    with open(os.path.join(ROOT, "ttcross_amd", "csrc", "ttx_op_plan.h")) as f:
        assert re.search(r"PROVISIONAL, NOT MEASURED[^#]*#define TTX_EN_AUTO_FLOPS TTX_BS_AUTO_FLOPS", f.read())
    import __graft_entry__ as g
    L = ctypes.CDLL(g.build_lib())
    for sym in ENTRIES:
        assert hasattr(L, sym), sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() == 3                                                 # added without a new version
    for m in ("enrich", "enrich_tab", "enrich_last", "fit_adaptive", "enrich_density", "enrich_ranks"):
        assert callable(getattr(E.TTCross, m)), m
    assert "LEFT OUT" in E.TTCross.enrich_density.__doc__ and "stays open" in E.TTCross.enrich_density.__doc__
    for sym in ENTRIES:
        assert getattr(E.load_library(), sym).argtypes is not None, sym


@pytest.mark.parametrize("name,n,r,k", SHAPES)
def test_directions_per_bond_are_the_issues_table(name, n, r, k):
    assert N.plan_k(n, r, ADD) == k
    assert N.plan_k(n, r, 0) == [0] * (len(n) - 1)
    assert all(a <= b for a, b in zip(N.plan_k(n, r, 1), k)) and max(N.plan_k(n, r, 1), default=0) <= 1


def test_omega_is_lincomb_rounds_formula_with_the_bond_in_the_mode_field():
    n, r = [4, 6, 5, 6, 4], [1, 4, 15, 17, 4, 1]
    k = N.plan_k(n, r, ADD)
    oms = N.omegas(n, r, k, 77)
    assert [o.shape for o in oms] == [(0, 6, 15), (9, 5, 17), (20, 6, 4), (4, 4, 1)]
    flat = E.roundsum_omega(77, 3, (20 * 6 * 4,))
    assert np.array_equal(oms[2][7, 3, 2], flat[7 + 20 * (3 + 6 * 2)]) and np.all(np.abs(oms[2]) < 1.0)
    assert not np.array_equal(oms[2], N.omegas(n, r, k, 78)[2])


@pytest.mark.parametrize("name,n,r,k", DENSE)
def test_restatement_agrees_with_a_dense_long_double_two_site_gradient(name, n, r, k):
    """The restatement's Y_b lies within N_b u B_b of the true G2_b Omega_b^T (enrich_ref's derivation), one half of the allowance
    2 N_b u B_b.  The long-double einsum, which forms G2_b itself, stands for the true value: its own error is the same count at
    u = 2^-64, below 2^-10 of that half, which the factor (1 + 2^-10) takes in."""
    for nonneg in (False, True):
        cores, phis, c = _data(n, r, 5 + len(n), nonneg)
        sk = N.sketch(cores, phis, c, ADD, 3)
        assert sk["k"] == k
        dense, bnd = N.dense_longdouble(cores, phis, c, ADD, 3), N.bound(cores, phis, c, ADD, 3)
        for b in range(1, len(n)):
            y = sk["y"][b - 1]
            assert y.shape == (r[b - 1], n[b - 1], k[b - 1]) == dense[b - 1].shape
            err = np.abs(y.astype(np.longdouble) - dense[b - 1]).astype(np.float64)
            assert np.all(err <= 0.5 * (1.0 + 2.0 ** -10) * bnd[b - 1]), (nonneg, b, float(np.max(err / bnd[b - 1])))
            assert sk["ynorm2"][b - 1] == pytest.approx(float(np.sum(y * y)), rel=1e-12, abs=0.0)


def test_count_is_the_formula_of_the_derivation():
    cores = R.rand_train(2, [3, 4, 2, 5], [1, 2, 70, 3, 1])
    assert N.count(cores, 1, 1, 10) == (4 * 70 + 2) + (2 * 3 + 2) + (5 * 1 + 2) + 10 + 4        # Omega_1 (1, 4, 70) in place of core 2
    assert N.count(cores, 3, 5, 7) == (3 * 1 + 2) + (4 * 2 + 2) + (5 * 1 + 2) + 7 + 4           # Omega_3 (5, 5, 1) in place of core 4


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no host C++ compiler")
    return c


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_plan_of_an_enrichment_call_agrees_with_the_restatement(cxx, tmp_path, flags):
    exe = str(tmp_path / "enrich_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "ttcross_amd", "csrc"), os.path.join(ROOT, "tests", "enrich_plan_main.cpp"), "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    lines = p.stdout.strip().splitlines()
    assert re.fullmatch(r"enrich plan: ok \((\d+) plans\)", lines[-1]), p.stdout
    assert int(re.search(r"\((\d+) plans", lines[-1]).group(1)) == 13 * 6 * 4 * 3 * 9 * 5 * 5
    assert len(lines) == len(SHAPES) + 1
    for line, (name, n, r, k) in zip(lines, SHAPES):
        got, want = json.loads(line), N.plan(n, r, ADD)
        assert got["k"] == want["k"] == k, name
        assert got["rnew"] == want["rnew"] and got["ldx"] == want["ldx"] and got["S"] == want["S"], name
        assert [tuple(q) for q in got["qr"]] == want["qr"], name


@pytest.mark.parametrize("name,n,r,k", DENSE)
def test_enriched_numpy_train_evaluates_bit_for_bit_like_the_source(name, n, r, k):
    cores, phis, c = _data(n, r, 11 + len(n), False)
    sk = N.sketch(cores, phis, c, ADD, 5)
    grown = N.enriched(cores, sk["y"], sk["k"])
    assert [u.shape for u in grown] == [(a, nk, b) for a, nk, b in zip(N.plan(n, r, ADD)["rnew"][:-1], n, N.plan(n, r, ADD)["rnew"][1:])]
    fresh = [np.random.default_rng(9).standard_normal((31, nk)) for nk in n]
    for tabs in (phis, fresh):
        assert np.array_equal(_bits(B.chain(grown, tabs)), _bits(B.chain(cores, tabs)))
    for b in range(1, len(n)):
        if not k[b - 1]:
            continue
        Q, gain, _ = N.new_directions(cores[b - 1], sk["y"][b - 1])
        UL = cores[b - 1].reshape((-1, r[b]), order="F")
        rows = UL.shape[0]
        assert np.max(np.abs(Q.T @ Q - np.eye(k[b - 1]))) <= 8 * rows * B.U
        assert np.max(np.abs(UL.T @ Q)) <= 8 * rows * B.U * np.linalg.norm(UL, 2)
        assert np.all(gain >= 0.0) and float(np.sum(gain * gain)) <= sk["ynorm2"][b - 1] * (1.0 + 1e-12)    # what lies outside range(U^L) is no longer than Y


def test_one_enrichment_recovers_a_fit_that_stalled_below_the_true_ranks():
    """fit_problem()'s truth has ranks [1, 3, 2, 1]; truncated to [1, 2, 1, 1] the fit stalls, one direction per bond from the residual
    and a second fit reach the data to rounding, for three seeds of the sketch"""
    for seed in (0, 1, 2):
        stalled, after, ranks = N.recovery_numpy(seed)
        print("seed", seed, "stalled", stalled, "after", after, "ratio", after / stalled)
        assert ranks == [1, 3, 2, 1]
        assert 6.8 < stalled < 6.9 and after <= 1e-20 * stalled
    start = N.recovery_start()[0]
    assert [u.shape for u in start] == [(1, 5, 2), (2, 6, 1), (1, 4, 1)]
    assert [u.shape for u in N.truth()] == [(1, 5, 3), (3, 6, 2), (2, 4, 1)] and np.array_equal(B.chain(N.truth(), C.fit_problem()[1]), C.fit_problem()[2])
