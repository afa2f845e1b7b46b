"""Gradient with respect to the cores of the train in a function basis (ttx_basis_core_grad_batch, ttx_basis_core_grad_tab,
ttx_cores_axpy): what can be checked without a GPU -- the numpy restatement (tests/basis_core_grad_ref.py) against a dense long-double
einsum of the definition and against the linearity identity, the C ABI as declared and exported, the plan of a call
(tests/basis_core_grad_plan_main.cpp, plain and under the sanitizers) and the block-coordinate fit that the GPU test repeats."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import basis_core_grad_ref as C
import basis_ref as B
import tt_ref as R
from ttcross_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ttx_basis_core_grad_batch", "ttx_basis_core_grad_batch_dev", "ttx_basis_core_grad_tab", "ttx_basis_core_grad_tab_dev",
           "ttx_basis_core_grad_last", "ttx_cores_axpy", "ttx_cores_axpy_dev")
SHAPES = [([7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]), ([3, 4, 2, 5], [1, 2, 70, 3, 1]), ([5, 7], [1, 3, 1]), ([5], [1, 1])]
NPTS = 23


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
    for decl in ("int ttx_basis_core_grad_batch (ttx_engine *h, int64_t npts, const double *x , const ttx_basis *basis , const double *c , double *val, double *g, int32_t accumulate, int32_t mode);",
                 "int ttx_basis_core_grad_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, const double *c_dev, double *val_dev, double *g_dev, int32_t accumulate, int32_t mode);",
                 "int ttx_basis_core_grad_tab (ttx_engine *h, int64_t npts, const double *phi , const double *c, double *val, double *g, int32_t accumulate, int32_t mode);",
                 "int ttx_basis_core_grad_tab_dev (ttx_engine *h, int64_t npts, const double *phi_dev, const double *c_dev, double *val_dev, double *g_dev, int32_t accumulate, int32_t mode);",
                 "int ttx_basis_core_grad_last (const ttx_engine *h, double *ms_table, double *ms_back, double *ms_fwd, double *ms_acc, double *flops, int32_t *mode_ran, int64_t *chunk_ran);",
                 "int ttx_cores_axpy (ttx_engine *h, const double *alpha , const double *g);",
                 "int ttx_cores_axpy_dev(ttx_engine *h, const double *alpha , const double *g_dev);"):
        assert decl in h, decl
    assert "gradients with respect to cores" not in raw                         # no longer on the open list of ttx_basis_grad_batch
    assert "MAY DEPEND ON THE POINTS PER CHUNK" in raw and "finite coordinates" in raw
    with open(os.path.join(ROOT, "ttcross_amd", "csrc", "ttx_op_plan.h")) as f:
        plan = f.read()
    assert re.search(r"PROVISIONAL, NOT MEASURED[^\n]*\n[^\n]*\n#define TTX_CG_AUTO_FLOPS TTX_BS_AUTO_FLOPS", plan)
    import __graft_entry__ as g
    L = ctypes.CDLL(g.build_lib())
    for sym in ENTRIES:
        assert hasattr(L, sym), sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() == 3                                                 # added without a new version
    for m in ("basis_core_grad", "basis_core_grad_tab", "basis_core_grad_last", "cores_axpy", "core_offsets"):
        assert callable(getattr(E.TTCross, m)), m
    for sym in ENTRIES:
        assert getattr(E.load_library(), sym).argtypes is not None, sym


@pytest.mark.parametrize("n,r", SHAPES)
def test_restatement_agrees_with_a_dense_long_double_einsum(n, r):
    """The restatement lies within N_i u B_i of the true G_i (basis_core_grad_ref's derivation), that is within one half of the
    allowance 2 N_i u B_i.  The long-double einsum stands for the true value: its own error is the same count at u = 2^-64, below
    2^-10 of that half, which the factor (1 + 2^-10) takes in.  val is basis_ref.chain's bit for bit."""
    for nonneg in (False, True):
        cores, phis, c = _data(n, r, 5 + len(n), nonneg)
        val, G = C.core_grad_chain(cores, phis, c)
        assert np.array_equal(_bits(val), _bits(B.chain(cores, phis)))
        dense, bnd = C.dense_longdouble(cores, phis, c), C.bound(cores, phis, c)
        for i in range(len(n)):
            assert G[i].shape == cores[i].shape
            err = np.abs(G[i].astype(np.longdouble) - dense[i]).astype(np.float64)
            assert np.all(err <= 0.5 * (1.0 + 2.0 ** -10) * bnd[i]), (nonneg, i, float(np.max(err / bnd[i])))
            if nonneg:
                assert np.all(G[i] > 0.0) and np.array_equal(_bits(bnd[i]), _bits(2.0 * C.count(cores, i, NPTS) * B.U * G[i]))   # B_i is G_i itself


def test_count_is_the_formula_of_the_derivation():
    cores = R.rand_train(2, [3, 4, 2, 5], [1, 2, 70, 3, 1])
    assert C.count(cores, 0, 10) == (4 * 70 + 2) + (2 * 3 + 2) + (5 * 1 + 2) + 10 + 4
    assert C.count(cores, 2, 10) == (3 * 1 + 2) + (4 * 2 + 2) + (5 * 1 + 2) + 10 + 4
    assert C.count(cores, 3, 7) == (3 * 1 + 2) + (4 * 2 + 2) + (2 * 70 + 2) + 7 + 4


@pytest.mark.parametrize("n,r", SHAPES)
def test_accumulating_onto_g0_continues_the_same_sum(n, r):
    cores, phis, c = _data(n, r, 21, False)
    _, G = C.core_grad_chain(cores, phis, c)
    h = NPTS // 2
    _, G1 = C.core_grad_chain(cores, [p[:h] for p in phis], c[:h])
    _, G2 = C.core_grad_chain(cores, [p[h:] for p in phis], c[h:], g0=G1)
    for a, b in zip(G, G2):
        assert np.array_equal(_bits(a), _bits(b))
    # appended points with c = 0 and finite tables add (0 * L) * (phi * X) = +-0.0: the bits stay
    phis0 = [np.vstack([p, np.ones((3, p.shape[1]))]) for p in phis]
    _, G0 = C.core_grad_chain(cores, phis0, np.concatenate([c, np.zeros(3)]))
    for a, b in zip(G, G0):
        assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("n,r", SHAPES)
def test_linearity_identity_holds_on_the_restatement(n, r):
    """sum_p c_p f_(U_i <- E)(x_p) = <G_i, E> for a random block E, within identity_allowance (derived in basis_core_grad_ref)"""
    rng = np.random.default_rng(33)
    for nonneg in (False, True):
        cores, phis, c = _data(n, r, 17 + len(n), nonneg)
        _, G = C.core_grad_chain(cores, phis, c)
        Bi = C.abs_core_grad(cores, phis, c)
        for i in range(len(n)):
            E_ = rng.uniform(0.0, 1.0, cores[i].shape) if nonneg else rng.standard_normal(cores[i].shape)
            left, right = C.identity_sides(cores, phis, c, i, E_, G[i])
            allow = C.identity_allowance(cores, phis, c, i, E_, Bi[i])
            assert abs(left - right) <= allow, (nonneg, i, abs(left - right) / allow)
            if nonneg:
                assert left > 0.0 and abs(left - right) <= 1e-12 * left         # and the allowance is no empty promise: a dropped point shows
                worse = C.identity_sides(cores, [p[1:] for p in phis], c[1:], i, E_, G[i])[0]
                assert abs(worse - right) > allow


def test_block_coordinate_fit_in_numpy_lowers_the_loss_at_every_step():
    """pins the inputs of the GPU test: n = [5, 6, 4], r = [1, 3, 2, 1], 200 points, hat-function tables, 3 sweeps"""
    cores, phis, y = C.fit_problem()
    assert [u.shape for u in cores] == [(1, 5, 3), (3, 6, 2), (2, 4, 1)] and y.shape == (200,) and [p.shape[1] for p in phis] == [5, 6, 4]
    for p in phis:
        assert np.all(p >= 0.0) and np.allclose(p.sum(axis=1), 1.0, rtol=0, atol=4 * B.U) and np.all(np.count_nonzero(p, axis=1) <= 2)
    losses, fitted = C.fit_numpy()
    assert len(losses) == 3 * 3 + 1 and np.isfinite(losses).all()
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert losses[-1] < losses[0]
    again, _ = C.fit_numpy()
    assert again == losses                                                      # seeded: the sequence is a fixed list of doubles


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no host C++ compiler")
    return c


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_plan_of_a_core_gradient_call(cxx, tmp_path, flags):
    exe = str(tmp_path / "basis_core_grad_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "ttcross_amd", "csrc"), os.path.join(ROOT, "tests", "basis_core_grad_plan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"basis core grad plan: ok \((\d+) plans\)", r.stdout.strip()), r.stdout
    assert int(re.search(r"\((\d+) plans", r.stdout).group(1)) == (16 + 128 + 1) * 4 * 3 * 8 * 6 * 8
