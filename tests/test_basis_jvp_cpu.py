"""The derivative along a direction in core space, the vector operations on packed buffers and the Gauss-Newton solver
(ttx_basis_jvp_batch, ttx_cores_dot, ttx_basis_fit_batch and their siblings): what can be checked without a GPU -- the numpy
restatements (tests/basis_jvp_ref.py) against a dense long-double einsum, against basis_ref.chain, against the adjoint identity with
basis_core_grad_ref and against homogeneity; the C ABI as declared and exported; the plan of a call (tests/basis_jvp_plan_main.cpp)
and the controller on a dense backend (tests/fit_plan_main.cpp), both plain and under the sanitizers as stand-alone host programs;
and the pinned solver runs that the GPU tests repeat."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import basis_core_grad_ref as C
import basis_jvp_ref as J
import basis_ref as B
import tt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ttx_basis_jvp_batch", "ttx_basis_jvp_batch_dev", "ttx_basis_jvp_tab", "ttx_basis_jvp_tab_dev", "ttx_basis_jvp_last", "ttx_cores_dot",
           "ttx_cores_dot_dev", "ttx_cores_axpby_dev", "ttx_cores_get", "ttx_cores_set", "ttx_cores_get_dev", "ttx_cores_set_dev", "ttx_basis_fit_batch",
           "ttx_basis_fit_batch_dev", "ttx_basis_fit_tab", "ttx_basis_fit_tab_dev", "ttx_basis_fit_last")
SHAPES = [([7, 2, 51, 1, 9], [1, 3, 17, 5, 4, 1]), ([3, 4, 2, 5], [1, 2, 70, 3, 1]), ([5, 7], [1, 3, 1]), ([5], [1, 1])]
NPTS = 23


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _data(n, r, seed, nonneg, npts=NPTS):
    rng = np.random.default_rng(seed)
    if nonneg:
        cores = [rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1])) for k in range(len(n))]
        return cores, [rng.uniform(0.0, 1.0, (npts, nk)) for nk in n], [rng.uniform(0.0, 1.0, u.shape) for u in cores], rng.uniform(0.0, 1.0, npts)
    cores = R.rand_train(seed, n, r)
    return cores, [rng.standard_normal((npts, nk)) for nk in n], [rng.standard_normal(u.shape) for u in cores], rng.standard_normal(npts)


def test_header_and_library_declare_the_entry_points():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        raw = f.read()
    h = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw, flags=re.S))
    for decl in ("int ttx_basis_jvp_batch (ttx_engine *h, int64_t npts, const double *x , const ttx_basis *basis , const double *v, double *val, double *dval, int32_t mode);",
                 "int ttx_basis_jvp_tab_dev (ttx_engine *h, int64_t npts, const double *phi_dev, const double *v_dev, double *val_dev, double *dval_dev, int32_t mode);",
                 "int ttx_cores_dot (ttx_engine *h, const double *a, const double *b, double *out);",
                 "int ttx_cores_axpby_dev(ttx_engine *h, double alpha, const double *x_dev, double beta, double *y_dev);",
                 "int ttx_cores_get_dev (ttx_engine *h, double *g_dev);", "int ttx_cores_set_dev (ttx_engine *h, const double *g_dev);",
                 "typedef struct { int32_t max_iter, cg_max, max_reject, mode; double lambda0, lambda_down, lambda_up, cg_tol, loss_tol; } ttx_fit_opts;",
                 "typedef struct { int32_t iters, stop; } ttx_fit_result;",
                 "int ttx_basis_fit_last (const ttx_engine *h, double *ms_jvp, double *ms_core_grad, double *ms_value, double *ms_vector, int64_t *n_jvp, int64_t *n_core_grad, int32_t *mode_ran);"):
        assert decl in h, decl
    assert "a Gauss-Newton or ALS solver" not in re.sub(r"\s*\n \*\s*", " ", raw)           # no longer on the open list of ttx_basis_core_grad_batch
    with open(os.path.join(ROOT, "ttcross_amd", "csrc", "ttx_op_plan.h")) as f:
        plan = f.read()
    assert re.search(r"PROVISIONAL, NOT MEASURED[^\n]*\n[^\n]*\n#define TTX_JV_AUTO_FLOPS TTX_BS_AUTO_FLOPS", plan)
    import __graft_entry__ as g
    L = ctypes.CDLL(g.build_lib())
    for sym in ENTRIES:
        assert hasattr(L, sym), sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() == 3                                                 # added without a new version
    from ttcross_amd import engine as E
    assert ctypes.sizeof(E._FitOpts) == 56 and ctypes.sizeof(E._FitResult) == 8


@pytest.mark.parametrize("n,r", SHAPES)
def test_jvp_chain_against_long_double_the_value_chain_the_adjoint_and_homogeneity(n, r):
    d = len(n)
    for nonneg in (False, True):
        cores, phis, V, c = _data(n, r, 29 + d, nonneg)
        val, dval = J.jvp_chain(cores, phis, V)
        assert np.array_equal(_bits(val), _bits(B.chain(cores, phis)))          # the z half is the value chain, bit for bit
        dense = J.dense_longdouble(cores, phis, V)
        bnd = J.bound(cores, phis, V)
        assert np.all(np.abs(dval - dense.astype(np.float64)) <= bnd), nonneg
        if nonneg:
            assert np.all(dval > 0.0) and np.all(bnd <= 2 * J.count(cores) * B.U * dval * (1 + 1e-9))
            assert not np.all(np.abs(J.jvp_chain(cores, phis, [v if k else 0 * v for k, v in enumerate(V)])[1] - dense.astype(np.float64)) <= bnd)     # a dropped term shows
        # the adjoint identity against the core gradient's restatement
        _, G = C.core_grad_chain(cores, phis, c)
        left, right = float(np.sum(c * dval)), float(sum(np.sum(g * v) for g, v in zip(G, V)))
        allow = J.adjoint_allowance(cores, phis, c, V, C.abs_core_grad(cores, phis, c))
        assert abs(left - right) <= allow, (nonneg, abs(left - right) / allow)
        if nonneg:
            assert left > 0.0 and allow < 1e-10 * left
        # f is homogeneous of degree d in the cores
        _, dh = J.jvp_chain(cores, phis, cores)
        assert np.all(np.abs(dh - d * val) <= J.homogeneity_allowance(cores, phis)), nonneg
        # a block direction is the chain of the replaced train
        for i in range(d):
            Vi = [v if k == i else np.zeros(v.shape) for k, v in enumerate(V)]
            rep = C.replaced(cores, i, V[i])
            assert np.all(np.abs(J.jvp_chain(cores, phis, Vi)[1] - B.chain(rep, phis)) <= J.bound(cores, phis, Vi) + B.bound(rep, phis))


def test_dot_and_axpby_restatements():
    rng = np.random.default_rng(4)
    for tot in (1, 59, 255, 256, 257, 65535, 65536, 65537, 200000):
        a, b = rng.standard_normal(tot), rng.standard_normal(tot)
        s = J.dot(a, b)
        assert abs(s - float(np.sum(a.astype(np.longdouble) * b.astype(np.longdouble)))) <= 2.0 * (tot + 1) * B.U * float(np.sum(np.abs(a * b)))
        assert J.dot(np.ones(tot), np.ones(tot)) == float(tot)
    assert J.dot_seg(65536) == 256 and J.dot_seg(65537) == 512 and J.dot_seg(1) == 256
    # the order is the stated one: 600 elements in segments of 256, one element per lane -- checked against a scalar loop
    a, b = rng.standard_normal(600), rng.standard_normal(600)
    L = J.dot_seg(600)
    assert L == 256
    segs = []
    for s0 in range(0, 256 * L, L):
        lane = [0.0 + (float(a[s0 + t]) * float(b[s0 + t])) if s0 + t < 600 else 0.0 for t in range(256)]
        h = 128
        while h >= 1:
            lane = [lane[t] + lane[t + h] for t in range(h)]
            h //= 2
        segs.append(lane[0])
    total = 0.0
    for v in segs:
        total = total + v
    assert _bits(total) == _bits(J.dot(a, b))
    x, y = rng.standard_normal(100), rng.standard_normal(100)
    assert np.array_equal(_bits(J.axpby(0.3, x, -1.7, y)), _bits(np.array([(0.3 * float(u)) + (-1.7 * float(v)) for u, v in zip(x, y)])))
    blocks = [rng.standard_normal((1, 3, 2)), rng.standard_normal((2, 4, 1))]
    assert all(np.array_equal(u, w) for u, w in zip(J.unpack(J.pack(blocks), [u.shape for u in blocks]), blocks))
    assert J.pack(blocks)[1] == blocks[0][0, 1, 0]                               # (a, j, k) at a + r0 (j + n k)


def test_the_numpy_solver_on_the_pinned_problems():
    """pins what the GPU tests repeat: from the random start of fit_problem() with lambda0 = 1, cg_max = 40, cg_tol = 1e-2 six
    iterations show accepted and rejected steps (iterations 0 and 1 accepted, 2 and 3 rejected, as the prototype of the solver
    showed: lambda0 did not have to move); from the truth perturbed by 10 % the loss falls below 1e-20 of its start in 12"""
    start, phis, y = C.fit_problem()
    h = J.fit_numpy(start, phis, y, max_iter=6, lambda0=1.0, cg_max=40, cg_tol=1e-2)
    assert h["accepted"].tolist()[:4] == [1, 1, 0, 0] and h["iters"] == 6 and h["stop"] == 1
    assert h["lambda_"].tolist()[:5] == [1.0, 0.3, 0.3 * 0.3, (0.3 * 0.3) * 4.0, ((0.3 * 0.3) * 4.0) * 4.0]
    assert np.all(h["loss"][1:] <= h["loss"][:-1]) and h["loss"][2] == h["loss"][3] == h["loss"][4] and h["loss"][-1] < h["loss"][0]
    assert h["n_jvp"] == int(h["cg_iters"].sum()) and h["n_core_grad"] == h["n_jvp"] + 1 + int(h["accepted"][:-1].sum())
    res = B.chain(h["cores"], phis) - y
    assert _bits(0.5 * J.dot(res, res)) == _bits(h["loss"][-1])
    for seed in (1, 2, 3):
        g = J.fit_numpy(J.perturbed_truth(seed), phis, y, max_iter=12, lambda0=1e-2, cg_max=60, cg_tol=1e-3)
        assert np.all(g["loss"][1:] <= g["loss"][:-1]) and 0.1 < g["loss"][0] < 2.0 and g["loss"][-1] <= 1e-28 * g["loss"][0], (seed, g["loss"])
    # stop reasons of the restatement: the tolerance, a non-finite loss, a zero gradient
    assert J.fit_numpy(start, phis, y, max_iter=3, loss_tol=100.0)["stop"] == 2
    yn = y.copy()
    yn[7] = np.nan
    assert J.fit_numpy(start, phis, yn, max_iter=3)["stop"] == 5
    assert J.fit_numpy([0 * start[0], start[1], 0 * start[2]], phis, y, max_iter=3)["stop"] == 3
    # weights: w = 0 on half the points, the masked targets change no bit
    w = (np.arange(y.size) % 2 == 0).astype(np.float64)
    y2 = y.copy()
    y2[w == 0.0] = 17.0
    a, b = (J.fit_numpy(start, phis, yy, w, max_iter=2) for yy in (y, y2))
    assert np.array_equal(_bits(a["loss"]), _bits(b["loss"])) and all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a["cores"], b["cores"]))


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no host C++ compiler")
    return c


def _build_and_run(cxx, tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "ttcross_amd", "csrc"), os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip()


SAN = [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]]


@pytest.mark.parametrize("flags", SAN, ids=["plain", "sanitizers"])
def test_plan_of_a_jvp_call(cxx, tmp_path, flags):
    out = _build_and_run(cxx, tmp_path, flags, "basis_jvp_plan_main")
    assert re.fullmatch(r"basis jvp plan: ok \((\d+) plans\)", out), out
    assert int(re.search(r"\((\d+) plans", out).group(1)) == (13 + 128 + 1) * 4 * 3 * 8 * 6


@pytest.mark.parametrize("flags", SAN, ids=["plain", "sanitizers"])
def test_the_controller_on_a_dense_backend(cxx, tmp_path, flags):
    assert _build_and_run(cxx, tmp_path, flags, "fit_plan_main") == "fit plan: ok"
