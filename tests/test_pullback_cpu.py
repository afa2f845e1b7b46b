"""Pulled-back integrands (TTX_FUN_PULLBACK): what can be checked without a GPU -- the launch plan and every argument refusal that
needs no device (tests/pullback_plan_main.cpp, stand-alone, also under the host sanitizers), the C-ABI as declared and exported, the
example combiner's code object and its host evaluation, the dense-table callback of tests/pullback_ref.c."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import pullback_util as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no host C++ compiler")
    return c


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_plan_and_refusals_on_the_host(cxx, tmp_path, flags):
    """LDS per wave and waves per workgroup at (4, 2, 1), (128, 1025, 255) and the first size that no longer fits, the node-end rule,
    the ref range rule, every argument refusal of the set call"""
    exe = str(tmp_path / "pullback_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "ttcross_amd", "csrc"), os.path.join(ROOT, "tests", "pullback_plan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"pullback plan: ok \((\d+) checks\)", r.stdout.strip()), r.stdout
    assert int(re.search(r"\((\d+) checks", r.stdout).group(1)) > 40000


def _header():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))


def test_header_declares_the_entry_points_and_constants():
    h = _header()
    assert "typedef struct { ttx_engine *x; const double *const *nodes; double gamma; } ttx_layer;" in h
    assert ("int ttx_set_integrand_pullback (ttx_engine *h, int32_t m, const ttx_layer *layer, const double *const *ref , const void *image, int64_t nbytes, "
            "const char *name, const double *par, int32_t npar);") in h
    assert ("int ttx_set_integrand_pullback_file(ttx_engine *h, int32_t m, const ttx_layer *layer, const double *const *ref, const char *path, const char *name, "
            "const double *par, int32_t npar);") in h
    assert "int ttx_pullback_points(ttx_engine *h, int64_t npts, const int32_t *ind , double *x , double *logq, double *val);" in h
    assert "int ttx_pullback_last(const ttx_engine *h, double *ms, int64_t *launches, int64_t *elements, int64_t *nfailed);" in h
    for name, val in (("TTX_FUN_PULLBACK", 8), ("TTX_PULLBACK_MAX", 8)):
        assert re.search(rf"#define {name} +{val}\b", h), name


def test_library_exports_the_entry_points_and_version_stays_3():
    import __graft_entry__ as g
    L = ctypes.CDLL(g.build_lib())
    for sym in ("ttx_set_integrand_pullback", "ttx_set_integrand_pullback_file", "ttx_pullback_points", "ttx_pullback_last"):
        assert hasattr(L, sym), sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() == 3


def test_engine_module_mirrors_the_constants():
    from ttcross_amd import engine as E
    assert (E.TTX_FUN_PULLBACK, E.TTX_PULLBACK_MAX) == (8, 8)
    assert all(callable(getattr(E.TTCross, f)) for f in ("pullback", "set_integrand_pullback", "pullback_points", "pullback_last"))
    assert callable(E.transport_sample) and callable(E.transport_rosenblatt)
    assert ctypes.sizeof(E._Layer) == 24


def test_example_combiner_compiles_to_a_code_object_with_the_combiner_symbols():
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    blob = open(P.tempered_object(), "rb").read()
    for sym in (b"ttx_devcomb_info_pullback_tempered", b"ttx_devcomb_slots_pullback_tempered", b"ttx_devcomb_list_pullback_tempered"):
        assert sym in blob, sym


def test_host_evaluation_of_the_example():
    """the host restatement against the formula written another way, and the failed row"""
    rng = np.random.default_rng(1)
    x, lq = rng.uniform(-1, 2, size=(50, 4)), rng.uniform(-3, 1, size=50)
    beta, mu, sigma, c, rho = P.TEMPERED_PAR
    logpi = -0.5 * (((x - mu) / sigma) ** 2).sum(axis=1) - c * (x[:, 0] * x[:, 1] - rho) ** 2
    got = P.tempered_host(x, lq)
    assert np.allclose(got, np.exp(0.5 * (beta * logpi - lq)), rtol=1e-13, atol=0.0)
    x[3, :] = np.nan
    lq[3] = np.nan
    assert P.tempered_host(x, lq)[3] == 0.0


def test_table_callback_walks_the_table_row_major():
    n = np.array([3, 4, 2], dtype=np.int32)
    ind = P.all_indices(n)
    assert ind.shape == (24, 3) and ind[0].tolist() == [1, 1, 1] and ind[1].tolist() == [1, 1, 2] and ind[-1].tolist() == [3, 4, 2]
    tab = np.arange(24, dtype=np.float64) + 0.5
    P.set_table(tab)
    f = P.ref_lib().pullback_lookup
    ip, m = ctypes.POINTER(ctypes.c_int32), ctypes.c_int32(3)
    got = [f(ctypes.byref(m), ind[p].ctypes.data_as(ip), n.ctypes.data_as(ip), None) for p in range(24)]
    assert got == tab.tolist()
    bad = np.array([1, 5, 1], dtype=np.int32)
    assert f(ctypes.byref(m), bad.ctypes.data_as(ip), n.ctypes.data_as(ip), None) == -3.0
