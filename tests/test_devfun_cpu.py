"""Loadable device integrands (TTX_FUN_DEVICE), the part that needs no GPU: the example sources and a minimal user file compile
for gfx950 against include/ttx_device_fun.h alone, the host C twins equal an independent numpy restatement, and the entry
points exist in libttx.so and in the Python layer."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import devfun_util as U
from conftest import ROOT
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
needs_hipcc = pytest.mark.skipif(HIPCC is None, reason="no hipcc on this box")


def _symbols(path):
    """dynamic symbols of the gfx950 code object inside the offload bundle hipcc --genco wrote"""
    blob = open(path, "rb").read()
    at = blob.find(b"\x7fELF", 24)                       # the device ELF behind the bundle header
    assert blob.startswith(b"__CLANG_OFFLOAD_BUNDLE__") and at > 0
    return blob[at:]


@needs_hipcc
@pytest.mark.parametrize("key,names", [("rational", ["rational", "rational_nan", "rational_partnan"]), ("rational_wave", ["rational_wave"]),
                                       ("ising_c", ["ising_c"]), ("second", ["second", "greedy", "future"])])
def test_example_sources_compile_for_gfx950(key, names, tmp_path):
    out = E.compile_device_fun(U.SOURCES[key], str(tmp_path / (key + ".hsaco")))
    elf = _symbols(out)
    for nm in names:
        for sym in ("ttx_devfun_slots_", "ttx_devfun_list_", "ttx_devfun_info_"):
            assert (sym + nm).encode() in elf, sym + nm
    # stale check: a second call does not rebuild
    t = os.path.getmtime(out)
    assert E.compile_device_fun(U.SOURCES[key], out) == out and os.path.getmtime(out) == t


@needs_hipcc
def test_minimal_user_file_needs_only_the_header(tmp_path):
    """What we ship to users: the header next to hip_runtime.h and nothing else of this repository."""
    inc = tmp_path / "inc"
    inc.mkdir()
    shutil.copy(os.path.join(ROOT, "include", "ttx_device_fun.h"), inc / "ttx_device_fun.h")
    src = tmp_path / "mine.hip"
    src.write_text('#include "ttx_device_fun.h"\n'
                   "__device__ double mine(int d, ttx_ind ind, const int *n, const double *par)\n"
                   "{ double s = 0.0; for (int k = 1; k <= d; k++) s = s + par[ind(k) - 1] * (double)n[k - 1]; return s; }\n"
                   "TTX_DEVICE_INTEGRAND(mine)\n"
                   "__device__ double minew(int d, ttx_ind ind, const int *n, const double *par, int lane)\n"
                   "{ return par[ind[lane % d] - 1]; }\n"
                   "TTX_DEVICE_INTEGRAND_WAVE(minew)\n")
    p = subprocess.run([HIPCC, "--genco", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I", str(inc), str(src), "-o", str(tmp_path / "mine.hsaco")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    assert b"ttx_devfun_slots_minew" in _symbols(str(tmp_path / "mine.hsaco"))


@needs_hipcc
def test_compile_failure_carries_the_compiler_message(tmp_path):
    src = tmp_path / "broken.hip"
    src.write_text('#include "ttx_device_fun.h"\n__device__ double broken(int d) { return undeclared_thing; }\n')
    with pytest.raises(E.TTXError, match="undeclared_thing"):
        E.compile_device_fun(str(src))


def test_c_twins_against_numpy():
    rng = np.random.default_rng(11)
    for d, n in [(2, 5), (7, 9), (24, 17)]:
        s = U.user_setup(d, n)
        ind = rng.integers(1, n + 1, size=(300, d)).astype(np.int32)
        x = s["par"][ind - 1]
        s1, s2, t = np.zeros(300), np.zeros(300), np.ones(300)
        for i in range(d):                              # left to right, one rounding per operation as in the C code
            s1 = s1 + x[:, i]
            s2 = s2 + x[:, i] * x[:, i]
            t = t + float(i + 1) * x[:, i]
        assert np.array_equal(U.twin_eval("ttx_devfun_rational", s["n"], s["par"], ind), s1 / (1.0 + s2))
        assert np.array_equal(U.twin_eval("ttx_devfun_second", s["n"], s["par"], ind), 1.0 / t)
        pn = U.twin_eval("ttx_devfun_rational_partnan", s["n"], s["par"], ind)
        bad = (ind[:, 0] == 2) | (ind[:, -1] == 1)
        assert np.isnan(pn[bad]).all() and np.array_equal(pn[~bad], (s1 / (1.0 + s2))[~bad])
        assert np.isnan(U.twin_eval("ttx_devfun_rational_nan", s["n"], s["par"], ind)).all()


def test_entry_points_exist():
    """Fails on an engine without the feature: the symbols of include/ttx.h and their Python wrappers."""
    so = E.lib_path()
    if not os.path.exists(so):
        pytest.skip("libttx.so not built on this box")
    L = ctypes.CDLL(so)
    for sym in ("ttx_set_integrand_device", "ttx_set_integrand_device_file", "ttx_eval_device"):
        assert hasattr(L, sym), sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() >= 2
    assert E.TTX_FUN_DEVICE == 6
    for attr in ("set_integrand_device", "eval_device"):
        assert callable(getattr(E.TTCross, attr))
    assert callable(E.compile_device_fun)
    hdr = open(os.path.join(ROOT, "include", "ttx.h")).read()
    assert "#define TTX_FUN_DEVICE 6" in hdr and "ttx_eval_device" in hdr
    assert "TTX_DEVFUN_ABI 1" in open(os.path.join(ROOT, "include", "ttx_device_fun.h")).read()


def test_devfun_driver_setup():
    s = D.devfun_setup(6, 64)
    assert s["n"] == [65] * 6 and s["par"].size == 2 * 65 + 1 and s["fun_id"] == E.TTX_FUN_DEVICE
    assert abs(sum(s["quad"][0]) - 1.0) < 1e-14
