"""Shared helpers of the device-integrand tests (test_devfun_cpu.py, test_gpu_devfun.py, devfun_mp_worker.py): code objects of
the example integrands under tests/_build/, the host C twins of tests/devfun_ref.c, the box set-up of the drivers."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
SOURCES = {"rational": os.path.join(ROOT, "examples", "devfun", "rational.hip"),
           "rational_wave": os.path.join(ROOT, "examples", "devfun", "rational_wave.hip"),
           "ising_c": os.path.join(ROOT, "examples", "devfun", "ising_c.hip"),
           "second": os.path.join(ROOT, "tests", "devfun_second.hip")}


def code_object(key):
    """tests/_build/<key>.hsaco: compiled when stale and a compiler is found, otherwise the file already there; neither: an
    error (compile_device_fun raises), never a skip."""
    from ttcross_amd import engine as E
    os.makedirs(BUILD, exist_ok=True)
    return E.compile_device_fun(SOURCES[key], os.path.join(BUILD, key + ".hsaco"))


def other_arch_object():
    """rational.hip compiled for ANOTHER GPU (gfx90a): a complete bundle without code for the MI355X, which the runtime refuses"""
    import shutil
    out = os.path.join(BUILD, "rational_gfx90a.hsaco")
    src = SOURCES["rational"]
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        os.makedirs(BUILD, exist_ok=True)
        subprocess.run([hipcc, "--genco", "--offload-arch=gfx90a", "-O3", "-I", os.path.join(ROOT, "include"), src, "-o", out], check=True)
    return out


_twins = None


def twins():
    """tests/devfun_ref.c -> shared object (no FP contraction); returns the CDLL."""
    global _twins
    if _twins is None:
        os.makedirs(BUILD, exist_ok=True)
        so, src = os.path.join(BUILD, "libdevfun_ref.so"), os.path.join(ROOT, "tests", "devfun_ref.c")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            tmp = so + f".{os.getpid()}"
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", tmp, "-lm"], check=True)
            os.replace(tmp, so)
        _twins = ctypes.CDLL(so)
        for f in ("ttx_devfun_rational", "ttx_devfun_second", "ttx_devfun_rational_nan", "ttx_devfun_rational_partnan"):
            getattr(_twins, f).restype = ctypes.c_double
    return _twins


def twin_addr(name):
    return ctypes.cast(getattr(twins(), name), ctypes.c_void_p).value


def twin_eval(name, n, par, ind):
    """The C twin at the multi-indices ind (npts x d, 1-based)."""
    f = getattr(twins(), name)
    n = np.ascontiguousarray(n, dtype=np.int32)
    par = np.ascontiguousarray(par, dtype=np.float64)
    ind = np.ascontiguousarray(ind, dtype=np.int32)
    m = ctypes.c_int32(n.size)
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    return np.array([f(ctypes.byref(m), ind[t].ctypes.data_as(ip), n.ctypes.data_as(ip), par.ctypes.data_as(dp)) for t in range(ind.shape[0])])


def user_setup(d, n):
    """nodes and weights on [0,1] (test_crs_box.inc with a=0, b=1), as the host-callback tests use"""
    from ttcross_amd import drivers as D
    x, w = D.lgwt(n)
    par = np.concatenate([0.5 * (x + 1.0), 0.5 * w])
    return dict(n=[n] * d, par=par, quad=[par[n:].copy()] * d, acc=500 * D.EPS)
