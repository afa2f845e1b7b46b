"""Shared by the COS-coefficient tests: the C restatement (tests/coscoeff_fun.c, built on first use) and the fixtures."""
import ctypes
import os
import subprocess

import numpy as np

from golden_util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def cclib():
    """tests/coscoeff_fun.c -> shared object, compiled like tests/userfun.c (no FP contraction)."""
    global _lib
    if _lib is None:
        bdir = os.path.join(ROOT, "tests", "_build")
        os.makedirs(bdir, exist_ok=True)
        so = os.path.join(bdir, "libcoscoeff.so")
        srcs = [os.path.join(ROOT, "tests", "coscoeff_fun.c")] + [os.path.join(ROOT, "ttcross_amd", "csrc", f)
                                                                  for f in ("ttx_coscoeff.h", "ttx_trig_coef.h", "ttx_exp.h", "ttx_exp_tab.h")]
        if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(s) for s in srcs):
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", srcs[0], "-o", so, "-lm"], check=True)
        _lib = ctypes.CDLL(so)
    return _lib


def fun_addr():
    """address of ttx_test_coscoeff(m, ind, n, par): the reference's callback interface, par = the engine's aux"""
    return ctypes.cast(cclib().ttx_test_coscoeff, ctypes.c_void_p).value


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def vec(name, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    getattr(cclib(), name)(ctypes.c_int64(x.size), _dp(x), _dp(out))
    return out


def host_values(d, aux, ind):
    """the C restatement at the rows of ind (1-based): (values, factor * sum over s of exp(-q/2))"""
    ind = np.ascontiguousarray(ind, dtype=np.int32)
    aux = np.ascontiguousarray(aux, dtype=np.float64)
    val, mag = np.empty(ind.shape[0]), np.empty(ind.shape[0])
    cclib().ttx_test_coscoeff_list(ctypes.c_int32(d), _dp(aux), ctypes.c_int64(ind.shape[0]),
                                   ind.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _dp(val), _dp(mag))
    return val, mag


def reference_values():
    """tests/golden/coscoeff_values.txt: {d: (indices, values)} of the genuine reference's calc_coefficient"""
    out = {}
    for line in open(os.path.join(GOLDEN, "coscoeff_values.txt")):
        t = line.split()
        d = int(t[0])
        out.setdefault(d, ([], []))
        out[d][0].append([int(x) for x in t[1:1 + d]])
        out[d][1].append(float(t[1 + d]))
    return {d: (np.array(a, dtype=np.int32), np.array(b)) for d, (a, b) in out.items()}
