"""Shared helpers of the tests of integrands of trains (TTX_FUN_TRAINS; test_trainfun_cpu.py, test_gpu_trainfun.py,
trainfun_nan_worker.py): the host twins of tests/trainfun_ref.c, random operand trains, the code object of the example combiner,
the bit-for-bit comparison of two runs."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
COMB_SOURCE = os.path.join(ROOT, "examples", "devfun", "comb_rational.hip")
TWIN_OF = {"product": "trainfun_product", "ratio": "trainfun_ratio", "sqrtabs": "trainfun_sqrtabs", "comb_rational": "trainfun_comb_rational"}

_twins = None


def twins():
    """tests/trainfun_ref.c -> shared object (no FP contraction); returns the CDLL."""
    global _twins
    if _twins is None:
        os.makedirs(BUILD, exist_ok=True)
        so, src = os.path.join(BUILD, "libtrainfun_ref.so"), os.path.join(ROOT, "tests", "trainfun_ref.c")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            tmp = so + f".{os.getpid()}"
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", tmp, "-lm"], check=True)
            os.replace(tmp, so)
        _twins = ctypes.CDLL(so)
        for f in list(TWIN_OF.values()) + ["trainfun_element"]:
            getattr(_twins, f).restype = ctypes.c_double
        _twins.trainfun_count.restype = None
    return _twins


def twin_set(trains):
    """The twin's table: trains = list of core lists ((r0, n, r1) arrays); sets the operand count too."""
    L = twins()
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    for t, cores in enumerate(trains):
        cores = [np.asarray(c, dtype=np.float64) for c in cores]
        n = np.array([c.shape[1] for c in cores], dtype=np.int32)
        r = np.array([cores[0].shape[0]] + [c.shape[2] for c in cores], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([c.ravel(order="F") for c in cores]))
        assert L.trainfun_set(t, len(cores), n.ctypes.data_as(ip), r.ctypes.data_as(ip), flat.ctypes.data_as(dp)) == 0
    L.trainfun_count(len(trains))


def twin_addr(name):
    return ctypes.cast(getattr(twins(), TWIN_OF.get(name, name)), ctypes.c_void_p).value


def twin_eval(name, n, ind, par=None):
    """The twin callback at the multi-indices ind (npts x d, 1-based)."""
    f = getattr(twins(), TWIN_OF.get(name, name))
    n = np.ascontiguousarray(n, dtype=np.int32)
    par = np.ascontiguousarray([0.0] if par is None else par, dtype=np.float64)
    ind = np.ascontiguousarray(ind, dtype=np.int32)
    m = ctypes.c_int32(n.size)
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    return np.array([f(ctypes.byref(m), ind[t].ctypes.data_as(ip), n.ctypes.data_as(ip), par.ctypes.data_as(dp)) for t in range(ind.shape[0])])


def twin_element(t, ind):
    f = twins().trainfun_element
    ind = np.ascontiguousarray(ind, dtype=np.int32)
    return np.array([f(ctypes.c_int(t), ind[p].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) for p in range(ind.shape[0])])


def random_cores(n, r, seed, positive=False):
    """cores (r[k], n[k], r[k+1]) with entries uniform in (-1, 1), or in (0.3, 0.9) where a ratio or a root needs a sign"""
    rng = np.random.default_rng(seed)
    r = [int(r)] * (len(n) + 1) if np.isscalar(r) else list(r)
    r[0] = r[-1] = 1
    lo, hi = (0.3, 0.9) if positive else (-1.0, 1.0)
    return [np.asfortranarray(rng.uniform(lo, hi, size=(r[k], n[k], r[k + 1]))) for k in range(len(n))]


def random_indices(n, npts, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(1, nk + 1, size=npts) for nk in n], axis=1).astype(np.int32)


def cores_of(tt):
    return [tt.core(k) for k in range(1, tt.d + 1)]


def comb_object():
    """tests/_build/comb_rational.hsaco (compile_device_fun: compiled when stale, an error without a compiler and a file)"""
    from ttcross_amd import engine as E
    os.makedirs(BUILD, exist_ok=True)
    return E.compile_device_fun(COMB_SOURCE, os.path.join(BUILD, "comb_rational.hsaco"))


def box_quad(n):
    """Gauss-Legendre weights on [0,1] per mode (any mode sizes)"""
    from ttcross_amd import drivers as D
    return [0.5 * D.lgwt(int(nk))[1] for nk in n]


def same_run(tt, oo, d, quad):
    """tapes, per-sweep records, ranks, cores and integral of an engine equal those of an oracle result (bit for bit); the lines
    of test_gpu_devfun._same_run"""
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d])
    for f in ("neval", "val", "amax"):
        assert [a[f] for a in tt.sweeps()] == [b[f] for b in oo["sweeps"]], f
    assert tt.neval == oo["neval"]
    assert np.array_equal(tt.ranks(), oo["r"])
    assert all(np.array_equal(tt.core(k), oo["cores"][k - 1]) for k in range(1, d + 1))
    assert tt.quad(quad) == oo["value"]


def as_result(tt, d, quad):
    return dict(tapes=tt.tapes(), sweeps=tt.sweeps(), neval=tt.neval, r=tt.ranks(), cores=[tt.core(k) for k in range(1, d + 1)], value=tt.quad(quad))
