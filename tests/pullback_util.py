"""Shared helpers of the tests of pulled-back integrands (TTX_FUN_PULLBACK; test_pullback_cpu.py, test_gpu_pullback.py,
pullback_grid_worker.py): layers of random trains, the chain of public sampler calls that DEFINES the result, the dense-table host
callback of tests/pullback_ref.c, the code object of the example combiner and its host evaluation."""
import ctypes
import os
import subprocess

import numpy as np

from trainfun_util import random_cores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
TEMPERED_SOURCE = os.path.join(ROOT, "examples", "devfun", "pullback_tempered.hip")
TEMPERED_PAR = [0.5, 0.4, 0.8, 2.0, 0.1]         # beta, mu, sigma, c, rho

_ref = None


def ref_lib():
    """tests/pullback_ref.c -> shared object; returns the CDLL."""
    global _ref
    if _ref is None:
        os.makedirs(BUILD, exist_ok=True)
        so, src = os.path.join(BUILD, "libpullback_ref.so"), os.path.join(ROOT, "tests", "pullback_ref.c")
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            tmp = so + f".{os.getpid()}"
            subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", tmp], check=True)
            os.replace(tmp, so)
        _ref = ctypes.CDLL(so)
        _ref.pullback_lookup.restype = ctypes.c_double
        _ref.pullback_table.restype = None
        _ref.pullback_table.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.c_int64]
    return _ref


def set_table(tab):
    """tab: the integrand over all multi-indices, row-major; the caller keeps the array alive while the callback is in use"""
    assert tab.dtype == np.float64 and tab.flags.c_contiguous
    ref_lib().pullback_table(tab.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), tab.size)


def lookup_addr():
    return ctypes.cast(ref_lib().pullback_lookup, ctypes.c_void_p).value


def all_indices(n):
    """every multi-index of the grid, 1-based, row-major (the last mode runs fastest): the order of pullback_ref.c's table"""
    g = np.meshgrid(*[np.arange(1, nk + 1) for nk in n], indexing="ij")
    return np.stack([a.ravel() for a in g], axis=1).astype(np.int32)


def unit_nodes(n, seed=None):
    """n strictly ascending nodes from exactly 0.0 to exactly 1.0; seed: uneven spacing"""
    if seed is None:
        t = np.arange(n) / (n - 1.0)
    else:
        t = np.concatenate([[0.0], np.cumsum(np.random.default_rng(seed).uniform(0.5, 1.5, size=n - 1))])
        t = t / t[-1]
    t[0], t[-1] = 0.0, 1.0
    return t


def box_nodes(n, lo, hi):
    t = lo + (hi - lo) * np.arange(n) / (n - 1.0)
    t[0], t[-1] = lo, hi
    return t


def make_layers(E, ns, ranks, gammas, seed, box=(-1.5, 2.0)):
    """m layers: layer t has mode sizes ns[t], ranks ranks[t] (a number or a list of d + 1) and gamma gammas[t]; layer 1's nodes span
    the box, the others run from 0 to 1 (uneven).  Returns [(train, nodes, gamma)]."""
    layers = []
    for t, (n, r, g) in enumerate(zip(ns, ranks, gammas)):
        x = E.TTCross.from_cores(random_cores(n, r, seed=seed + 11 * t))
        nodes = [box_nodes(nk, *box) if t == 0 else unit_nodes(nk, seed=seed + 100 * t + k) for k, nk in enumerate(n)]
        layers.append((x, nodes, g))
    return layers


def chain(layers, u):
    """THE DEFINITION: the chain of sample_sq_real(.., mode="exact") calls on the layers' own engines, m .. 1, on host arrays"""
    logq = val = None
    for x, nodes, gamma in reversed(layers):
        o = x.sample_sq_real(u, nodes, gamma=gamma, mode="exact", want=("x", "logq", "val"))
        u, val = o["x"], o["val"]
        logq = o["logq"] if logq is None else logq + o["logq"]
    return u, logq, val


def ref_points(ref, ind):
    return np.stack([np.asarray(ref[k])[ind[:, k] - 1] for k in range(ind.shape[1])], axis=1)


def random_indices(n, npts, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(1, nk + 1, size=npts) for nk in n], axis=1).astype(np.int32)


def same_bits(a, b):
    """np.array_equal with NaN equal to NaN: the doubles as bytes, but +0.0 and -0.0 told apart only where both are numbers"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def tempered_object():
    from ttcross_amd import engine as E
    os.makedirs(BUILD, exist_ok=True)
    return E.compile_device_fun(TEMPERED_SOURCE, os.path.join(BUILD, "pullback_tempered.hsaco"))


def tempered_host(x, logq, par=TEMPERED_PAR):
    """examples/devfun/pullback_tempered.hip on the host, operation by operation: sums from 0.0 over ascending k, separate multiplies
    and adds; a failed sample (NaN) gives 0.0"""
    beta, mu, sigma, c, rho = par
    s = np.zeros(x.shape[0])
    for k in range(x.shape[1]):
        z = (x[:, k] - mu) / sigma
        s = s + z * z
    b = x[:, 0] * x[:, 1] - rho
    logpi = -0.5 * s - c * (b * b)
    e = beta * logpi - logq
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(e), 0.0, np.sqrt(np.exp(e)))
