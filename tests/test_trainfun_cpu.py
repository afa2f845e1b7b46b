"""Integrands of resident trains (TTX_FUN_TRAINS): what can be checked without a GPU -- the C-ABI as declared and exported, the host
twin of tests/trainfun_ref.c against tests/tt_ref.py, the example combiner's code object, the oracle driven by the twin."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import trainfun_util as T
import tt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))


def test_header_declares_the_entry_points_and_constants():
    h = _header()
    assert "int ttx_set_integrand_trains(ttx_engine *h, int32_t m, ttx_engine *const *x, int32_t op);" in h
    assert "int ttx_set_integrand_trains_device(ttx_engine *h, int32_t m, ttx_engine *const *x, const void *image, int64_t nbytes, const char *name, const double *par, int32_t npar);" in h
    assert "int ttx_set_integrand_trains_device_file(ttx_engine *h, int32_t m, ttx_engine *const *x, const char *path, const char *name, const double *par, int32_t npar);" in h
    assert "int ttx_trainfun_last(const ttx_engine *h, double *ms, int64_t *launches, int64_t *elements);" in h
    for name, val in (("TTX_FUN_TRAINS", 7), ("TTX_TRAINS_MAX", 8), ("TTX_TOP_PRODUCT", 1), ("TTX_TOP_RATIO", 2), ("TTX_TOP_SQRTABS", 3), ("TTX_TOP_DEVICE", 4)):
        assert re.search(rf"#define {name} +{val}\b", h), name


def test_library_exports_the_entry_points_and_version_stays_3():
    import __graft_entry__ as g
    L = ctypes.CDLL(g.build_lib())
    for sym in ("ttx_set_integrand_trains", "ttx_set_integrand_trains_device", "ttx_set_integrand_trains_device_file", "ttx_trainfun_last"):
        assert hasattr(L, sym), sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() == 3


def test_engine_module_mirrors_the_constants():
    from ttcross_amd import engine as E
    assert (E.TTX_FUN_TRAINS, E.TTX_TRAINS_MAX) == (7, 8)
    assert (E.TTX_TOP_PRODUCT, E.TTX_TOP_RATIO, E.TTX_TOP_SQRTABS, E.TTX_TOP_DEVICE) == (1, 2, 3, 4)
    assert callable(E.TTCross.of_trains) and callable(E.TTCross.set_integrand_trains) and callable(E.TTCross.trainfun_last)


@pytest.mark.parametrize("n,r", [([5, 4], [1, 3, 1]), ([3, 9, 2], [1, 2, 2, 1]), ([3, 5, 2, 7, 4, 6, 3, 5], [1, 3, 17, 64, 65, 9, 128, 2, 1]), ([5] * 40, 2)],
                         ids=["d2", "d3", "edge_64_65_128", "d40"])
def test_twin_elements_within_the_chain_bound_of_the_reference(n, r):
    """|twin - true| <= sum_k (r_k + 1) u B for any summation order of the chain (u = 2^-53, B the chain on |cores|); the same for
    tt_ref.element, so the two differ by at most twice that -- the bound test_gpu_tijk_batch.py derives."""
    cores = T.random_cores(n, r, seed=len(n))
    T.twin_set([cores])
    ind = T.random_indices(n, 200, seed=7)
    got = T.twin_element(0, ind)
    rr = [cores[0].shape[0]] + [c.shape[2] for c in cores]
    ab = [np.abs(c) for c in cores]
    for p in range(ind.shape[0]):
        ref, B = R.element(cores, ind[p]), R.element(ab, ind[p])
        assert abs(got[p] - ref) <= 2.0 * sum(rk + 1 for rk in rr) * 2.0 ** -53 * B, (p, got[p], ref)


def test_twin_combiners_apply_the_ops_in_the_written_order():
    n = [4, 3, 5]
    a, b, c = (T.random_cores(n, 2, seed=s, positive=True) for s in (1, 2, 3))
    ind = T.random_indices(n, 50, seed=3)
    T.twin_set([a, b, c])
    va, vb, vc = (T.twin_element(t, ind) for t in range(3))
    assert np.array_equal(T.twin_eval("product", n, ind), va * vb * vc)
    T.twin_set([a, b])
    assert np.array_equal(T.twin_eval("ratio", n, ind), va / vb)
    assert np.array_equal(T.twin_eval("comb_rational", n, ind, [0.125]), va / (1.0 + vb * vb) + 0.125 * ind[:, 0])
    T.twin_set([a])
    assert np.array_equal(T.twin_eval("sqrtabs", n, ind), np.sqrt(np.abs(va)))


def test_comb_rational_compiles_and_exports_the_three_symbols(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = tmp_path / "comb_rational.hsaco"
    subprocess.run([hipcc, "--genco", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), T.COMB_SOURCE, "-o", str(out)], check=True)
    blob = out.read_bytes()
    for sym in (b"ttx_devcomb_info_comb_rational", b"ttx_devcomb_slots_comb_rational", b"ttx_devcomb_list_comb_rational"):
        assert sym in blob, sym


def test_oracle_with_the_twin_callback_repeats():
    """case (5, 17, 10, 2, 1), the product of two random trains: two oracle runs with identical logs"""
    from ttcross_amd import drivers as D
    n = [17] * 5
    T.twin_set([T.random_cores(n, 4, seed=11), T.random_cores(n, 3, seed=12)])
    quad = T.box_quad(n)
    a = O.dmrgg(n, 4, [0.0], 10, piv=2, accuracy=500 * D.EPS, quad=quad, user=T.twin_addr("product"))
    b = O.dmrgg(n, 4, [0.0], 10, piv=2, accuracy=500 * D.EPS, quad=quad, user=T.twin_addr("product"))
    assert len(a["sweeps"]) >= 2 and np.array_equal(a["tapes"], b["tapes"])
    for f in ("neval", "val", "amax", "pivotmax", "pivotmin"):
        assert [s[f] for s in a["sweeps"]] == [s[f] for s in b["sweeps"]], f
    assert a["value"] == b["value"] and all(np.array_equal(x, y) for x, y in zip(a["cores"], b["cores"]))
