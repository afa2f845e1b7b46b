"""CPU tests of the COS-coefficient integrand (TTX_FUN_COSCOEFF): the header's own sin / cos against the run-time library, the
C restatement (ttcross_amd/csrc/ttx_coscoeff.h on the host) against the genuine reference's values, the oracle's sweep on it
against the reference's sweep log, and the refusals of ttx_create / ttx_k_eval that come before any device call."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import coscoeff_util as CU
import oracle_lib as O
from golden_util import GOLDEN, parse_log
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

TRIG_MAX = 2.0 ** 19          # TTX_TRIG_MAX


def _ulps(a, b):
    ia, ib = a.view(np.int64), b.view(np.int64)
    ia = np.where(ia < 0, np.int64(-2 ** 63) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2 ** 63) - ib, ib)
    return np.abs(ia - ib)


def test_sin_cos_within_one_ulp_of_libm():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(-TRIG_MAX, TRIG_MAX, 400000), rng.uniform(-64.0, 64.0, 300000),
                        rng.uniform(-1.0, 1.0, 300000) * np.exp2(rng.uniform(-40.0, 0.0, 300000))])
    assert x.size == 10 ** 6
    for f in ("sin", "cos"):
        u = _ulps(CU.vec("ttx_test_" + f, x), CU.vec("ttx_test_libm_" + f, x))
        assert u.max() <= 1, (f, x[np.argmax(u)])


def test_sin_cos_near_multiples_of_half_pi():
    """the hardest arguments of the reduction: the doubles nearest k pi/2 and their neighbours, k up to the range limit"""
    k = np.concatenate([np.arange(1, 2000), np.arange(2000, 333000, 97)]).astype(np.float64)
    x = k * (math.pi / 2)
    x = np.concatenate([x, np.nextafter(x, 0.0), np.nextafter(x, np.inf), np.nextafter(np.nextafter(x, 0.0), 0.0)])
    x = x[x <= TRIG_MAX]
    x = np.concatenate([x, -x])
    for f in ("sin", "cos"):
        u = _ulps(CU.vec("ttx_test_" + f, x), CU.vec("ttx_test_libm_" + f, x))
        assert u.max() <= 1, (f, x[np.argmax(u)])


def test_sin_cos_exact_symmetry_and_special_values():
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.uniform(0.0, TRIG_MAX, 100000), np.exp2(rng.uniform(-1060.0, 19.0, 100000))])
    assert np.array_equal(CU.vec("ttx_test_sin", -x).view(np.int64), (-CU.vec("ttx_test_sin", x)).view(np.int64))
    assert np.array_equal(CU.vec("ttx_test_cos", -x).view(np.int64), CU.vec("ttx_test_cos", x).view(np.int64))
    z = np.array([0.0, -0.0])
    assert np.array_equal(CU.vec("ttx_test_sin", z).view(np.int64), z.view(np.int64))           # sin(+-0) = +-0
    assert np.array_equal(CU.vec("ttx_test_cos", z), np.ones(2))
    tiny = np.array([5e-324, -5e-324, 2.2250738585072014e-308, 1e-300, 1e-20, -3e-9, 2.0 ** -27])
    assert np.array_equal(CU.vec("ttx_test_sin", tiny), tiny)                                     # sin x = x below 2^-26
    assert np.array_equal(CU.vec("ttx_test_cos", tiny), np.ones(tiny.size))


def test_restatement_matches_genuine_reference_values():
    """calc_coefficient of the genuine reference (tests/golden/coscoeff_values.txt) vs the C restatement: within 1e-14 of the
    sum of |terms| (glibc's sin / cos are not restated, so the two agree to rounding, not bit for bit)"""
    ref = CU.reference_values()
    assert sorted(ref) == [2, 4, 6, 10] and sum(v[0].shape[0] for v in ref.values()) == 2000
    for d, (ind, val) in ref.items():
        aux = D.coscoeff_setup(d, 65)["aux"]
        mine, mag = CU.host_values(d, aux, ind)
        assert (np.abs(mine - val) <= 1e-14 * mag).all(), (d, np.max(np.abs(mine - val) / mag))
        assert np.max(np.abs(val) / mag) > 0.1     # the set holds coefficients far from cancellation, not only cancelled ones


# leading sweeps of the reference's log the oracle (netlib-order linear algebra, this sin / cos) reproduces exactly: the whole log.
# The pivots of this integrand stay far above the rounding noise up to the rank limit (maxrank 20 is reached before the
# accuracy 500 eps), so a last-ulp difference of single elements does not re-route the pivot path.
EXACT_PREFIX = 20


def test_oracle_with_restatement_reproduces_reference_sweep_log():
    s = D.coscoeff_setup(6, 65)
    oo = O.dmrgg(s["n"], E.TTX_FUN_HOST, s["aux"], 20, piv=1, accuracy=s["acc"], user=CU.fun_addr())
    g_rows, _, g_neval = parse_log(open(os.path.join(GOLDEN, "coscoeff_6_65_20_1.txt")).read())
    assert len(g_rows) == len(oo["sweeps"])
    k = 0
    for a, b in zip(g_rows, oo["sweeps"]):
        if a["erank"] == round(b["erank"], 1) and a["neval"] == b["neval"]:
            k += 1
        else:
            break
    assert k >= EXACT_PREFIX, f"only {k} leading sweeps match the reference"
    assert g_neval == oo["neval"]




@pytest.mark.parametrize("case,match", [
    ("naux", "aux must hold"), ("nan", "not finite"), ("inf", "not finite"), ("a_ge_b", "lower bound"), ("a_eq_b", "lower bound"),
    ("d21", "at most 20 dimensions"), ("range_mu", "beyond the supported"), ("range_a", "beyond the supported"), ("noaux", "aux must hold")])
def test_create_refuses_invalid_coscoeff_problems(case, match):
    """each refusal is TTX_EINVAL before any device call (so it reads the same with or without a GPU)"""
    d, n = 4, 17
    aux = D.coscoeff_setup(d, n)["aux"].copy()
    nn = [n] * d
    if case == "naux":
        aux = aux[:-1]
    elif case == "nan":
        aux[d + 3] = np.nan
    elif case == "inf":
        aux[0] = np.inf
    elif case == "a_ge_b":
        aux[-2], aux[-1] = aux[-1], aux[-2]
    elif case == "a_eq_b":
        aux[-2] = aux[-1]
    elif case == "d21":
        d = 21
        aux = D.coscoeff_setup(d, 5)["aux"]
        nn = [5] * d
    elif case == "range_mu":
        aux[:d] = 1e5                 # |t'mu| up to about 4 * 6.3 * 1e5
    elif case == "range_a":
        aux[-2], aux[-1] = -3e4, -3e4 + 8.0
    elif case == "noaux":
        aux = None
    with pytest.raises(E.TTXError, match=match):
        E.TTCross(nn, E.TTX_FUN_COSCOEFF, [], 8, pivoting=1, accuracy=500 * D.EPS, aux=aux)
    if aux is not None:
        with pytest.raises(E.TTXError, match=match):
            E.k_eval(E.TTX_FUN_COSCOEFF, nn, [], np.ones((1, d), dtype=np.int32), aux=aux)


def test_create_accepts_valid_coscoeff_problem_up_to_the_device():
    """a valid problem (modes of different sizes, larger than the first: allowed, par is not indexed) passes every check;
    without a GPU it then fails for want of a device, with one it is created"""
    import torch
    s = D.coscoeff_setup(5, 17)
    try:
        tt = E.TTCross([9, 17, 33, 17, 5], E.TTX_FUN_COSCOEFF, [], 8, pivoting=1, accuracy=s["acc"], aux=s["aux"])
    except E.TTXError as e:
        assert not torch.cuda.is_available() and "no HIP device" in str(e)
    else:
        assert tt.fun_id == E.TTX_FUN_COSCOEFF
        tt.close()


@pytest.mark.parametrize("fun_id", [0, 4, 6, -1, 99])
def test_k_eval_refuses_unknown_ids_before_the_device(fun_id):
    s = D.coscoeff_setup(3, 9)
    with pytest.raises(E.TTXError, match="unknown fun_id"):
        E.k_eval(fun_id, s["n"], np.zeros(20), np.ones((2, 3), dtype=np.int32), aux=s["aux"])


def test_k_eval_refuses_indices_outside_the_modes():
    s = D.coscoeff_setup(3, 9)
    with pytest.raises(E.TTXError, match="outside"):
        E.k_eval(E.TTX_FUN_COSCOEFF, s["n"], [], np.array([[1, 10, 1]], dtype=np.int32), aux=s["aux"])


def test_driver_setup_mirrors_reference_parameter_block():
    s = D.coscoeff_setup(3, 64)
    assert s["n"] == [65] * 3 and s["acc"] == 500 * D.EPS and s["fun_id"] == E.TTX_FUN_COSCOEFF == 5
    mu, cov = s["aux"][:3], s["aux"][3:12].reshape(3, 3, order="F")
    assert (mu == math.log(100.0) - 0.5 * 0.4 ** 2).all()
    assert cov[0, 0] == 0.4 * 0.4 and cov[0, 1] == 0.4 * 0.5 * 0.4 and (cov == cov.T).all()
    assert s["aux"][-2:].tolist() == [0.525170185988090843, 8.52517018598809173]


def test_reference_driver_compiles_against_dropin():
    """the fork's test_crs_coscoeff.f90, unchanged, compiles and links against the drop-in modules and libttx.so"""
    ref = "/root/reference/test_crs_coscoeff.f90"
    fc = shutil.which("amdflang") or ("/opt/rocm/bin/amdflang" if os.path.exists("/opt/rocm/bin/amdflang") else None)
    if not os.path.exists(ref) or not fc:
        pytest.skip("the reference driver or amdflang is absent")
    from conftest import fortran_exe
    fortran_exe("test_crs_coscoeff")           # builds the drop-in layer (fails loudly if it does not build)
    fdir = os.path.join(CU.ROOT, "ttcross_amd", "fortran")
    bdir = os.path.join(fdir, "build")
    tmp = os.path.join(CU.ROOT, "tests", "_build", "coscoeff_ref")
    os.makedirs(tmp, exist_ok=True)
    objs = [os.path.join(bdir, f) for f in sorted(os.listdir(bdir)) if f.endswith(".o") and not f.startswith("test_")]
    p = subprocess.run([fc, "-O2", "-fopenmp", "-I" + bdir, "-I" + fdir, "-module-dir", tmp, ref] + objs +
                       ["-o", os.path.join(tmp, "dropin_test_crs_coscoeff"), "-L" + os.path.join(CU.ROOT, "ttcross_amd", "lib"), "-lttx",
                        "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib/llvm/lib"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
