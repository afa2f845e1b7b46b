"""GPU tests of the COS-coefficient integrand on the device (TTX_FUN_COSCOEFF): the element evaluator against the C restatement
bit for bit, and whole sweeps -- which run the host integrand's two passes with k_coscoeff_slots between them -- against the
oracle and against the engine's own host-callback run bit for bit.  Every test first creates an engine with fun_id = 5, which a
library without this integrand refuses on the host (TTX_EINVAL) before anything reaches the device."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import coscoeff_util as CU
import oracle_lib as O
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

pytestmark = pytest.mark.gpu
ROOT = CU.ROOT


def _engine(d, n, r, piv, groups=1, **kw):
    s = D.coscoeff_setup(d, n)
    tt = E.TTCross(s["n"], E.TTX_FUN_COSCOEFF, [], r, pivoting=piv, accuracy=s["acc"], aux=s["aux"], nproc=groups, **kw)
    assert tt.fun_id == E.TTX_FUN_COSCOEFF
    return tt, s


@pytest.mark.parametrize("d", [2, 4, 6, 10])
def test_k_eval_bit_identical_to_restatement(d):
    _engine(d, 65, 4, 1)[0].close()
    s = D.coscoeff_setup(d, 65)
    rng = np.random.default_rng(100 + d)
    ind = np.concatenate([rng.integers(1, 66, size=(3072, d)), rng.integers(1, 4, size=(1024, d))]).astype(np.int32)
    dev = E.k_eval(E.TTX_FUN_COSCOEFF, s["n"], [], ind, aux=s["aux"])
    host, _ = CU.host_values(d, s["aux"], ind)
    assert np.array_equal(dev.view(np.int64), host.view(np.int64)), np.flatnonzero(dev != host)[:10]
    # and the genuine reference's elements, to rounding
    ref = CU.reference_values()[d]
    dv = E.k_eval(E.TTX_FUN_COSCOEFF, s["n"], [], ref[0], aux=s["aux"])
    hv, mag = CU.host_values(d, s["aux"], ref[0])
    assert np.array_equal(dv, hv) and (np.abs(dv - ref[1]) <= 1e-14 * mag).all()


def _same(tt, oo):
    d = tt.d
    assert np.array_equal(tt.tapes()[:, 1:d], oo["tapes"][:, 1:d])
    for f in ("it", "dir", "erank", "neval", "val", "amax", "pivotmax", "pivotmin"):
        assert [a[f] for a in tt.sweeps()] == [b[f] for b in oo["sweeps"]], f
    assert tt.neval == oo["neval"]
    assert np.array_equal(tt.ranks(), oo["r"])
    assert all(np.array_equal(tt.core(k), oo["cores"][k - 1]) for k in range(1, d + 1))


@pytest.mark.parametrize("d,n,r,piv,groups", [(6, 65, 20, 1, 1), (6, 33, 12, 2, 2), (8, 17, 10, 0, 1), (5, 17, 8, -1, 1), (6, 33, 12, 3, 3)])
def test_sweep_bit_exact_vs_oracle(d, n, r, piv, groups):
    tt, s = _engine(d, n, r, piv, groups)
    tt.run()
    oo = O.dmrgg(s["n"], E.TTX_FUN_HOST, s["aux"], r, piv=piv, accuracy=s["acc"], nproc=groups, user=CU.fun_addr(), accchk=700)
    _same(tt, oo)
    assert tt.host_calls == 0
    a = tt.accchk(700)
    assert all(a[k] == oo["accchk"][k] for k in ("einf", "efro", "ainf", "afro")) and np.array_equal(a["pivot"], oo["accchk"]["pivot"])
    tt.close()


def test_device_integrand_equals_host_callback_run():
    """the same problem through ttx_set_integrand_host (the C restatement on the host) and on the device: identical results, and
    the device run never calls the host; TTX_ARITH=fast leaves this integrand exact"""
    tt, s = _engine(6, 65, 20, 1, arith="fast")
    assert tt.arith == "exact"
    tt.run()
    hh = E.TTCross(s["n"], E.TTX_FUN_HOST, [], 20, pivoting=1, accuracy=s["acc"])
    hh.set_integrand_host(CU.fun_addr(), s["aux"]).run()
    assert tt.host_calls == 0 and hh.host_calls > 0
    oo = dict(tapes=hh.tapes(), sweeps=hh.sweeps(), neval=hh.neval, r=hh.ranks(), cores=[hh.core(k) for k in range(1, 7)])
    _same(tt, oo)
    assert [a["erank"] for a in tt.sweeps()][-1] == 20.0
    hh.close()
    tt.close()


def test_driver_runs_on_device():
    tt, val, s = D.run_driver(["coscoeff", "6", "65", "20", "1"], verbose=False)
    assert val is None and tt.fun_id == E.TTX_FUN_COSCOEFF and tt.host_calls == 0 and tt.neval == 121104   # the reference's count
    tt.close()


def test_two_processes_over_host_transport():
    _engine(6, 33, 12, 2, 2)[0].close()
    name = "ttx_cc_" + uuid.uuid4().hex[:12]
    procs = []
    for rk in range(2):
        env = dict(os.environ, RANK=str(rk), WORLD_SIZE="2", TTX_SHM_NAME=name)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "coscoeff_mp_worker.py"), "6", "33", "12", "2", "2"],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    for p in procs:
        o, e = p.communicate(timeout=300)
        assert p.returncode == 0 and " OK" in o, o[-1500:] + e[-1500:]


def test_fortran_driver_recognised_as_device_integrand():
    """ttcross_amd/fortran/test_crs_coscoeff.f90 (the fork's driver without its HDF5 output) hands calc_coefficient of the drop-in
    coefficients_mod to dtt_dmrgg without par: it must be recognised as TTX_FUN_COSCOEFF, and its sweep log must equal the
    TTX_INTEGRAND=host run, the Python driver's run and the genuine reference's log"""
    from conftest import fortran_exe
    from golden_util import GOLDEN, engine_env, parse_log
    _engine(6, 65, 20, 1)[0].close()
    exe = fortran_exe("test_crs_coscoeff")
    runs = {}
    for mode in ("auto", "host"):
        env = engine_env(dict(os.environ, TTX_INTEGRAND=mode))
        p = subprocess.run([exe, "6", "65", "20", "1"], capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        runs[mode] = p.stdout
    assert "integrand: fun_id 5" in runs["auto"] and "integrand: fun_id 4" in runs["host"]
    (ra, _, na), (rh, _, nh) = parse_log(runs["auto"]), parse_log(runs["host"])
    key = lambda rows: [(r["it"], r["dir"], r["erank"], r["neval"]) for r in rows]
    assert key(ra) == key(rh) and na == nh
    tt, _, _ = D.run_driver(["coscoeff", "6", "65", "20", "1"], verbose=False)
    assert [(a["erank"], a["neval"]) for a in tt.sweeps()] == [(r["erank"], r["neval"]) for r in ra] and tt.neval == na
    tt.close()
    rg, _, ng = parse_log(open(os.path.join(GOLDEN, "coscoeff_6_65_20_1.txt")).read())
    assert key(rg) == key(ra) and ng == na
