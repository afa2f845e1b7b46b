"""GPU tests of loadable device integrands (TTX_FUN_DEVICE, include/ttx_device_fun.h): a user's `fun` written as a HIP __device__
function, compiled to a code object and evaluated on the device between the two passes of every evaluating kernel.  The example
integrands use only + * /, so everything is compared BIT FOR BIT: single elements against the host C twins (tests/devfun_ref.c)
and the built-in Ising integrand, whole sweeps against the oracle and against the host-callback engine."""
import os
import subprocess
import sys
import threading
import uuid

import numpy as np
import pytest

import devfun_util as U
import oracle_lib as O
from conftest import ROOT, fortran_exe
from golden_util import engine_env
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

pytestmark = pytest.mark.gpu

CASES = [(5, 17, 10, 2, 1), (6, 13, 8, 1, 3), (4, 9, 6, 0, 1), (8, 11, 7, 3, 2), (4, 7, 5, -1, 1), (5, 5, 4, -1, 2)]


@pytest.fixture(scope="module")
def co():
    """code objects of the example integrands: {key: path}"""
    return {k: U.code_object(k) for k in U.SOURCES}


def _dev(s, r, piv, nproc, path, name, par=None):
    tt = E.TTCross(s["n"], E.TTX_FUN_DEVICE, [], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], nproc=nproc)
    return tt.set_integrand_device(path, name, s["par"] if par is None else par)


def _same_run(tt, oo, d, quad):
    """tapes, per-sweep records, ranks, cores and integral of an engine equal those of an oracle result (bit for bit)"""
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d])
    for f in ("neval", "val", "amax"):
        assert [a[f] for a in tt.sweeps()] == [b[f] for b in oo["sweeps"]], f
    assert tt.neval == oo["neval"]
    assert np.array_equal(tt.ranks(), oo["r"])
    assert all(np.array_equal(tt.core(k), oo["cores"][k - 1]) for k in range(1, d + 1))
    assert tt.quad(quad) == oo["value"]


def _as_result(tt, d, quad):
    return dict(tapes=tt.tapes(), sweeps=tt.sweeps(), neval=tt.neval, r=tt.ranks(), cores=[tt.core(k) for k in range(1, d + 1)], value=tt.quad(quad))


# ---- elements ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key,name", [("rational", "rational"), ("rational_wave", "rational_wave")])
@pytest.mark.parametrize("n", [[5, 4], [3, 9, 2], [17] * 5, [7, 11, 5, 13, 9, 3], [9] * 70, [5] * 300],
                         ids=["d2", "d3_unequal", "d5", "d6_unequal", "d70", "d300"])
def test_elements_of_rational_equal_the_c_twin(co, key, name, n):
    """eval_device (the code object's list kernel), lane and wave form, against the C twin: identical doubles.  d = 2 (the
    smallest train), unequal mode sizes, d = 70 (more than one chunk of the wave form), d = 300 (the largest d of the host tests)."""
    rng = np.random.default_rng(len(n))
    nmax = max(n)
    x = np.sort(rng.random(nmax))
    par = np.concatenate([x, rng.random(nmax)])
    npts = 3000 if len(n) <= 70 else 600
    ind = np.stack([rng.integers(1, nk + 1, size=npts) for nk in n], axis=1).astype(np.int32)
    tt = E.TTCross(n, E.TTX_FUN_DEVICE, [], 2, pivoting=1).set_integrand_device(co[key], name, par)
    got = tt.eval_device(ind)
    assert np.array_equal(got, U.twin_eval("ttx_devfun_rational", n, par, ind))
    tt.close()


@pytest.mark.parametrize("m,n", [(3, 9), (6, 33), (16, 51), (64, 17)])
def test_elements_of_ising_c_equal_the_builtin(co, m, n):
    s = D.ising_setup("c", m, n)
    d, nn = m - 1, s["n"][0]
    rng = np.random.default_rng(m)
    ind = rng.integers(1, nn + 1, size=(4000, d)).astype(np.int32)
    tt = E.TTCross(s["n"], E.TTX_FUN_DEVICE, [], 2, pivoting=1).set_integrand_device(co["ising_c"], "ising_c", s["par"])
    got = tt.eval_device(ind)
    L = E.load_library()
    ref = np.zeros(ind.shape[0])
    nv, pv = np.asarray(s["n"], dtype=np.int32), np.ascontiguousarray(s["par"])
    E._check(L.ttx_k_eval(0, E.TTX_FUN_ISING, d, E._ip(nv), E._dp(pv), pv.size, None, 0, ind.shape[0], E._ip(ind), E._dp(ref)))
    assert np.array_equal(got, ref)
    assert np.array_equal(got, O.fun(1, s["n"], s["par"], ind))
    tt.close()


def test_eval_device_refuses_an_index_outside_the_modes(co):
    s = U.user_setup(3, 5)
    tt = _dev(s, 2, 1, 1, co["rational"], "rational")
    with pytest.raises(E.TTXError, match="outside 1..5"):
        tt.eval_device([[1, 6, 1]])
    with pytest.raises(E.TTXError, match="outside 1..5"):
        tt.eval_device([[0, 1, 1]])
    tt.close()


# ---- sweeps ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,n,r,piv,nproc", CASES)
def test_device_integrand_bit_exact_vs_oracle_and_host_callback(co, d, n, r, piv, nproc):
    """The rational integrand loaded as a code object: initial cross, lottery, rook half-steps (piv >= 1), lottery only (piv = 0), full
    pivoting (piv = -1), one to three bond groups -- identical to the oracle calling the C twin AND to the engine's host-callback
    path with the C twin; not one value goes through the host."""
    s = U.user_setup(d, n)
    addr = U.twin_addr("ttx_devfun_rational")
    tt = _dev(s, r, piv, nproc, co["rational"], "rational").run()
    oo = O.dmrgg(s["n"], 4, s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], nproc=nproc, user=addr)
    _same_run(tt, oo, d, s["quad"])
    hh = E.TTCross(s["n"], E.TTX_FUN_HOST, [], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], nproc=nproc)
    hh.set_integrand_host(addr, s["par"]).run()
    _same_run(tt, _as_result(hh, d, s["quad"]), d, s["quad"])
    assert tt.host_calls == 0 and hh.host_calls >= hh.neval
    assert tt.fun_id == E.TTX_FUN_DEVICE
    tt.close()
    hh.close()


@pytest.mark.parametrize("d,n,r,piv,nproc", [CASES[0], CASES[5]])
def test_wave_form_bit_exact_vs_oracle(co, d, n, r, piv, nproc):
    s = U.user_setup(d, n)
    tt = _dev(s, r, piv, nproc, co["rational_wave"], "rational_wave").run()
    oo = O.dmrgg(s["n"], 4, s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], nproc=nproc, user=U.twin_addr("ttx_devfun_rational"))
    _same_run(tt, oo, d, s["quad"])
    assert tt.host_calls == 0
    tt.close()


def test_unequal_mode_sizes(co):
    """mode sizes differ: the slots of a fiber batch have holes (rows of NM slots, n(k) of them raised)"""
    n = [9, 5, 11, 7, 6]
    x, _ = D.lgwt(11)
    par = np.concatenate([0.5 * (x + 1.0), np.zeros(11)])
    quad = [np.full(nk, 1.0 / nk) for nk in n]
    tt = E.TTCross(n, E.TTX_FUN_DEVICE, [], 6, pivoting=2, accuracy=500 * D.EPS, quad=quad, nproc=2).set_integrand_device(co["rational"], "rational", par).run()
    oo = O.dmrgg(n, 4, par, 6, piv=2, accuracy=500 * D.EPS, quad=quad, nproc=2, user=U.twin_addr("ttx_devfun_rational"))
    _same_run(tt, oo, len(n), quad)
    tt.close()


def test_fast_arithmetic_leaves_a_device_integrand_exact(co):
    s = U.user_setup(5, 17)
    tt = E.TTCross(s["n"], E.TTX_FUN_DEVICE, [], 10, pivoting=2, accuracy=s["acc"], quad=s["quad"], arith="fast")
    tt.set_integrand_device(co["rational"], "rational", s["par"]).run()
    assert tt.arith == "exact"
    oo = O.dmrgg(s["n"], 4, s["par"], 10, piv=2, accuracy=s["acc"], quad=s["quad"], user=U.twin_addr("ttx_devfun_rational"))
    _same_run(tt, oo, 5, s["quad"])
    tt.close()


@pytest.mark.parametrize("m,n,r,piv,nproc", [(6, 33, 12, 2, 1), (10, 17, 8, 2, 4)], ids=["c6_smoke_case", "c10_g4"])
def test_ising_c_three_ways(co, m, n, r, piv, nproc):
    """ising_c.hip through the loader, the built-in TTX_FUN_ISING and the oracle: identical tapes, cores, integral."""
    s = D.ising_setup("c", m, n)
    d = m - 1
    dev = E.TTCross(s["n"], E.TTX_FUN_DEVICE, [], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=nproc)
    dev.set_integrand_device(co["ising_c"], "ising_c", s["par"]).run()
    blt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=nproc).run()
    oo = O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=nproc)
    _same_run(dev, oo, d, s["quad"])
    _same_run(blt, oo, d, s["quad"])
    dev.close()
    blt.close()


def test_accchk_equals_the_host_callback_engine(co):
    s = U.user_setup(5, 17)
    tt = _dev(s, 10, 2, 1, co["rational"], "rational").run()
    hh = E.TTCross(s["n"], E.TTX_FUN_HOST, [], 10, pivoting=2, accuracy=s["acc"], quad=s["quad"])
    hh.set_integrand_host(U.twin_addr("ttx_devfun_rational"), s["par"]).run()
    a, b = tt.accchk(3000), hh.accchk(3000)
    for k in ("einf", "efro", "ainf", "afro"):
        assert a[k] == b[k], k
    assert np.array_equal(a["pivot"], b["pivot"])
    assert tt.host_calls == 0
    tt.close()
    hh.close()


def test_two_engines_with_two_integrands_in_two_threads(co):
    """Two engines, two code objects, two host threads (ctypes releases the GIL inside ttx_run): each equals its oracle run."""
    cases = [(5, 17, 10, 2, "rational", "rational", "ttx_devfun_rational"), (6, 13, 8, 1, "second", "second", "ttx_devfun_second")]
    out = [None, None]

    def job(i):
        d, n, r, piv, key, name, _ = cases[i]
        s = U.user_setup(d, n)
        tt = _dev(s, r, piv, 1, co[key], name).run()
        out[i] = _as_result(tt, d, s["quad"])
        tt.close()

    th = [threading.Thread(target=job, args=(i,)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    for i, (d, n, r, piv, _, _, twin) in enumerate(cases):
        s = U.user_setup(d, n)
        oo = O.dmrgg(s["n"], 4, s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], user=U.twin_addr(twin))
        assert out[i] is not None and out[i]["neval"] == oo["neval"] and out[i]["value"] == oo["value"]
        assert np.array_equal(out[i]["tapes"][:, 1:d], oo["tapes"][:, 1:d])
        assert all(np.array_equal(a, b) for a, b in zip(out[i]["cores"], oo["cores"]))


def test_replacing_the_integrand_between_two_runs(co):
    """Setting an integrand again replaces the first (and unloads its module); par is COPIED: changing the caller's array after
    the call changes nothing."""
    d, n, r, piv = 5, 17, 10, 2
    s = U.user_setup(d, n)
    par = s["par"].copy()
    tt = _dev(s, r, piv, 1, co["rational"], "rational", par=par)
    par[:] = 0.0                                     # the engine has its own copy
    tt.run()
    _same_run(tt, O.dmrgg(s["n"], 4, s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], user=U.twin_addr("ttx_devfun_rational")), d, s["quad"])
    tt.set_integrand_device(open(co["second"], "rb").read(), "second", s["par"]).run()      # from memory this time
    _same_run(tt, O.dmrgg(s["n"], 4, s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], user=U.twin_addr("ttx_devfun_second")), d, s["quad"])
    tt.set_integrand_device(co["rational"], "rational", s["par"]).run()
    _same_run(tt, O.dmrgg(s["n"], 4, s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], user=U.twin_addr("ttx_devfun_rational")), d, s["quad"])
    tt.close()


# ---- several processes ----------------------------------------------------------------------------------------------------------

def test_two_processes_over_shm(co):
    """Two engine processes on one GPU over the shared-memory transport, each loading the code object; the worker compares the job
    with the one-process run and checks dtt_accchk on the job (which works on a replica that shares the module)."""
    name = "ttx_" + uuid.uuid4().hex[:12]
    procs = []
    for rk in range(2):
        env = dict(os.environ, RANK=str(rk), WORLD_SIZE="2", TTX_SHM_NAME=name, HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "devfun_mp_worker.py"), "6", "13", "8", "2", "4"],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((p.returncode, o, e))
    for rc, o, e in outs:
        assert rc == 0 and " OK" in o, o[-2000:] + e[-2000:]


def test_replica_shares_the_integrand(co):
    """ttx_replicate of an engine with a device integrand: the replica evaluates (accchk) after the original is gone."""
    s = U.user_setup(5, 17)
    tt = _dev(s, 10, 2, 1, co["rational"], "rational").run()
    want = tt.accchk(1000)
    tt2 = _dev(s, 10, 2, 1, co["rational"], "rational").run()
    rep = tt2.replicate()
    tt2.close()
    got = rep.accchk(1000)
    assert all(got[k] == want[k] for k in ("einf", "efro", "ainf", "afro"))
    rep.close()
    tt.close()


# ---- NaN ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["rational_nan", "rational_partnan"])
@pytest.mark.parametrize("piv,nproc", [(2, 1), (1, 3), (-1, 1), (0, 2)])
def test_nan_device_integrand_ends_like_the_host_callback(co, name, piv, nproc):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "devfun_nan_worker.py"), name, str(piv), str(nproc)],
                       capture_output=True, text=True, timeout=300)
    blob = p.stdout + p.stderr
    assert "Memory access fault" not in blob and "core dump" not in blob.lower(), blob[-3000:]
    assert p.returncode == 0 and " OK" in p.stdout, blob[-3000:]


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_engine_usable(co, tmp_path):
    s = U.user_setup(4, 9)
    L = E.load_library()
    good = open(co["rational"], "rb").read()
    p = np.ascontiguousarray(s["par"])

    def rc_msg(rc):
        return rc, L.ttx_last_error().decode()

    # an engine of another kind
    hh = E.TTCross(s["n"], E.TTX_FUN_HOST, [], 6, pivoting=1, accuracy=s["acc"])
    rc, msg = rc_msg(L.ttx_set_integrand_device(hh._h, good, len(good), b"rational", E._dp(p), p.size))
    assert rc == 4 and "TTX_FUN_DEVICE" in msg
    rc, msg = rc_msg(L.ttx_set_integrand_device_file(hh._h, co["rational"].encode(), b"rational", E._dp(p), p.size))
    assert rc == 4 and "TTX_FUN_DEVICE" in msg
    out = np.zeros(1)
    one = np.ones(4, dtype=np.int32)
    rc, msg = rc_msg(L.ttx_eval_device(hh._h, 1, E._ip(one), E._dp(out)))
    assert rc == 4 and "TTX_FUN_DEVICE" in msg
    hh.close()

    tt = E.TTCross(s["n"], E.TTX_FUN_DEVICE, [], 6, pivoting=1, accuracy=s["acc"], quad=s["quad"])
    # nothing set yet
    with pytest.raises(E.TTXError, match="ttx_set_integrand_device first"):
        tt.run()
    rc, msg = rc_msg(L.ttx_eval_device(tt._h, 1, E._ip(one), E._dp(out)))
    assert rc == 4 and "ttx_set_integrand_device first" in msg
    # null / empty image
    rc, msg = rc_msg(L.ttx_set_integrand_device(tt._h, None, 100, b"rational", E._dp(p), p.size))
    assert rc == 1 and "empty code object" in msg
    rc, msg = rc_msg(L.ttx_set_integrand_device(tt._h, good, 0, b"rational", E._dp(p), p.size))
    assert rc == 1 and "empty code object" in msg
    # name missing
    rc, msg = rc_msg(L.ttx_set_integrand_device(tt._h, good, len(good), None, E._dp(p), p.size))
    assert rc == 1 and "name missing" in msg
    # unreadable / empty file
    rc, msg = rc_msg(L.ttx_set_integrand_device_file(tt._h, str(tmp_path / "nothing.hsaco").encode(), b"rational", E._dp(p), p.size))
    assert rc == 1 and "cannot read" in msg
    (tmp_path / "empty.hsaco").write_bytes(b"")
    rc, msg = rc_msg(L.ttx_set_integrand_device_file(tt._h, str(tmp_path / "empty.hsaco").encode(), b"rational", E._dp(p), p.size))
    assert rc == 1 and "is empty" in msg
    # garbage bytes
    (tmp_path / "garbage.hsaco").write_bytes(np.random.default_rng(1).integers(0, 256, size=5000, dtype=np.uint8).tobytes())
    rc, msg = rc_msg(L.ttx_set_integrand_device_file(tt._h, str(tmp_path / "garbage.hsaco").encode(), b"rational", E._dp(p), p.size))
    assert rc == 1 and "neither a complete code object" in msg
    # a truncated bundle never reaches the runtime; a complete one built for another GPU does, and the runtime's refusal comes back
    cut = good[:len(good) // 2]
    rc, msg = rc_msg(L.ttx_set_integrand_device(tt._h, cut, len(cut), b"rational", E._dp(p), p.size))
    assert rc == 1 and "neither a complete code object" in msg
    other = open(U.other_arch_object(), "rb").read()
    rc, msg = rc_msg(L.ttx_set_integrand_device(tt._h, other, len(other), b"rational", E._dp(p), p.size))
    assert rc == 1 and "refused the code object" in msg
    # a valid code object without the symbol
    rc, msg = rc_msg(L.ttx_set_integrand_device(tt._h, good, len(good), b"nosuch", E._dp(p), p.size))
    assert rc == 1 and "no integrand 'nosuch'" in msg
    # ABI mismatch, too much LDS
    with pytest.raises(E.TTXError, match="slot ABI version 99"):
        tt.set_integrand_device(co["second"], "future", s["par"])
    with pytest.raises(E.TTXError, match="more than 64 KB"):
        tt.set_integrand_device(co["second"], "greedy", s["par"])
    # par
    rc, msg = rc_msg(L.ttx_set_integrand_device(tt._h, good, len(good), b"rational", E._dp(p), -1))
    assert rc == 1 and "par missing" in msg
    rc, msg = rc_msg(L.ttx_set_integrand_device(tt._h, good, len(good), b"rational", None, 3))
    assert rc == 1 and "par missing" in msg
    # still nothing set, and still usable
    with pytest.raises(E.TTXError, match="ttx_set_integrand_device first"):
        tt.run()
    tt.set_integrand_device(co["rational"], "rational", s["par"]).run()
    oo = O.dmrgg(s["n"], 4, s["par"], 6, piv=1, accuracy=s["acc"], quad=s["quad"], user=U.twin_addr("ttx_devfun_rational"))
    _same_run(tt, oo, 4, s["quad"])
    # a refusal after a good integrand keeps the good one
    with pytest.raises(E.TTXError, match="no integrand"):
        tt.set_integrand_device(co["rational"], "nosuch", s["par"])
    tt.run()
    _same_run(tt, oo, 4, s["quad"])
    tt.close()


def test_accchk_before_a_run_is_a_state_error():
    s = U.user_setup(4, 9)
    tt = E.TTCross(s["n"], E.TTX_FUN_DEVICE, [], 6, pivoting=1)
    with pytest.raises(E.TTXError, match="run first"):
        tt.accchk(10)
    tt.close()


# ---- Fortran -------------------------------------------------------------------------------------------------------------------

def _lines(txt):
    """sweep lines without the timing column, and the result lines"""
    keep = []
    for ln in txt.splitlines():
        if "n_evals" in ln:
            t = ln.split()
            keep.append(" ".join(x for i, x in enumerate(t) if not (i > 0 and t[i - 1] == "time:")))
        elif ln.startswith("computed value"):
            keep.append(ln)
        elif ln.startswith("...with"):
            keep.append(" ".join(ln.split()[:3]))
    return keep


def test_fortran_driver_moves_to_the_device_without_a_source_change(co):
    """test_crs_devfun.f90 passes an ordinary Fortran `fun` to dtt_dmrgg.  Without TTX_DEVICE_FUN it runs as a host callback; with
    TTX_DEVICE_FUN=<code object>:<name> the same binary evaluates on the device: identical sweep lines and integral."""
    exe = fortran_exe("test_crs_devfun")
    base = engine_env()
    base.pop("TTX_DEVICE_FUN", None)
    base.pop("TTX_INTEGRAND", None)
    a = subprocess.run([exe, "5", "17", "10", "2"], capture_output=True, text=True, timeout=300, env=base)
    b = subprocess.run([exe, "5", "17", "10", "2"], capture_output=True, text=True, timeout=300, env=dict(base, TTX_DEVICE_FUN=co["rational"] + ":rational"))
    assert a.returncode == 0 and b.returncode == 0, a.stdout + a.stderr + b.stdout + b.stderr
    assert "integrand on the host" in a.stdout and "integrand on the device" in b.stdout, a.stdout + b.stdout
    la, lb = _lines(a.stdout), _lines(b.stdout)
    assert len(la) >= 4 and la == lb, "\n".join(la + ["----"] + lb)
    # TTX_INTEGRAND=host keeps its meaning: it forces the host callback
    c = subprocess.run([exe, "5", "17", "10", "2"], capture_output=True, text=True, timeout=300,
                       env=dict(base, TTX_DEVICE_FUN=co["rational"] + ":rational", TTX_INTEGRAND="host"))
    assert c.returncode == 0 and "integrand on the host" in c.stdout and _lines(c.stdout) == la
