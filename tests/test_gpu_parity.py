"""GPU parity tests: the HIP engine (through the C-ABI of libttx.so) against the CPU oracle on the same
inputs.  Integer/index work (pivot tapes, ranks, evaluation counts) must be IDENTICAL; floating point must
be bit-identical for ALL integrands (same operation order, no FMA contraction, IEEE division; the exp of the
stdnorm / mvn integrands restates the run-time library's algorithm operation for operation, ttx_exp.h)."""
import numpy as np
import pytest

import oracle_lib as O
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

pytestmark = pytest.mark.gpu


def _run_both(s, r, piv, nproc=1, path=None):
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"],
                   aux=s["aux"], nproc=nproc)
    if path is not None:
        assert tt.sweep_path() == path
    tt.run()
    oo = O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], aux=s["aux"],
                 nproc=nproc)
    return tt, oo


ISING_CASES = [("c", 6, 33, 20, 2), ("c", 6, 33, 10, 1), ("c", 5, 17, 8, 0), ("c", 8, 25, 12, 3), ("d", 6, 33, 12, 2),
               ("e", 5, 33, 12, 2), ("d", 12, 33, 10, 2), ("c", 16, 51, 32, 2), ("c", 64, 51, 32, 2),
               ("c", 5, 9, 6, -1), ("d", 4, 11, 5, -1), ("d", 32, 33, 12, 2),
               # long chains: several 16-column chunks per row of the pair triangle in the row-wise lottery kernel, 8-wide division batches
               ("d", 50, 9, 6, 2), ("e", 70, 5, 4, 1), ("d", 100, 17, 10, 3),
               # maxrank above 97: the chain matrices of the per-sweep quadrature no longer fit the LDS (global scratch); ranks saturate below
               ("c", 7, 9, 120, 2)]


@pytest.mark.parametrize("kind,m,n,r,piv", ISING_CASES, ids=[f"{c[0]}{c[1]}_n{c[2]}_r{c[3]}_p{c[4]}" for c in ISING_CASES])
def test_ising_sweep_bit_exact(kind, m, n, r, piv):
    s = D.ising_setup(kind, m, n)
    tt, oo = _run_both(s, r, piv)
    gs, os_ = tt.sweeps(), oo["sweeps"]
    assert len(gs) == len(os_)
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d]), "pivot tapes differ"
    for a, b in zip(gs, os_):
        assert a["neval"] == b["neval"] and a["erank"] == b["erank"]
        assert a["val"] == b["val"], f"sweep {a['it']}: val {a['val']!r} vs {b['val']!r}"
        assert a["amax"] == b["amax"] and a["pivotmax"] == b["pivotmax"]
    assert tt.neval == oo["neval"]
    assert np.array_equal(tt.ranks(), oo["r"])
    for k in range(1, tt.d + 1):
        assert np.array_equal(tt.core(k), oo["cores"][k - 1]), f"core {k} differs"
    assert tt.quad(s["quad"]) == oo["value"]
    if s["tru"]:      # known-answer check (the driver's `correct digits`); low-rank cases stop at ~1e-7
        assert abs(1 - tt.quad(s["quad"]) / s["tru"]) < (1e-12 if r >= 32 else 1e-6 if n >= 17 else 1e-3)


GROUP_CASES = [("c", 6, 33, 20, 2, 2), ("c", 6, 33, 20, 2, 4), ("d", 8, 33, 10, 2, 3), ("c", 16, 51, 32, 2, 8), ("c", 64, 51, 32, 2, 8),
               ("c", 64, 51, 32, 2, 5), ("e", 9, 33, 12, 3, 7), ("c", 7, 9, 5, -1, 2), ("c", 12, 17, 6, 0, 3), ("d", 60, 9, 6, 2, 4)]


@pytest.mark.parametrize("kind,m,n,r,piv,nproc", GROUP_CASES, ids=[f"{c[0]}{c[1]}_r{c[3]}_p{c[4]}_np{c[5]}" for c in GROUP_CASES])
def test_bond_groups_bit_exact(kind, m, n, r, piv, nproc):
    """nproc bond groups on one GPU == the reference's nproc MPI ranks (oracle virtual ranks): tape, boundary
    exchange both ways, corner evaluations, lagged erank, inv shift and the quadrature tree."""
    s = D.ising_setup(kind, m, n)
    tt, oo = _run_both(s, r, piv, nproc=nproc)
    gs, os_ = tt.sweeps(), oo["sweeps"]
    assert len(gs) == len(os_)
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d]), "pivot tapes differ"
    for a, b in zip(gs, os_):
        assert a["neval"] == b["neval"], f"sweep {a['it']}: neval {a['neval']} vs {b['neval']}"
        assert a["erank"] == b["erank"]
        assert a["val"] == b["val"], f"sweep {a['it']}: val {a['val']!r} vs {b['val']!r}"
        assert a["amax"] == b["amax"] and a["pivotmax"] == b["pivotmax"]
    assert np.array_equal(tt.ranks(), oo["r"])
    for k in range(1, tt.d + 1):
        assert np.array_equal(tt.core(k), oo["cores"][k - 1]), f"core {k} differs"
    assert tt.quad(s["quad"]) == oo["value"]


def _assert_identical(tt, oo, cores=True):
    """tapes, per-sweep records, ranks, evaluation count (and finalised cores) of the engine == the oracle's, bit for bit"""
    gs, os_ = tt.sweeps(), oo["sweeps"]
    assert len(gs) == len(os_)
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d]), "pivot tapes differ"
    for a, b in zip(gs, os_):
        assert a["neval"] == b["neval"] and a["erank"] == b["erank"], f"sweep {a['it']}"
        assert a["val"] == b["val"], f"sweep {a['it']}: val {a['val']!r} vs {b['val']!r}"
        assert a["amax"] == b["amax"] and a["pivotmax"] == b["pivotmax"], f"sweep {a['it']}"
    assert tt.neval == oo["neval"] and np.array_equal(tt.ranks(), oo["r"])
    if cores:
        for k in range(1, tt.d + 1):
            assert np.array_equal(tt.core(k), oo["cores"][k - 1]), f"core {k} differs"


def test_exp_device_is_the_runtime_libm():
    """The integrands' exp on the device (ttx_exp.h) against the host's libm, bit for bit -- the arguments the
    stdnorm / mvn integrands produce (0 down to the subnormal tail), plus the special values."""
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.exp.restype = ctypes.c_double
    libm.exp.argtypes = [ctypes.c_double]
    rng = np.random.default_rng(11)
    x = np.concatenate([-rng.random(200000) * 800.0, -745.2 + rng.random(50000) * 40.0, (rng.random(50000) - 0.5) * 1400.0,
                        (rng.random(20000) - 0.5) * 1e-9, [0.0, -0.0, 709.78, 710.0, -745.13, -745.14, -746.0, float("inf"), -float("inf")]])
    got = E.k_exp(x)
    want = np.array([libm.exp(v) for v in x])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


EXP_CASES = [("stdnorm", 4, 33, 10, 2, 1), ("mvn", 6, 33, 12, 2, 1), ("stdnorm", 7, 17, 8, 1, 3), ("mvn", 9, 17, 10, 3, 2),
             ("mvn", 5, 9, 6, 0, 1), ("stdnorm", 5, 9, 5, -1, 1), ("mvn", 24, 17, 12, 2, 4), ("mvn-np", 20, 17, 12, 2, 2),
             ("mvn-np", 40, 17, 16, 2, 1),
             # d a multiple of 64: the quadratic form with register-resident terms (one, two and three registers of a row per lane)
             ("mvn", 64, 5, 4, 2, 2), ("mvn", 128, 5, 5, 3, 3), ("mvn", 192, 3, 3, 1, 2), ("mvn", 256, 3, 2, 1, 1),
             ("mvn", 288, 2, 2, 1, 2)]       # not a multiple of 64: the LDS-broadcast sums with five registers of a row per lane


@pytest.mark.parametrize("kind,d,n,r,piv,nproc", EXP_CASES, ids=[f"{c[0]}{c[1]}_n{c[2]}_r{c[3]}_p{c[4]}_np{c[5]}" for c in EXP_CASES])
def test_exp_integrands_bit_exact(kind, d, n, r, piv, nproc):
    """stdnorm / mvn: with the run-time library's exp restated on the device (ttx_exp.h) these runs are bit-identical to
    the oracle like the Ising ones -- tapes, every per-sweep record, cores, integral (round 1 could only assert 1e-9 on
    the integral: one last-ulp difference in exp re-routes the pivots of these symmetric integrands)."""
    s = D.box_setup(kind.split("-")[0], d, n)
    if kind == "mvn":
        s["aux"] = O.mvn_init(d)            # "mvn-np" keeps numpy's inverse covariance / determinant (other last bits)
    tt, oo = _run_both(s, r, piv, nproc=nproc)
    _assert_identical(tt, oo)
    assert tt.quad(s["quad"]) == oo["value"]


@pytest.mark.parametrize("name,need", [("stdnorm_4_33_10_2", 2), ("mvn_6_33_12_2", 8)])
def test_exp_integrands_leading_sweeps_vs_reference_log(name, need):
    """The GPU path against the golden logs of the GENUINE reference, as tests/test_oracle_golden.py asserts for the oracle:
    `need` leading sweeps identical in (erank, n_evals) and to 2e-13 in val; then the noise floor decides near-ties
    (the reference inverts the covariance with LAPACK and sums with MKL)."""
    import os
    from golden_util import GOLDEN, parse_log
    kind, d, n, r, piv = name.split("_")[0], *[int(v) for v in name.split("_")[1:]]
    s = D.box_setup(kind, d, n)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], aux=s["aux"]).run()
    g_rows, g_val, _ = parse_log(open(os.path.join(GOLDEN, name + ".txt")).read())
    rows = tt.sweeps()
    assert len(rows) == len(g_rows)
    k = 0
    for a, b in zip(g_rows, rows):
        if a["erank"] == round(b["erank"], 1) and a["neval"] == b["neval"] and abs(a["val"] - b["val"]) <= 2e-13 * abs(a["val"]):
            k += 1
        else:
            break
    assert k >= need, f"only {k} leading sweeps match the reference (need {need})"
    assert abs(tt.quad(s["quad"]) - g_val) <= (1e-13 if kind == "stdnorm" else 1e-3) * abs(g_val)


@pytest.mark.parametrize("nproc", [1, 4])
def test_config4_mvn_128_full_size_vs_oracle_fixture(nproc):
    """BASELINE config 4 at FULL size (test_crs_mvn 128 33 50 2; d = 128, n = 33, r = 50) through the C-ABI, against the
    per-sweep fixture of the oracle made in the build container (tests/golden/make_oracle_fixture.py; the oracle needs
    minutes, so it does not run here): nproc = 1, the reference's own decomposition, and nproc = 4, the configuration's
    four bond groups.  Everything the fixture holds must be IDENTICAL: 49 sweeps of tapes, erank, n_evals, val, amax,
    pivotmax, the final ranks and the integral."""
    import os
    from golden_util import GOLDEN
    f = np.load(os.path.join(GOLDEN, f"oracle_mvn_128_33_50_2_np{nproc}.npz"))
    s = D.box_setup("mvn", 128, 33)
    s["aux"] = O.mvn_init(128)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], 50, pivoting=2, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], aux=s["aux"], nproc=nproc).run()
    rows = tt.sweeps()
    assert len(rows) == len(f["it"]) == 50
    assert np.array_equal(tt.tapes()[:, 1:tt.d].astype(np.int16), f["tapes"][:, 1:tt.d]), "pivot tapes differ"
    assert [a["neval"] for a in rows] == f["neval"].tolist()
    assert [a["erank"] for a in rows] == f["erank"].tolist()
    assert [a["val"] for a in rows] == f["val"].tolist()
    assert [a["amax"] for a in rows] == f["amax"].tolist() and [a["pivotmax"] for a in rows] == f["pivotmax"].tolist()
    assert np.array_equal(tt.ranks(), f["r"]) and tt.neval == int(f["total_neval"])
    assert tt.quad(s["quad"]) == float(f["value"])


def test_config4_mvn_128_full_size_vs_reference_log():
    """The same run (nproc = 1) against the golden log of the GENUINE reference (oracle/_ref/test_crs_mvn 128 33 50 2).
    The integrand is symmetric under permutations of the dimensions, so exact ties between symmetric pivot candidates are
    broken by rounding alone: the reference (LAPACK inverse, MKL sums) and this engine part ways in n_evals at sweep 1 and
    the run is far from converged at r = 50 (1.2 correct digits).  What must agree: the number of sweeps, erank over the
    first 10 sweeps, val to 1e-9 over the first 6, n_evals to 3 % in every sweep, the final value to 5 %.
    (mu, inverse covariance, determinant as the reference computes them: LU inverse, oracle_lib.mvn_init.)"""
    import os
    from golden_util import GOLDEN, parse_log
    g_rows, g_val, g_nev = parse_log(open(os.path.join(GOLDEN, "mvn_128_33_50_2.txt")).read())
    s = D.box_setup("mvn", 128, 33)
    s["aux"] = O.mvn_init(128)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], 50, pivoting=2, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], aux=s["aux"]).run()
    rows = tt.sweeps()
    assert len(rows) == len(g_rows) == 50
    for k, (a, b) in enumerate(zip(g_rows, rows)):
        if k < 10:
            assert a["erank"] == round(b["erank"], 1), f"sweep {k}"
        if k < 6:
            assert abs(a["val"] - b["val"]) <= 1e-9 * abs(a["val"]), f"sweep {k}"
        assert abs(a["neval"] - b["neval"]) <= 0.03 * a["neval"], f"sweep {k}"
    assert abs(tt.quad(s["quad"]) - g_val) <= 0.05 * abs(g_val)


FULLPIV = [("c", 5, 9, 6), ("d", 4, 11, 5), ("c", 8, 17, 10), ("e", 6, 9, 8)]


@pytest.mark.parametrize("kind,m,n,r", FULLPIV, ids=[f"{c[0]}{c[1]}_n{c[2]}_r{c[3]}" for c in FULLPIV])
def test_full_pivoting_dense_mfma_by_tolerance(monkeypatch, kind, m, n, r):
    """pivoting = -1 as one dense step (TTX_FULLPIV=mfma, lib/dmrgg.f90:341-408): the superblock evaluated once, the
    residual A - col x row by an fp64 MFMA GEMM fused with the arg-max.  The matrix cores accumulate in their own order, so
    the residuals differ from the reference's dgemm in the last bits: parity BY TOLERANCE against the oracle -- the same
    number of sweeps, ranks and evaluations, every per-sweep value to 1e-9 relative, the integral to 1e-11 -- and against
    the engine's own column-by-column path, which stays bit-identical to the oracle (test_ising_sweep_bit_exact)."""
    s = D.ising_setup(kind, m, n)
    oo = O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=-1, accuracy=s["acc"], quad=s["quad"], tru=s["tru"])
    monkeypatch.setenv("TTX_FULLPIV", "mfma")
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=-1, accuracy=s["acc"], quad=s["quad"], tru=s["tru"]).run()
    gs, os_ = tt.sweeps(), oo["sweeps"]
    assert len(gs) == len(os_)
    for a, b in zip(gs, os_):
        assert a["neval"] == b["neval"] and a["erank"] == b["erank"]
        assert abs(a["val"] - b["val"]) <= 1e-9 * abs(b["val"]), f"sweep {a['it']}"
        assert a["amax"] == b["amax"]
    assert np.array_equal(tt.ranks(), oo["r"])
    assert abs(tt.quad(s["quad"]) - oo["value"]) <= 1e-11 * abs(oo["value"])


def test_k2_residual_argmax_bit_exact():
    rng = np.random.default_rng(1)
    for m, r in [(1632, 32), (6464, 64), (33, 1), (700, 17), (51, 0)]:
        a = rng.standard_normal(m)
        F = rng.standard_normal((m, max(r, 1)))[:, :r]
        x = rng.standard_normal(r)
        b, im, bm = E.k_residual_argmax(a, F, x)
        want = a.copy()
        for s in range(r):                      # netlib dgemv 'n', alpha=-1
            want = want + (-x[s]) * F[:, s]
        assert np.array_equal(b, want)
        assert im == int(np.argmax(np.abs(want))) and bm == want[im]
    # tie rule: lowest index wins
    a = np.zeros(600)
    a[[5, 300, 599]] = [-2.0, 2.0, 2.0]
    b, im, bm = E.k_residual_argmax(a, np.zeros((600, 1)), np.zeros(1))
    assert im == 5 and bm == -2.0


def test_k1_integrands_vs_oracle():
    rng = np.random.default_rng(2)
    for kind, m in [("c", 16), ("d", 9), ("e", 7)]:
        s = D.ising_setup(kind, m, 33)
        d = m - 1
        ind = rng.integers(1, 34, size=(500, d)).astype(np.int32)
        g = E.k_eval(E.TTX_FUN_ISING, s["n"], s["par"], ind)
        o = O.fun(1, s["n"], s["par"], ind)
        assert np.array_equal(g, o)
    s = D.box_setup("stdnorm", 5, 33)
    ind = rng.integers(1, 34, size=(300, 5)).astype(np.int32)
    assert np.array_equal(E.k_eval(E.TTX_FUN_STDNORM, s["n"], s["par"], ind), O.fun(2, s["n"], s["par"], ind))
    s = D.box_setup("mvn", 6, 33)
    aux = O.mvn_init(6)
    ind = rng.integers(1, 34, size=(300, 6)).astype(np.int32)
    assert np.array_equal(E.k_eval(E.TTX_FUN_MVN, s["n"], s["par"], ind, aux=aux), O.fun(3, s["n"], s["par"], ind, aux=aux))


def test_lottery_bit_exact():
    rng = np.random.default_rng(3)
    for (m, n, nz, npnt, pos) in [(1632, 1632, 31, 166, 0), (6464, 6464, 63, 330, 12345), (33, 33, 1, 68, 7), (640, 1020, 20, 120, 999)]:
        zc = np.sort(rng.choice(np.arange(1, m + 1), nz, replace=False)).astype(np.int32)
        zr = np.sort(rng.choice(np.arange(1, n + 1), nz, replace=False)).astype(np.int32)
        wc = np.ones(m)
        wc[zc - 1] = 0
        wr = np.ones(n)
        wr[zr - 1] = 0
        draws = O.flang_draws(pos, 2 * npnt)
        want = O.lottery2(npnt, wc, wr, draws)
        got = E.k_lottery(npnt, m, n, zc, zr, rngpos=pos)
        assert np.array_equal(got, want)


@pytest.mark.parametrize("world,args", [(2, "c 6 33 20 2 4"), (2, "c 64 51 32 2 8"), (3, "d 8 33 10 2 3"), (4, "c 16 51 32 2 8")],
                         ids=["w2_c6_g4", "w2_c64_g8", "w3_d8_g3", "w4_c16_g8"])
def test_multi_process_bond_split(world, args):
    """The N>1 path: `world` engine processes (one per GPU in production; here they share the card, <= 4 ranks)
    split the bond groups and exchange through the transport layer; bit-identical to the oracle."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(29500 + world), os.path.join(root, "tests", "mp_worker.py")] + args.split() + ["gloo"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count(" OK") == world


def test_rccl_transport_on_real_gpus():
    """The in-library RCCL transport (ncclSend/ncclRecv + ncclAllReduce on the engine's stream) needs one GPU per rank:
    skipped on a one-GPU box.  Until this has passed somewhere the RCCL path is EXPERIMENTAL."""
    import os
    import subprocess
    import sys
    import torch
    world = 2
    if torch.cuda.device_count() < world:
        pytest.skip(f"needs {world} GPUs (have {torch.cuda.device_count()}): the RCCL transport has never moved data yet")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", "29533", os.path.join(root, "tests", "mp_worker.py")] + "c 64 51 32 2 8".split() + ["rccl"]
    out = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count(" OK") == world


def test_rccl_loopback_selftest():
    """The RCCL transport's primitives on the one GPU of this pool: a one-rank communicator, a grouped ncclSend / ncclRecv of a
    neighbour-sized message to itself, the MAX and SUM all-reduces of the sweep, on a non-blocking stream (include/ttx.h:
    ttx_k_rccl_selftest).  The 2-GPU test above cannot run here; this one at least moves bytes through librccl."""
    import os
    import subprocess
    import sys
    # a process of its own: RCCL's communicator set-up wants a process that has not already opened dozens of engines and streams
    # (inside the full suite ncclCommInitRank failed with "unhandled cuda error"; alone it passes)
    code = ("import ctypes, sys; sys.path.insert(0, %r); from ttcross_amd import engine as E; L = E.load_library(); "
            "L.ttx_k_rccl_selftest.argtypes = [ctypes.c_int32, ctypes.c_int64, ctypes.c_int32]\n"
            "for nb, ns in [(8 * (64 * 101 + 64 * 64) + 1040, 8 * 64 * 64 + 16), (4096, 3), (1, 1)]:\n"
            "    rc = L.ttx_k_rccl_selftest(0, nb, ns)\n"
            "    assert rc == 0, L.ttx_last_error().decode()\n"
            "print('SELFTEST OK')") % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert p.returncode == 0 and "SELFTEST OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def _spawn_ranks(world, argv, extra_env=None, timeout=600, name=None):
    """`world` processes with RANK / WORLD_SIZE (and the TTX_WORLD_* twins the Fortran layer reads), a fresh shm name each."""
    import os
    import subprocess
    import uuid
    name = name or "ttx_" + uuid.uuid4().hex[:12]
    procs = []
    for rk in range(world):
        env = dict(os.environ, RANK=str(rk), WORLD_SIZE=str(world), TTX_WORLD_RANK=str(rk), TTX_WORLD_SIZE=str(world),
                   TTX_SHM_NAME=name, TTX_TRANSPORT="shm", HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.update(extra_env or {})
        procs.append(subprocess.Popen(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    outs = []
    for p in procs:
        try:
            o, e = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((p.returncode, o, e))
    return outs


@pytest.mark.parametrize("world,args,pipeline", [(2, "c 6 33 20 2 4", "1"), (2, "c 64 51 32 2 8", "1"), (3, "d 8 33 10 2 3", "1"), (4, "c 16 51 32 2 8", "1"),
                                                 (2, "c 64 51 32 2 8", "0")],
                         ids=["w2_c6_g4", "w2_c64_g8", "w3_d8_g3", "w4_c16_g8", "w2_c64_g8_hostsync"])
def test_multi_process_shm_transport(world, args, pipeline):
    """The N>1 path without torch or MPI: `world` engine processes on this one card over the engine's built-in
    shared-memory transport (RCCL refuses several ranks on one device).  The exchange is stream-ordered (host functions in
    the engine's stream), so the Ising C cases run the PIPELINED loop with the cluster kernel -- the control flow of the
    multi-GPU job -- and must be bit-identical to the oracle's virtual ranks; once more with the host-synchronised loop."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = _spawn_ranks(world, [sys.executable, os.path.join(root, "tests", "mp_worker.py")] + args.split() + ["shm"], {"TTX_PIPELINE": pipeline})
    for rc, o, e in outs:
        assert rc == 0 and " OK" in o, o[-2000:] + e[-2000:]


@pytest.mark.parametrize("world,args", [(2, "c 6 33 20 2 4"), (3, "d 8 33 10 2 3"), (4, "c 16 51 32 2 8")], ids=["w2_c6_g4", "w3_d8_g3", "w4_c16_g8"])
def test_multi_process_post_processing(world, args):
    """dtt_accchk, norm, dot_product, ztt_quad, dtt_write and ttx_replicate on the engines of a MULTI-PROCESS job (they used to be
    refused there): collective calls over the job's transport, compared inside every worker with the same job run as one process --
    accchk identical, norm / dot 1e-12, ztt_quad 1e-13, the replica's cores and the written file identical."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = _spawn_ranks(world, [sys.executable, os.path.join(root, "tests", "mp_worker.py")] + args.split() + ["shm"], {"TTX_MP_UTILS": "1"})
    for rc, o, e in outs:
        assert rc == 0 and " OK" in o, o[-3000:] + e[-3000:]


@pytest.mark.parametrize("world,args", [(3, "d 8 33 10 2 3"), (2, "mvn 6 17 8 2 4"), (2, "e 20 9 6 3 2")])
def test_multi_process_fast_mode_equals_single_process_fast_mode(world, args):
    """TTX_ARITH=fast on a multi-process job (persistent per-bond tables of Ising D/E and mvn, boundary pivots' entries built from
    the RECEIVED messages): every record and every core identical to the single-process engine in the same mode and groups."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = _spawn_ranks(world, [sys.executable, os.path.join(root, "tests", "mp_worker.py")] + args.split() + ["shm"], {"TTX_MP_FAST": "1"})
    for rc, o, e in outs:
        assert rc == 0 and " OK" in o, o[-2000:] + e[-2000:]


def test_shm_transport_survives_stale_and_reused_segment_names():
    """The attach handshake of ttx_comm_init_shm (a nonce per initialisation): (1) a job whose processes die without closing
    leaves its segment behind under the name -- ready = 1, handshake over --; the next job under the SAME name must not join
    that segment; (2) two dtt_dmrgg-like jobs in a row inside the same processes reuse the name while rank 0 replaces the
    segment.  Both must end bit-identical to the oracle (before the handshake the ranks could wait on different barriers)."""
    import os
    import sys
    import uuid
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    name = "ttx_stale_" + uuid.uuid4().hex[:8]
    cmd = [sys.executable, os.path.join(root, "tests", "mp_worker.py")] + "c 6 33 20 2 4 shm".split()
    try:
        for rc, o, e in _spawn_ranks(2, cmd, {"TTX_MP_LEAK": "1"}, name=name):
            assert rc == 0 and " OK" in o, o[-2000:] + e[-2000:]
        assert os.path.exists("/dev/shm/" + name), "the leaked segment should still be there"
        for rc, o, e in _spawn_ranks(2, cmd, name=name):
            assert rc == 0 and " OK" in o, o[-2000:] + e[-2000:]
        for rc, o, e in _spawn_ranks(3, [sys.executable, os.path.join(root, "tests", "mp_worker.py")] + "d 8 33 10 2 3 shm".split(), {"TTX_MP_REPEAT": "3"}, name=name):
            assert rc == 0 and o.count(" OK") == 3, o[-2000:] + e[-2000:]
    finally:
        if os.path.exists("/dev/shm/" + name):
            os.unlink("/dev/shm/" + name)


def test_team_halfstep_fault_is_replayed_without_teams(monkeypatch):
    """k_halfstep_det reports a launch whose grid is smaller than the number of units (never expected: the host sizes the grid
    from its bound on the ranks) in ctl[3]; ttx_run must see the report after the run -- the finalisation used to clear it --,
    retire the teams for the engine and repeat the run.  TTX_DE_TEST_FAULT=2 gives the team launches of sweep 2 a grid of one."""
    monkeypatch.setenv("TTX_DE_CUT", "0")                 # the wave teams belong to the full-table kernels of round 2
    monkeypatch.setenv("TTX_DE_TEST_FAULT", "2")
    monkeypatch.setenv("TTX_DE_TEAM_UNITS", "1000000")
    s = D.ising_setup("d", 20, 17)
    tt, oo = _run_both(s, 8, 2)
    assert tt.det_fallbacks == 1
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d])
    assert [a["val"] for a in tt.sweeps()] == [b["val"] for b in oo["sweeps"]]
    assert tt.neval == oo["neval"] and tt.quad(s["quad"]) == oo["value"]
    tt.run()                                   # the engine stays on the wave-per-unit kernel: no second fallback
    assert tt.det_fallbacks == 1 and tt.quad(s["quad"]) == oo["value"]


@pytest.mark.parametrize("world,name", [(2, "ising_C_6_33_20_2_np4"), (4, "ising_C_6_33_20_2_np4"), (2, "ising_C_16_51_32_2_np8")])
def test_fortran_driver_multi_process(world, name):
    """The Fortran drop-in as a multi-process job (one process per GPU in production; here the ranks share the card):
    TTX_WORLD_RANK / TTX_WORLD_SIZE, bond groups by TTX_NGROUPS, transport TTX_TRANSPORT=shm.  Rank 0 prints the
    reference's log -- compared with the golden log of the reference under mpiexec -np <groups> (patched build)."""
    import os
    from conftest import fortran_exe
    from golden_util import GOLDEN, parse_log
    exe = fortran_exe("test_crs_ising")
    t = name.split("_")
    ng = int(t[-1][2:])
    outs = _spawn_ranks(world, [exe] + t[1:-1], {"TTX_NGROUPS": str(ng)})
    for rc, o, e in outs:
        assert rc == 0, o[-2000:] + e[-2000:]
    g_rows, g_val, g_nev = parse_log(open(os.path.join(GOLDEN, name + ".txt")).read())
    o_rows, o_val, o_nev = parse_log(outs[0][1])
    assert len(g_rows) == len(o_rows)
    need = 17 if "C_6" in name else 18                 # as tests/test_oracle_golden.py for these logs
    k = 0
    for a, b in zip(g_rows, o_rows):
        if a["erank"] == b["erank"] and a["neval"] == b["neval"] and abs(a["val"] - b["val"]) <= 2e-13 * abs(a["val"]):
            k += 1
        else:
            break
    assert k >= need, f"only {k} leading sweeps match the reference (need {need})"
    assert abs(g_val - o_val) <= 1e-13 * abs(g_val)
    assert all(len(parse_log(o)[0]) == 0 for _, o, _ in outs[1:]), "only rank 0 prints the sweep log"


@pytest.mark.parametrize("name", ["ising_C_6_33_20_2", "ising_C_8_25_12_3", "ising_D_6_33_12_2", "ising_C_5_17_8_0", "ising_C_16_33_24_0"])
def test_fortran_dropin_driver_matches_reference_log(name):
    """The Fortran drop-in layer (ttcross_amd/fortran: modules named like the reference's, drivers with the
    reference's CLI) on the GPU against the golden stdout of the GENUINE reference."""
    import os
    import subprocess
    from golden_util import GOLDEN, parse_log
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from conftest import fortran_exe
    exe = fortran_exe("test_crs_ising")
    argv = name.split("_")[1:]
    out = subprocess.run([exe] + argv, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    g_rows, g_val, g_nev = parse_log(open(os.path.join(GOLDEN, name + ".txt")).read())
    o_rows, o_val, o_nev = parse_log(out.stdout)
    assert len(g_rows) == len(o_rows) and g_nev == o_nev
    for a, b in zip(g_rows, o_rows):
        assert a["it"] == b["it"] and a["dir"] == b["dir"] and a["erank"] == b["erank"] and a["neval"] == b["neval"]
        assert abs(a["val"] - b["val"]) <= 2e-13 * abs(a["val"])
    assert abs(g_val - o_val) <= 1e-14 * abs(g_val)


@pytest.mark.parametrize("m,n,r,piv,nlot,ng", [(6, 33, 12, 2, 2000, 1), (8, 25, 10, 3, 5000, 1), (8, 25, 10, 3, 1500, 3)])
def test_accchk(m, n, r, piv, nlot, ng):
    """dtt_accchk (A14): the engine vs the oracle (same RNG stream position, same samples; the per-sample values are
    bit-identical so einf, ainf and the worst index must match exactly; the two Frobenius sums are accumulated
    in sample order on the host) and vs the GENUINE reference's output (tests/golden/accchk_*.txt)."""
    import os
    from golden_util import GOLDEN
    s = D.ising_setup("c", m, n)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], nproc=ng).run()
    oo = O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], nproc=ng, accchk=nlot)
    g, o = tt.accchk(nlot), oo["accchk"]
    assert g["einf"] == o["einf"] and g["ainf"] == o["ainf"] and np.array_equal(g["pivot"], o["pivot"])
    assert g["efro"] == o["efro"] and g["afro"] == o["afro"]
    f = os.path.join(GOLDEN, f"accchk_C_{m}_{n}_{r}_{piv}_{nlot}.txt")
    if ng == 1 and os.path.exists(f):
        lines = open(f).read().split("\n")
        ref = [float(x) for x in lines[0].split()[1:]]
        refpiv = [int(x) for x in lines[1].split()[1:]]
        assert list(g["pivot"]) == refpiv
        assert g["ainf"] == ref[2] and abs(g["afro"] - ref[3]) <= 1e-14 * ref[3]
        assert abs(g["einf"] - ref[0]) <= 1e-6 * ref[0] and abs(g["efro"] - ref[1]) <= 1e-6 * ref[1]


def _full(cores):
    """dense tensor of a small TT (numpy, test-side only)"""
    t = cores[0]
    for c in cores[1:]:
        t = np.tensordot(t, c, axes=([t.ndim - 1], [0]))
    return t.reshape(t.shape[1:-1])


@pytest.mark.parametrize("m,n,r,piv,ng,env", [(6, 33, 12, 2, 1, {}), (10, 25, 16, 2, 1, {}), (7, 9, 8, 2, 3, {}), (9, 51, 32, 2, 1, {}),
                                              (9, 51, 32, 2, 1, {"TTX_QR_OWN": "0", "TTX_SVD_POLL": "0"}), (9, 51, 32, 2, 1, {"TTX_QR_PANEL": "64", "TTX_QR_THREADS": "512"})],
                         ids=["c6", "c10", "c7_3groups", "c9_r32_tsqr", "c9_r32_lds_qr_and_copied_rank", "c9_r32_short_panels_8_waves"])
# c9: 1632 x 32 unfoldings, tall-skinny QR over several workgroups; default = register-resident QR (k_qr_own) and the polled rank report
def test_tt_ort_svd_norm_dot(m, n, r, piv, ng, env, monkeypatch):
    """N1 (A12/A13): dtt_ort / dtt_svd / dtt_norm / dtt_dot / dtt_ijk on the device against the oracle's restatement
    and the GENUINE reference's numbers (tests/golden/ttops_*.txt).  Floating point: LAPACK's QR/SVD are restated
    (Householder with a different reduction order, Jacobi SVD, fp64 MFMA GEMMs): tolerance 1e-11 relative to the
    norm; truncation ranks must be identical."""
    import os
    from golden_util import GOLDEN
    from test_oracle_ttops import _fixture, probe_indices
    for k_, v_ in env.items():
        monkeypatch.setenv(k_, v_)
    s = D.ising_setup("c", m, n)
    mk = lambda: E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], nproc=ng).run()
    tt = mk()
    cores0 = [tt.core(k) for k in range(1, tt.d + 1)]
    ot = O.OracleTT(cores0)
    nrm0 = ot.norm()
    assert abs(tt.norm() - nrm0) <= 1e-12 * nrm0
    assert np.array_equal(tt.ranks(), ot.ranks)                      # norm() leaves the TT untouched
    assert all(np.array_equal(tt.core(k), cores0[k - 1]) for k in range(1, tt.d + 1))
    assert abs(tt.dot(tt) - ot.dot(ot)) <= 1e-12 * nrm0 ** 2
    ind = probe_indices(m, n, 2)
    assert abs(tt.tijk(ind) - ot.ijk(ind)) <= 1e-13 * abs(ot.ijk(ind))
    # ort: same tensor, orthonormal unfoldings (up to the reference's norm equalisation)
    t1 = mk().ort()
    o1 = O.OracleTT(cores0)
    o1.ort()
    assert np.array_equal(t1.ranks(), o1.ranks)
    c1 = [t1.core(k) for k in range(1, t1.d + 1)]
    scale = nrm0 ** (1.0 / t1.d)
    for k in range(t1.d - 1):
        u = c1[k].reshape(-1, c1[k].shape[2], order="F") / scale
        assert np.allclose(u.T @ u, np.eye(u.shape[1]), atol=1e-12)
    for k in range(1, 5):
        ind = probe_indices(m, n, k)
        assert abs(t1.tijk(ind) - ot.ijk(ind)) <= 1e-11 * nrm0 / np.sqrt(float(n) ** (m - 1)) + 1e-12 * abs(ot.ijk(ind))
    if m <= 7:
        assert np.allclose(_full(c1), _full(cores0), rtol=0, atol=1e-12 * np.abs(_full(cores0)).max())
    # svd: identical truncation ranks, norms / dots / elements to tolerance
    fx = None
    f = os.path.join(GOLDEN, f"ttops_C_{m}_{n}_{r}_{piv}.txt")
    if ng == 1 and os.path.exists(f):
        fx = _fixture(os.path.basename(f))
    for case, (tol, rmax) in enumerate([(1e-4, 0), (1e-8, 0), (1e-12, 5)], start=1):
        t2 = mk().svd(tol, rmax)
        o2 = O.OracleTT(cores0)
        o2.svd(tol, rmax)
        assert np.array_equal(t2.ranks(), o2.ranks), f"svd case {case}: ranks {t2.ranks()} vs {o2.ranks}"
        assert abs(t2.norm() - o2.norm()) <= 1e-11 * nrm0
        assert abs(tt.dot(t2) - ot.dot(o2)) <= 1e-11 * nrm0 ** 2
        for k in range(1, 5):
            ind = probe_indices(m, n, k)
            assert abs(t2.tijk(ind) - o2.ijk(ind)) <= 1e-9 * abs(ot.ijk(ind))
        if fx:
            assert list(t2.ranks()) == [int(x) for x in fx["ranks_svd"][case - 1][1:]]
            assert abs(t2.norm() - float(fx["norm_svd"][case - 1][1])) <= 1e-11 * nrm0
            assert abs(tt.dot(t2) - float(fx["dot_svd"][case - 1][1])) <= 1e-11 * nrm0 ** 2


def test_zquad_complex_weights():
    """N2 (A15): ztt_quad with the complex weights of the characteristic-function driver, batched over frequencies,
    against the oracle (tolerance 1e-13 of |value|) and the GENUINE reference (tests/golden/zquad_*.txt)."""
    import os
    from golden_util import GOLDEN
    m, n, r, piv = 6, 33, 12, 2
    s = D.ising_setup("c", m, n)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"]).run()
    ot = O.OracleTT([tt.core(k) for k in range(1, tt.d + 1)])
    sc = float(n // 2)
    x = s["par"][:n]
    W = np.array([np.tile((1.0 / sc) * np.exp(1j * (k * np.pi / 300.0) * np.exp(x) / (m - 1)), m - 1) for k in range(8)])
    got = tt.zquad(W)
    for k in range(8):
        want = ot.zquad(W[k])
        assert abs(got[k] - want) <= 1e-13 * abs(want)
    ref = [l.split() for l in open(os.path.join(GOLDEN, "zquad_C_6_33_12_2.txt"))]
    for k in range(8):
        want = complex(float(ref[k][2]), float(ref[k][3]))
        assert abs(got[k] - want) <= 1e-12 * abs(want)


# the last two: piv = 1 and ranks above 32 (full-width triangular solves) on every path; for them the path asked for must be the one
# that runs (a silent fall-back to the chain would hide the other two)
PATH_CHECKED = [("c", 15, 2, 3, 1, 1), ("c", 6, 9, 48, 1, 4)]


@pytest.mark.parametrize("fused", ["chain", "fused", "cluster"])
@pytest.mark.parametrize("kind,m,n,r,piv,nproc", [("c", 16, 51, 32, 2, 1), ("c", 64, 51, 32, 2, 8), ("c", 8, 25, 12, 3, 2), ("c", 5, 17, 8, 0, 1), ("c", 16, 33, 24, 0, 5)] + PATH_CHECKED)
def test_both_sweep_paths_bit_exact(monkeypatch, fused, kind, m, n, r, piv, nproc):
    """The three sweep implementations -- multi-kernel chain, one workgroup per group (ttx_fused.h), a cluster of
    workgroups per group (ttx_cluster.h) -- selected with TTX_SWEEP, each bit for bit against the oracle."""
    monkeypatch.setenv("TTX_SWEEP", fused)
    s = D.ising_setup(kind, m, n)
    tt, oo = _run_both(s, r, piv, nproc=nproc, path=fused if (kind, m, n, r, piv, nproc) in PATH_CHECKED else None)
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d])
    assert [a["val"] for a in tt.sweeps()] == [b["val"] for b in oo["sweeps"]]
    assert [a["neval"] for a in tt.sweeps()] == [b["neval"] for b in oo["sweeps"]]
    assert tt.quad(s["quad"]) == oo["value"]


@pytest.mark.parametrize("kind,m,n,r,piv,own", [("c", 13, 17, 10, 2, [1, 3, 4, 9, 12]), ("d", 9, 9, 6, 3, [1, 2, 8]), ("c", 20, 9, 8, 1, [1, 18, 19])])
def test_user_supplied_bond_groups_bit_exact(kind, m, n, r, piv, own):
    """`mybonds` given by the caller (lib/dmrgg.f90:126-130 takes it instead of share()): uneven groups incl. one-bond groups."""
    s = D.ising_setup(kind, m, n)
    ng = len(own) - 1
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=ng, mybonds=own).run()
    oo = O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=ng, mybonds=own)
    _assert_identical(tt, oo)
    assert tt.quad(s["quad"]) == oo["value"]


def test_mode_larger_than_the_first_is_refused_for_builtin_integrands():
    s = _ising_problem([9, 9, 11, 9])
    with pytest.raises(E.TTXError, match="more than the first mode"):
        E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"], quad=s["quad"])


@pytest.mark.parametrize("own", [[0, 3, 5], [1, 3, 6], [2, 3, 5], [1, 3, 3, 5], [1, 4, 3, 5]])
def test_bad_bond_groups_are_refused(own):
    s = D.ising_setup("c", 6, 9)            # d = 5: bonds 1..4, own must run from 1 to 5
    with pytest.raises(E.TTXError, match="mybonds"):
        E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=2, accuracy=s["acc"], quad=s["quad"], nproc=len(own) - 1, mybonds=own)


@pytest.mark.parametrize("env", [{}, {"TTX_DE_LOT_POINT": "0"}, {"TTX_DE_LANE": "1"}, {"TTX_DE_V2": "0"},
                                 {"TTX_DE_CUT": "0"}, {"TTX_DE_CUT": "0", "TTX_DE_FASTDIV": "0"}, {"TTX_DE_CUT": "0", "TTX_LOTTERY_ROWS": "2"},
                                 {"TTX_DE_CUT": "0", "TTX_LOTTERY_WAVE": "0"}, {"TTX_DE_CUT": "0", "TTX_DE_V5": "1"}, {"TTX_DE_CUT": "0", "TTX_DE_V2": "0"},
                                 {"TTX_DE_CUT": "0", "TTX_DE_TEAM": "0"}, {"TTX_DE_CUT": "0", "TTX_DE_TEAM_UNITS": "1000000"},
                                 {"TTX_DE_CUT": "0", "TTX_DE_TEAM_UNITS": "1000000", "TTX_DE_FASTDIV": "0"},
                                 {"TTX_DE_CUT": "0", "TTX_DE_TEAM_UNITS": "0", "TTX_DE_TEAM6_UNITS": "1000000"}],
                         ids=["compact_tables_default", "lottery_from_compact_tables", "unit_cut_lane_per_element_no_tables", "compact_tables_generic_kernels",
                              "full_tables_round2_default", "general_division", "lottery_rows_with_tables", "lottery_lane_per_candidate", "relay_halfstep",
                              "lane_per_element", "wave_per_unit_halfstep", "team_halfstep_always", "team_halfstep_general_division",
                              "six_wave_team_halfstep_always"])
def test_ising_de_kernel_variants_bit_exact(env, monkeypatch):
    """Every selectable variant of the D/E kernels gives the oracle's bits.  Round 3 (default for nodes in [0,1]): the compact tables whose
    rows end at the unit cut (k_de_ctables, k_halfstep_dec, the row-parallel point evaluator of lottery candidates and boundary corners;
    second case: the lottery candidates from the compact tables as at d > 160, k_lottery_eval_dec), the same cut with one
    lane per element and no tables, the compact tables through the generic lane-per-element kernels.  TTX_DE_CUT=0 -- the kernels
    of round 2 on the full pair triangle: the IEEE division instead of the short sequence for nodes in [0,1], the row-wise lottery
    with the pivots' factor tables (default: without), the lottery and the boundary corners with one lane per element, the
    four-wave relay half-step, the round-1 lane-per-element kernels, the half-step without the 16-wave teams (default: teams while
    the ranks are small) and with teams at every rank.  The second case has two bond groups (boundary corners)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for kind, m, n, r, piv, ng in [("d", 45, 9, 6, 2, 1), ("e", 38, 5, 5, 3, 2)]:
        s = D.ising_setup(kind, m, n)
        tt, oo = _run_both(s, r, piv, nproc=ng)
        assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d])
        assert [a["val"] for a in tt.sweeps()] == [b["val"] for b in oo["sweeps"]]
        assert tt.neval == oo["neval"] and tt.quad(s["quad"]) == oo["value"]


# the wave half-steps (one wave per pivot and 64-mode chunk): kernel -> (switches, what plan()["halfstep"] says or begins with)
WAVE_KERNELS = {
    "dec": ({}, "k_halfstep_dec"),
    "de_true": ({"TTX_DE_CUT": "0", "TTX_DE_TEAM": "0"}, "k_halfstep_de<true>"),
    "de_false": ({"TTX_DE_CUT": "0", "TTX_DE_TEAM": "0", "TTX_DE_FASTDIV": "0"}, "k_halfstep_de<false>"),
    "det_true_3": ({"TTX_DE_CUT": "0", "TTX_DE_TEAM_UNITS": "1000000"}, "k_halfstep_det<true,3>[<=1000000], "),
    "det_true_1": ({"TTX_DE_CUT": "0", "TTX_DE_TEAM_UNITS": "0", "TTX_DE_TEAM6_UNITS": "1000000"},
                   "k_halfstep_det<true,3>[<=0], k_halfstep_det<true,1>[<=1000000], "),
    "de5_true": ({"TTX_DE_CUT": "0", "TTX_DE_V5": "1"}, "k_halfstep_de5<true>"),
    "mvn": ({}, "k_halfstep_mvn"),
}
# (kind, m or d, n, r, piv, groups).  d: two chunks, the second with 5 live lanes -- rook search, then piv = 0 (modes 1 and 2, no
# residual, amax untouched in mode 1); e: three chunks, id 3 without the b-part, two bond groups, pivots in the second chunk
WAVE_ISING_SHAPES = [("d", 9, 69, 3, 2, 1), ("d", 9, 69, 3, 0, 1), ("e", 8, 129, 3, 1, 2)]
WAVE_MVN_SHAPES = [("mvn", 6, 69, 3, 2, 1), ("mvn", 6, 69, 3, 0, 2)]


@pytest.fixture(scope="module")
def wave_oracle():
    """The oracle's run per shape, made once, shared by the kernels and left unchanged."""
    runs = {}

    def run(shape, s):
        if shape not in runs:
            kind, m, n, r, piv, ng = shape
            runs[shape] = O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], aux=s["aux"], nproc=ng)
        return runs[shape]
    return run


@pytest.mark.parametrize("kernel", list(WAVE_KERNELS))
def test_wave_halfsteps_at_several_chunks_bit_exact(kernel, monkeypatch, wave_oracle):
    """k_halfstep_dec, _de, _det, _de5 and _mvn with n = 69 and n = 129: a pivot's fiber takes two or three waves, so the split
    of the slot w into (pivot, chunk), a last chunk with few live lanes and the linear index t of a later chunk are exercised --
    the other tests of these kernels have at most 64 modes, except k_halfstep_dec at the full D_256 (mvn: n = 33).  The kernel
    asked for must be the one the plan names, on the chain path.  The cores are compared with the oracle's: at these shapes most
    pivots lie below mode 64 (only the E shape takes some above), so a wrong store of a later chunk shows in the cores."""
    env, halfstep = WAVE_KERNELS[kernel]
    monkeypatch.setenv("TTX_SWEEP", "chain")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for shape in (WAVE_MVN_SHAPES if kernel == "mvn" else WAVE_ISING_SHAPES):
        kind, m, n, r, piv, ng = shape
        s = D.box_setup("mvn", m, n) if kind == "mvn" else D.ising_setup(kind, m, n)
        tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], aux=s["aux"], nproc=ng)
        assert tt.sweep_path() == "chain"
        hs = tt.plan()["halfstep"]
        assert hs.startswith(halfstep) if halfstep.endswith(", ") else hs == halfstep, hs
        tt.run()
        oo = wave_oracle(shape, s)
        assert len(oo["sweeps"]) == 3 and max(oo["r"]) == r      # the initial cross and two sweeps; the ranks reach r
        _assert_identical(tt, oo, cores=True)
        assert tt.quad(s["quad"]) == oo["value"]
        if kernel == "de5_true":
            assert tt.det_fallbacks == 0         # a silent replay on k_halfstep_de must not pass for the relay


def test_full_size_d256_against_reference_value():
    """BASELINE config 5 at FULL size (Ising D_256, n=101, r=64, PIV=5; 255 cores, 7.4e7 O(d^2) evaluations), 8 bond
    groups on one GPU.  No oracle run at this size (minutes of CPU): the size-independent property is the integral
    itself -- BASELINE.md's value of the genuine reference (8 ranks: 0.30027620068537628e-1, 1 rank: ...538038e-1;
    they differ by 1.4e-14) -- plus the reference's own stop behaviour (38 sweeps to maxrank... 63 would be the cap;
    the accuracy rule never fires here) and the evaluation count within 0.1 % of the reference's 73 621 774."""
    s = D.ising_setup("d", 256, 101)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], 64, pivoting=5, accuracy=s["acc"], quad=s["quad"], nproc=8).run()
    v = tt.quad(s["quad"])
    assert abs(v - 0.030027620068538038) <= 1e-12 * abs(v)
    assert abs(tt.neval - 73621774) <= 1e-3 * 73621774
    acc = tt.accchk(2000)
    assert acc["einf"] <= 1e-9 * acc["ainf"]


def test_config5_d256_full_size_vs_oracle_fixture_and_reference_log():
    """BASELINE config 5 at FULL size (test_crs_ising D 256 101 64 5; 255 cores, ranks to 64, PIV = 5, 38 sweeps, 7.4e7 evaluations of a
    32 640-factor product), 8 bond groups on one GPU, through the C-ABI against
      * the per-sweep fixture of the ORACLE with 8 virtual ranks (tests/golden/oracle_ising_D_256_101_64_5_np8.npz, made in the build
        container by tests/golden/make_oracle_fixture.py in 9 minutes; the oracle's bit-neutral unit-factor shortcut is pinned by
        tests/test_oracle_golden.py::test_unit_skip_changes_no_bit): EVERYTHING it holds must be identical -- 38 sweeps of pivot
        tapes, erank, n_evals, val, amax, pivotmax, the final ranks, the evaluation count and the integral;
      * the log of the GENUINE reference under mpiexec -np 8 (tests/golden/ising_D_256_101_64_5_np8.txt): the leading sweeps
        (erank, n_evals, val to 2e-13) as for the other golden logs -- the reference sums with MKL, a near-tie turns a later pivot --,
        the same number of sweeps, the integral to 1e-13."""
    import os
    from golden_util import GOLDEN, parse_log
    f = np.load(os.path.join(GOLDEN, "oracle_ising_D_256_101_64_5_np8.npz"))
    s = D.ising_setup("d", 256, 101)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], 64, pivoting=5, accuracy=s["acc"], quad=s["quad"], nproc=8).run()
    rows = tt.sweeps()
    assert len(rows) == len(f["it"]) == 39
    assert np.array_equal(tt.tapes()[:, 1:tt.d].astype(np.int16), f["tapes"][:, 1:tt.d]), "pivot tapes differ"
    assert [a["neval"] for a in rows] == f["neval"].tolist()
    assert [a["erank"] for a in rows] == f["erank"].tolist()
    assert [a["val"] for a in rows] == f["val"].tolist()
    assert [a["amax"] for a in rows] == f["amax"].tolist() and [a["pivotmax"] for a in rows] == f["pivotmax"].tolist()
    assert np.array_equal(tt.ranks(), f["r"]) and tt.neval == int(f["total_neval"])
    v = tt.quad(s["quad"])
    assert v == float(f["value"])
    g_rows, g_val, g_nev = parse_log(open(os.path.join(GOLDEN, "ising_D_256_101_64_5_np8.txt")).read())
    assert len(g_rows) == len(rows)
    k = 0
    for a, b in zip(g_rows, rows):
        if a["erank"] == round(b["erank"], 1) and a["neval"] == b["neval"] and abs(a["val"] - b["val"]) <= 2e-13 * abs(a["val"]):
            k += 1
        else:
            break
    assert k >= 6, f"only {k} leading sweeps match the reference's log"
    assert abs(v - g_val) <= 1e-13 * abs(g_val) and abs(tt.neval - g_nev) <= 1e-3 * g_nev


def _ising_problem(n_list, ident=1.0):
    """Ising-type problem with RAGGED mode sizes (the API allows arg%n(p) to differ; n(1) must be the largest because
    the integrand addresses the weights at par(n(1)+ind), test_crs_ising.f90:181-183)."""
    nmax = n_list[0]
    x, w = D.lgwt(nmax)
    par = np.zeros(2 * nmax + 1)
    par[:nmax] = (x + 1.0) / 2
    par[nmax:2 * nmax] = 0.5 * w * float(nmax // 2)
    par[2 * nmax] = ident
    quad = [np.full(n, 1.0 / float(nmax // 2)) for n in n_list]
    return dict(n=list(n_list), par=par, quad=quad, fun_id=E.TTX_FUN_ISING, aux=None, acc=500 * D.EPS, tru=None)


EDGE = [("ragged_c", [17, 9, 13, 17, 11], 1.0, 8, 2, 1), ("ragged_c_groups", [17, 9, 13, 17, 11, 5, 16], 1.0, 7, 2, 3),
        ("ragged_d", [15, 7, 11, 15], 2.0, 6, 3, 1), ("d2", [21, 21], 1.0, 9, 2, 1), ("d3_two_groups", [13, 13, 13], 1.0, 6, 1, 2),
        ("maxrank1", [17, 17, 17, 17], 1.0, 1, 2, 1), ("saturating", [3, 3, 3, 3], 1.0, 12, 2, 1), ("maxrank2", [9, 9, 9], 3.0, 2, 0, 1)]


@pytest.mark.parametrize("name,n_list,ident,r,piv,nproc", EDGE, ids=[e[0] for e in EDGE])
def test_edge_cases_bit_exact(name, n_list, ident, r, piv, nproc):
    """Ragged mode sizes, the smallest trains (d = 2, 3), maxrank = 1 (no sweep at all), ranks that saturate below
    maxrank (every later pivot is rejected by the threshold test, lib/dmrgg.f90:599-600)."""
    s = _ising_problem(n_list, ident)
    tt, oo = _run_both(s, r, piv, nproc=nproc)
    gs, os_ = tt.sweeps(), oo["sweeps"]
    assert len(gs) == len(os_)
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d])
    for a, b in zip(gs, os_):
        assert (a["neval"], a["erank"], a["val"], a["amax"], a["pivotmax"]) == (b["neval"], b["erank"], b["val"], b["amax"], b["pivotmax"])
    assert np.array_equal(tt.ranks(), oo["r"])
    for k in range(1, tt.d + 1):
        assert np.array_equal(tt.core(k), oo["cores"][k - 1])
    assert tt.quad(s["quad"]) == oo["value"]


# ---- N3: trains from outside the sweep (ttx_from_tt) and the reference's stream file (lib/ttio.f90) -----------------
def _rand_tt(seed, n, r):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((r[k], n[k], r[k + 1])) for k in range(len(n))]


def test_stream_file_read_write_against_reference_file(tmp_path):
    """ttx_read of the file the GENUINE reference wrote (tests/golden/ttio_5.tt) must give its closed-form cores exactly;
    ttx_write must reproduce the file byte for byte (apart from header bytes the reference never sets)."""
    import os
    from golden_util import GOLDEN
    from test_host_cpu import _closed_form_cores
    from ttcross_amd import ttio
    gold = os.path.join(GOLDEN, "ttio_5.tt")
    tt = E.TTCross.read(gold)
    assert tt.d == 5 and list(tt.ranks()) == [1, 2, 3, 2, 2, 1]
    want = _closed_form_cores()
    assert all(np.array_equal(tt.core(k), want[k - 1]) for k in range(1, 6))
    out = tmp_path / "dev.tt"
    tt.write(out)
    assert ttio.same_file(out, gold)
    # a train read from disk is resident: quadrature, element access and norm work on it
    full = _full(want)
    assert abs(tt.quad() - full.sum()) <= 1e-12 * abs(full.sum())
    assert abs(tt.norm() - np.linalg.norm(full)) <= 1e-12 * np.linalg.norm(full)
    assert abs(tt.tijk([2, 3, 1, 4, 2]) - full[1, 2, 0, 3, 1]) <= 1e-13 * abs(full[1, 2, 0, 3, 1])
    with pytest.raises(E.TTXError, match="no integrand"):
        tt.run()
    with pytest.raises(E.TTXError, match="no integrand"):
        tt.accchk(10)
    with pytest.raises(E.TTXError, match="not exist"):
        E.TTCross.read(tmp_path / "missing.tt")
    bad = tmp_path / "bad.tt"
    bad.write_bytes(b"XX" + open(gold, "rb").read()[2:])
    with pytest.raises(E.TTXError, match="not TT header"):
        E.TTCross.read(bad)
    bad.write_bytes(open(gold, "rb").read()[:300])
    with pytest.raises(E.TTXError, match="error reading cores"):
        E.TTCross.read(bad)


@pytest.mark.parametrize("seed,n,r", [(1, [4, 5, 3, 6], [1, 3, 7, 4, 1]), (2, [7] * 9, [1, 5, 9, 12, 12, 12, 12, 9, 5, 1]),
                                      (3, [33] * 5, [1, 16, 24, 24, 16, 1]), (4, [2, 3], [1, 2, 1]),
                                      (5, [2, 2, 3, 2], [1, 5, 7, 4, 1]), (6, [3, 2, 2, 2, 4], [1, 9, 14, 11, 6, 1]),
                                      # 6464 x 64 unfoldings (the cores of D_256): four levels of the tall-skinny QR, 64 x 64 Jacobi SVD
                                      (7, [101] * 4, [1, 64, 64, 64, 1]),
                                      # 144 x 100 and 1200 x 12 unfoldings: eight columns per wave of the register-resident QR, a wide middle core
                                      (8, [12] * 4, [1, 12, 100, 12, 1])])
def test_uploaded_train_roundtrip_and_tt_lib(tmp_path, seed, n, r):
    """ttx_from_tt: arbitrary (random) trains, not only sweep results, through ort / svd / norm / dot / quad against the
    oracle's tt_lib restatement (tolerances as in test_tt_ort_svd_norm_dot), plus file round trip (bit-exact)."""
    cores = _rand_tt(seed, n, r)
    tt = E.TTCross.from_cores(cores)
    assert list(tt.ranks()) == r
    assert all(np.array_equal(tt.core(k), cores[k - 1]) for k in range(1, len(n) + 1))
    f = tmp_path / "t.tt"
    tt.write(f)
    t2 = E.TTCross.read(f)
    assert all(np.array_equal(t2.core(k), cores[k - 1]) for k in range(1, len(n) + 1))
    ot = O.OracleTT(cores)
    nrm = ot.norm()
    assert abs(tt.norm() - nrm) <= 1e-12 * nrm
    assert abs(tt.dot(t2) - ot.dot(ot)) <= 1e-12 * nrm ** 2
    w = [np.cos(np.arange(1, nk + 1)) for nk in n]
    qref = 1.0
    v = np.ones((1, 1))
    for k, c in enumerate(cores):
        v = v @ np.einsum("ijk,j->ik", c, w[k])
    qref = float(v[0, 0])
    assert abs(tt.quad(w) - qref) <= 1e-11 * nrm
    t2.ort()
    o1 = O.OracleTT(cores)
    o1.ort()
    assert np.array_equal(t2.ranks(), o1.ranks)
    assert abs(t2.norm() - nrm) <= 1e-11 * nrm
    for tol, rmax in [(1e-2, 0), (1e-10, 0), (1e-12, 3)]:
        t3 = E.TTCross.from_cores(cores).svd(tol, rmax)
        o3 = O.OracleTT(cores)
        o3.svd(tol, rmax)
        assert np.array_equal(t3.ranks(), o3.ranks), (tol, rmax, t3.ranks(), o3.ranks)
        assert abs(t3.norm() - o3.norm()) <= 1e-11 * nrm
        assert abs(tt.dot(t3) - ot.dot(o3)) <= 1e-11 * nrm ** 2


def test_fortran_ttio_dropin(tmp_path):
    """ttio_lib drop-in (ttcross_amd/fortran/ttio_lib.f90): `call read(tt,f)` / `call write(tt,f)` on the reference's file."""
    import os
    import subprocess
    from golden_util import GOLDEN
    from ttcross_amd import ttio
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from conftest import fortran_exe
    exe = fortran_exe("test_ttio")
    gold = os.path.join(GOLDEN, "ttio_5.tt")
    p = subprocess.run([exe, gold, str(tmp_path / "copy.tt"), str(tmp_path / "ones.tt")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = {ln.split()[0] + ("_" + ln.split()[1] if ln.split()[1] in ("info", "ones") else ""): ln for ln in p.stdout.splitlines() if ln.strip()}
    ref = open(os.path.join(GOLDEN, "ttio_5.txt")).read().splitlines()
    for key in ("lm", "n", "r", "checksum"):
        assert out[key] == [ln for ln in ref if ln.split()[0] == key][0]
    assert out["read_info"].split()[-1] == "0" and out["write_info"].split()[-1] == "0"
    assert out["missing_info"].split()[-1] == "-1"
    assert ttio.same_file(tmp_path / "copy.tt", gold)
    l, n, r, cores = ttio.read_tt(tmp_path / "ones.tt")
    assert list(n) == [2, 3, 4, 5] and list(r) == [1] * 5 and all(np.all(c == 1.0) for c in cores)


def test_workgroups_are_dealt_round_robin_to_the_xcds():
    """The cluster sweep kernel places the workgroups of a bond group on one XCD by giving them block ids that are
    congruent modulo 8 (ttx_cluster.h).  That is a performance assumption, not a correctness one (its barrier and
    record exchange are agent-scope); this probe documents that it holds on the device under test."""
    import ctypes
    L = E.load_library()
    L.ttx_k_xcc_map.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    out = np.zeros(64, dtype=np.int32)
    assert L.ttx_k_xcc_map(0, 64, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == 0
    assert out.min() >= 0 and out.max() <= 7
    assert all(len(set(out[x::8])) == 1 for x in range(8)), out.tolist()


def test_sweep_path_selection(monkeypatch):
    s = D.ising_setup("c", 6, 33)
    mk = lambda **kw: E.TTCross(s["n"], s["fun_id"], s["par"], 8, pivoting=2, accuracy=s["acc"], quad=s["quad"], **kw)
    for want in ("chain", "fused", "cluster"):
        monkeypatch.setenv("TTX_SWEEP", want)
        assert mk().sweep_path() == want
    monkeypatch.setenv("TTX_SWEEP", "auto")
    assert mk().sweep_path() == "cluster"
    sd = D.ising_setup("d", 6, 33)          # D/E and the exp integrands run on the multi-kernel chain
    assert E.TTCross(sd["n"], sd["fun_id"], sd["par"], 8, pivoting=2).sweep_path() == "chain"
    monkeypatch.setenv("TTX_SWEEP", "bogus")
    with pytest.raises(E.TTXError, match="TTX_SWEEP"):
        mk()


@pytest.mark.parametrize("coop", ["1", "0"])
def test_cluster_abort_falls_back_to_the_chain_path(monkeypatch, coop):
    """Residency safety net of the cluster sweep kernel: a workgroup that never arrives (test hook TTX_CLUSTER_TEST_ABORT =
    launch number) makes its partners time out; the kernel stops the rest of the sweep, ttx_run replays the run on the
    multi-kernel chain and the result is still the oracle's, bit for bit.  Once with the cooperative launch, once plain."""
    monkeypatch.setenv("TTX_CLUSTER_TEST_ABORT", "3")
    monkeypatch.setenv("TTX_CLUSTER_COOP", coop)
    s = D.ising_setup("c", 10, 17)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], 12, pivoting=2, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=2)
    assert tt.sweep_path() == "cluster"
    tt.run()
    assert tt.cluster_fallbacks == 1 and tt.sweep_path() == "chain"
    oo = O.dmrgg(s["n"], s["fun_id"], s["par"], 12, piv=2, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=2)
    _assert_identical(tt, oo)
    assert tt.quad(s["quad"]) == oo["value"]
    tt.run()                                       # the engine stays on the chain path
    assert tt.cluster_fallbacks == 1 and tt.quad(s["quad"]) == oo["value"]


SHAPES = [(21, 17, 33, 3, 3), (9, 33, 48, 0, 2), (18, 3, 40, 0, 2), (15, 2, 3, 1, 1), (6, 9, 48, 1, 4), (4, 2, 6, 3, 2),
          (13, 40, 40, 2, 3), (5, 7, 48, 3, 1), (19, 2, 33, 2, 1), (12, 40, 48, 3, 3), (20, 9, 40, 1, 4), (4, 33, 33, 2, 1),
          # pivoting = 0 run into the noise floor: the acceptance test then depends on amax, which the piv = 0 branch of the
          # reference (lib/dmrgg.f90:492-513) does NOT update with the two fibers it evaluates
          (16, 33, 24, 0, 5), (7, 5, 40, 0, 1), (23, 16, 33, 0, 1)]


@pytest.mark.parametrize("m,n,r,piv,ng", SHAPES, ids=[f"C{c[0]}_n{c[1]}_r{c[2]}_p{c[3]}_g{c[4]}" for c in SHAPES])
def test_cluster_kernel_odd_shapes_bit_exact(m, n, r, piv, ng):
    """The default (cluster) sweep kernel on shapes that stress its slicing: fewer mode indices than workgroups of a
    cluster, ranks above 32 (one triangular solve per wave instead of two), tiny ranks, 1-4 bond groups, every pivoting
    mode -- tapes, per-sweep values, evaluation counts, integral and finalised cores identical to the oracle."""
    s = D.ising_setup("c", m, n)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=ng)
    assert tt.sweep_path() == "cluster"
    tt.run()
    oo = O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=ng)
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d])
    assert [a["val"] for a in tt.sweeps()] == [b["val"] for b in oo["sweeps"]]
    assert [a["neval"] for a in tt.sweeps()] == [b["neval"] for b in oo["sweeps"]]
    assert tt.quad(s["quad"]) == oo["value"]
    assert all(np.array_equal(tt.core(k), oo["cores"][k - 1]) for k in range(1, tt.d + 1))


def test_chf_driver_against_oracle():
    """The caller on the far side of the path: test_crs_chf.f90's pipeline -- cross of the mvn density
    without quad, then the 32 complex quadratures -- through ttcross_amd.drivers.run_chf.  Checked against the oracle:
    ztt_quad of the SAME device train (1e-13), and the oracle's own cross + ztt_quad (exp-based integrand: 1e-9 of the
    k = 0 value, which is the plain integral)."""
    tt, vals, s = D.run_chf(["4", "17", "8", "2"], verbose=False)
    n, d = s["n"][0], len(s["n"])
    W = D.chf_weights(s["par"], n, d)
    ot = O.OracleTT([tt.core(k) for k in range(1, d + 1)])
    for k in range(32):
        want = ot.zquad(W[k])
        assert abs(vals[k] - want) <= 1e-13 * abs(want) + 1e-300
    oo = O.dmrgg(s["n"], s["fun_id"], s["par"], 8, piv=2, accuracy=s["acc"], aux=s["aux"])
    oref = O.OracleTT(oo["cores"])
    scale = abs(oref.zquad(W[0]))
    assert abs(vals[0].imag) <= 1e-12 * scale                  # omega = 0: real weights
    for k in range(32):
        assert abs(vals[k] - oref.zquad(W[k])) <= 1e-9 * scale


def test_fortran_chf_dropin_matches_python_driver():
    """N2 behind the Fortran boundary: the drop-in `ztt` type, `tt_z = tt` and `ztt_quad` (ttcross_amd/fortran) in a
    driver with the pipeline of test_crs_chf.f90, against the Python driver on the same arguments.  Both run the same
    engine; the complex weights come from two different libm's, hence 1e-12 instead of bit equality."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from conftest import fortran_exe
    exe = fortran_exe("test_crs_chf")
    p = subprocess.run([exe, "5", "17", "8", "2"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    got = {int(ln.split()[2]): complex(float(ln.split()[3]), float(ln.split()[4])) for ln in p.stdout.splitlines() if ln.startswith("computed value:")}
    assert sorted(got) == list(range(32))
    _, vals, _ = D.run_chf(["5", "17", "8", "2"], verbose=False)
    scale = abs(vals[0])
    for k in range(32):
        assert abs(got[k] - vals[k]) <= 1e-12 * scale, (k, got[k], vals[k])
