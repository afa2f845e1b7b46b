"""The two ends of a run around its sweeps in their new forms against the old ones: the initial summary written by k_init_final
straight into the pinned slot (TTX_HEAD_DIRECT), k_init_samples in one pass with the mode sizes in LDS (TTX_INIT_WIDE), k_init_final
with one wave per core (TTX_INIT_WAVE), the finalisation behind the last quadrature's k_quad_build with its collect and copy enqueued
ahead (TTX_FIN_EARLY), no final exchange behind a sweep of one process (TTX_FIN_SKIP_EXCH), and the quadrature's tree in LDS
(TTX_QUAD_LDS).  One fresh child process per problem (tests/run_ends_worker.py) runs it with all six switches off, with the
defaults (all on) and with each switch alone; everything a run leaves -- all cores, ranks, the per-sweep records (val, erank, neval,
amax, pivotmax, pivotmin), tapes, the evaluation count and the integral -- is compared BYTE FOR BYTE between the forms, and the
launches per kind are the same in all of them.  Two of the problems also against the oracle, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from ttcross_amd import drivers as D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "run_ends_worker.py")
SWITCHES = ("TTX_HEAD_DIRECT", "TTX_INIT_WIDE", "TTX_INIT_WAVE", "TTX_FIN_EARLY", "TTX_FIN_SKIP_EXCH", "TTX_QUAD_LDS", "TTX_TAIL", "TTX_TAIL_SIDE", "TTX_SWEEP", "TTX_ARITH",
            "TTX_PIPELINE", "TTX_CLUSTER_TEST_ABORT", "TTX_CLUSTER_COOP", "TTX_CLUSTER_NB", "TTX_CL_PAD")
FORMS = ("old", "new", "only_head_direct", "only_init_wide", "only_init_wave", "only_fin_early", "only_fin_skip_exch", "only_quad_lds")


def _userfun():
    bdir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(bdir, exist_ok=True)
    so, src = os.path.join(bdir, "libuserfun.so"), os.path.join(ROOT, "tests", "userfun.c")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", so, "-lm"], check=True)
    return so


def _worker(tmp_path, tag, family, m, n, r, piv, groups, arith="exact", runs=1, quad=True, env=None):
    out = str(tmp_path / f"{tag}.npz")
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env or {})
    argv = [sys.executable, WORKER, out, family] + [str(x) for x in (m, n, r, piv, groups, arith, runs)] + ["quad" if quad else "noquad"]
    if family == "host":
        argv.append(_userfun())
    p = subprocess.run(argv, capture_output=True, text=True, env=e, timeout=300)
    assert p.returncode == 0 and "WORKER OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    return dict(np.load(out))


def _same_bytes(x, ta, tb):
    """every array of run `ta` == the same array of run `tb`, as bytes (dtype and shape included)"""
    names = sorted(k[len(ta):] for k in x if k.startswith(ta))
    assert names == sorted(k[len(tb):] for k in x if k.startswith(tb)) and any(k.startswith("core") for k in names)
    for k in names:
        a, b = x[ta + k], x[tb + k]
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f"{k} differs between {ta} and {tb}"


def _forms_agree(x, path=None, runs=1):
    for form in FORMS:
        if path:
            assert x[form + "_path"][0] == path
        assert x[form + "_path"][0] == x["old_path"][0] and x[form + "_arith"][0] == x["old_arith"][0]
        for k in range(runs):
            _same_bytes(x, "old_run0_", f"{form}_run{k}_")
        assert all(int(x[f"{form}_launches_{kind}"][0]) == int(x[f"old_launches_{kind}"][0]) for kind in ("other", "halfstep", "exchange", "quad"))
    return x


def _against_the_oracle(x, s, r, piv, groups):
    oo = O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=groups)
    d = len(s["n"])
    for form in ("old", "new"):
        t = form + "_run0_"
        assert np.array_equal(x[t + "tapes"][:, 1:d], oo["tapes"][:, 1:d])
        assert [int(v) for v in x[t + "sw_neval"]] == [b["neval"] for b in oo["sweeps"]]
        assert [float(v) for v in x[t + "sw_val"]] == [b["val"] for b in oo["sweeps"]]
        assert int(x[t + "neval"][0]) == oo["neval"] and np.array_equal(x[t + "ranks"], oo["r"])
        assert all(np.array_equal(x[f"{t}core{k}"], oo["cores"][k - 1]) for k in range(1, d + 1))
        assert float(x[t + "quad"][0]) == oo["value"]


@pytest.mark.parametrize("groups", [1, 2, 4])
@pytest.mark.parametrize("path", ["cluster", "chain"])
def test_ising_c6(tmp_path, path, groups):
    """Ising C_6, n = 33, r = 20, piv = 2 on the cluster and on the chain path; two groups on the cluster path also against the oracle"""
    x = _forms_agree(_worker(tmp_path, f"c6_{path}_g{groups}", "c", 6, 33, 20, 2, groups, env={"TTX_SWEEP": path}), path)
    if path == "cluster" and groups == 2:
        _against_the_oracle(x, D.ising_setup("c", 6, 33), 20, 2, groups)


@pytest.mark.parametrize("m,groups", [(5, 3), (6, 4)])
def test_a_group_of_one_bond(tmp_path, m, groups):
    """n = 17, r = 8, piv = 0, every group owns a single bond.  Four groups need five dimensions, which is Ising C_6; Ising C_5 has
    four dimensions and three bonds, so it runs with three groups (the engine, like the reference, refuses nproc >= d)."""
    _forms_agree(_worker(tmp_path, f"c{m}_g{groups}", "c", m, 17, 8, 0, groups))


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_ising_d8(tmp_path, arith):
    """Ising D_8, n = 33, r = 10, piv = 2 with three groups; fast: the tables of the rank-1 start and of the apply.  Exact also
    against the oracle."""
    x = _forms_agree(_worker(tmp_path, "d8_" + arith, "d", 8, 33, 10, 2, 3, arith=arith))
    assert x["new_arith"][0] == arith
    if arith == "exact":
        _against_the_oracle(x, D.ising_setup("d", 8, 33), 10, 2, 3)


@pytest.mark.parametrize("arith", ["exact", "fast"])
def test_mvn(tmp_path, arith):
    _forms_agree(_worker(tmp_path, "mvn_" + arith, "mvn", 6, 33, 12, 2, 2, arith=arith))


def test_stdnorm(tmp_path):
    _forms_agree(_worker(tmp_path, "stdnorm", "stdnorm", 4, 33, 10, 2, 2))


def test_host_integrand(tmp_path):
    """the two-pass initial cross: d = 4, n = 9, r = 6, piv = 0, the smallest of the host cases of tests/test_gpu_boundary.py, in two groups"""
    _forms_agree(_worker(tmp_path, "host", "host", 4, 9, 6, 0, 2))


@pytest.mark.parametrize("path", ["cluster", "chain"])
def test_no_sweep_keeps_the_final_exchange(tmp_path, path):
    """maxrank = 1 with four groups: no sweep runs, so the finalisation must still shift inv(last) to the neighbour (the initial
    cross leaves inv(first-1) = 1) -- with the exchange left out the first core of every later group would differ from the old form"""
    x = _forms_agree(_worker(tmp_path, "c6_r1_" + path, "c", 6, 33, 1, 2, 4, env={"TTX_SWEEP": path}))
    assert len(x["new_run0_sw_it"]) == 1 and all(int(v) == 1 for v in x["new_run0_ranks"])


def test_without_quadrature_weights(tmp_path):
    x = _forms_agree(_worker(tmp_path, "c6_noquad", "c", 6, 33, 20, 2, 4, quad=False), "cluster")
    assert len(x["new_run0_sw_it"]) > 2


def test_engine_reuse(tmp_path):
    """two run() calls on one engine give identical results under every form: the second final summary lands in a pinned slot again"""
    _forms_agree(_worker(tmp_path, "c6_twice", "c", 6, 33, 20, 2, 4, runs=2), "cluster", runs=2)


@pytest.mark.parametrize("groups", [4, 8])
def test_ranks_above_32(tmp_path, groups):
    """Ising C_12, n = 9, r = 40, piv = 3.  The tree's two regions of 40 x 40 matrices fit the LDS with four groups and do not with
    eight, where it keeps its global scratch."""
    x = _forms_agree(_worker(tmp_path, f"c12_g{groups}", "c", 12, 9, 40, 3, groups), "cluster")
    assert max(int(v) for v in x["new_run0_ranks"]) > 32
