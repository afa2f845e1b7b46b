"""The end of a sweep of the pipelined cluster loop as one exchange launch (k_exch_tail, TTX_TAIL=1, the default) against the
launches it replaces (k_exch_max_apply, k_exch_boundary, k_sweep_end; TTX_TAIL=0): the same engine set-up under both switches in
fresh child processes (tests/sweep_tail_worker.py), everything a run leaves compared BYTE FOR BYTE -- all cores, ranks, the per-sweep
records (val, erank, neval, amax, pivotmax, pivotmin), tapes, the evaluation count and the integral.  TTX_TAIL=1 runs twice: with
the summary on the quadrature's stream and the stopping rule at the sweep kernel's entry (the default), and with k_sweep_end on
the main stream behind the one exchange launch (TTX_TAIL_SIDE=0).
The forms of the sweep loop (ttx_loop_plan.h) against each other in the same way: the host-synchronised loop of one process
(TTX_PIPELINE=0) against the pipelined one, the tail without a quadrature, and what each form launches per kind."""
import os
import subprocess
import sys

import numpy as np
import pytest

from golden_util import GOLDEN, parse_log

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "sweep_tail_worker.py")
SWITCHES = ("TTX_TAIL", "TTX_TAIL_SIDE", "TTX_SWEEP", "TTX_ARITH", "TTX_PIPELINE", "TTX_CLUSTER_TEST_ABORT", "TTX_CLUSTER_COOP", "TTX_CLUSTER_NB", "TTX_CL_PAD")


def _worker(tmp_path, tag, tail, m, n, r, piv, groups, acc="default", runs=1, arith="exact", env=None, noquad=False):
    """tail: the value of TTX_TAIL, or None to leave it unset"""
    out = str(tmp_path / f"{tag}_tail{tail}.npz")
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update({} if tail is None else {"TTX_TAIL": str(tail)}, **(env or {}))
    p = subprocess.run([sys.executable, WORKER, out] + [str(x) for x in (m, n, r, piv, groups, acc, runs, arith)] + ["noquad"] * noquad,
                       capture_output=True, text=True, env=e, timeout=300)
    assert p.returncode == 0 and "WORKER OK" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
    return dict(np.load(out))


def _same_bytes(a, b, keys=None, ta="run0_", tb="run0_"):
    """every array of run `ta` of dump a == the same array of run `tb` of dump b, as bytes (dtype and shape included)"""
    names = sorted(k[len(ta):] for k in a if k.startswith(ta))
    assert names == sorted(k[len(tb):] for k in b if k.startswith(tb)) and any(k.startswith("core") for k in names)
    for k in names:
        if keys is not None and k not in keys:
            continue
        x, y = a[ta + k], b[tb + k]
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{k} differs between the two tails"


def _both(tmp_path, tag, *shape, **kw):
    """TTX_TAIL=0 against TTX_TAIL=1, the latter with the summary on the quadrature's stream (the default) and, TTX_TAIL_SIDE=0, with
    k_sweep_end on the main stream.  Returns (old, new with the defaults)."""
    old, new = _worker(tmp_path, tag, 0, *shape, **kw), _worker(tmp_path, tag, 1, *shape, **kw)
    main = _worker(tmp_path, tag + "_main", 1, *shape, **dict(kw, env=dict(kw.get("env") or {}, TTX_TAIL_SIDE="0")))
    for x in (new, main):
        assert old["path_before"][0] == x["path_before"][0] == "cluster"        # sweep_path() is what it was
        assert old["path_after"][0] == x["path_after"][0]
        _same_bytes(old, x)
    return old, new


@pytest.mark.parametrize("groups", [1, 2, 4, 8])
def test_modes_shorter_than_the_rank(tmp_path, groups):
    """Ising C_12, n = 9, r = 40, piv = 3: modes shorter than the rank.  One group has no messages (no boundary block has work);
    eight groups are one or two bonds each, both sides of every boundary active in every sweep."""
    old, new = _both(tmp_path, f"c12_g{groups}", 12, 9, 40, 3, groups)
    if groups == 1:         # the golden log of the reference covers one group: the leading sweeps as test_oracle_golden.py pins them
        g_rows, g_val, _ = parse_log(open(os.path.join(GOLDEN, "ising_C_12_9_40_3.txt")).read())
        assert len(g_rows) == len(new["run0_sw_it"])
        for k in range(9):
            assert g_rows[k]["erank"] == round(float(new["run0_sw_erank"][k]), 1) and g_rows[k]["neval"] == int(new["run0_sw_neval"][k])
        assert abs(float(new["run0_quad"][0]) - g_val) <= 1e-14 * abs(g_val)


@pytest.mark.parametrize("groups,need", [(2, 17), (4, 20)])
def test_c6_against_the_reference_logs(tmp_path, groups, need):
    """Ising C_6, n = 33, r = 20, piv = 2 with 2 and 4 groups; the new tail also against the reference's log under mpiexec -np <groups>
    (leading sweeps and tolerances as tests/test_oracle_golden.py holds the oracle to them)."""
    old, new = _both(tmp_path, f"c6_g{groups}", 6, 33, 20, 2, groups)
    g_rows, g_val, _ = parse_log(open(os.path.join(GOLDEN, f"ising_C_6_33_20_2_np{groups}.txt")).read())
    assert len(g_rows) == len(new["run0_sw_it"])
    k = 0
    for a, er, ne, va in zip(g_rows, new["run0_sw_erank"], new["run0_sw_neval"], new["run0_sw_val"]):
        if a["erank"] == round(float(er), 1) and a["neval"] == int(ne) and abs(a["val"] - float(va)) <= 2e-13 * abs(a["val"]):
            k += 1
        else:
            break
    assert k >= need, f"only {k} leading sweeps match the reference (need {need})"
    assert abs(float(new["run0_quad"][0]) - g_val) <= 1e-14 * abs(g_val)


@pytest.mark.parametrize("piv", [0, 1, 2])
def test_pivoting(tmp_path, piv):
    _both(tmp_path, f"c8_p{piv}", 8, 25, 12, piv, 3)


def test_three_strikes_end_the_run(tmp_path):
    """An accuracy large enough that the three-strike rule stops the run well before maxrank; its late sweeps carry rejected
    boundary pivots (upd == 0)."""
    old, new = _both(tmp_path, "c8_strikes", 8, 25, 12, 2, 3, acc=1e-3)
    assert 3 <= len(new["run0_sw_it"]) - 1 < 11


def test_rule_off_runs_to_maxrank(tmp_path):
    old, new = _both(tmp_path, "c8_norule", 8, 25, 12, 2, 3, acc=-1.0)
    assert len(new["run0_sw_it"]) - 1 == 11


def test_one_sweep(tmp_path):
    """maxrank = 2: one sweep, no speculative launch"""
    old, new = _both(tmp_path, "c8_r2", 8, 25, 2, 2, 3)
    assert len(new["run0_sw_it"]) - 1 == 1


def test_fast_arithmetic(tmp_path):
    """--arith fast: the apply block also writes the persistent fast tables"""
    old, new = _both(tmp_path, "c12_fast", 12, 9, 40, 3, 4, arith="fast")
    assert old["arith"][0] == new["arith"][0] == "fast"


@pytest.mark.parametrize("side", ["1", "0"])
def test_engine_reuse(tmp_path, side):
    """two run() calls on one engine give identical results: the parity-indexed buffers are reset"""
    new = _worker(tmp_path, "c8_twice", 1, 8, 25, 12, 2, 3, runs=2, env={"TTX_TAIL_SIDE": side})
    _same_bytes(new, new, ta="run0_", tb="run1_")


def test_abort_replay(tmp_path):
    """TTX_CLUSTER_TEST_ABORT=3: the third cluster launch aborts behind two sweeps that ended with the new tail; the replay on the
    chain path gives what TTX_TAIL=0 gives without an abort"""
    old = _worker(tmp_path, "c10_plain", 0, 10, 17, 12, 2, 2)
    new = _worker(tmp_path, "c10_abort", 1, 10, 17, 12, 2, 2, env={"TTX_CLUSTER_TEST_ABORT": "3"})
    assert new["path_before"][0] == "cluster" and new["path_after"][0] == "chain" and int(new["cluster_fallbacks"][0]) == 1
    assert int(old["cluster_fallbacks"][0]) == 0
    _same_bytes(old, new)


C8 = (8, 25, 12, 2)     # Ising C_8, n = 25, r = 12, piv = 2: the shape of the loop-form tests below


@pytest.mark.parametrize("groups,sweep", [(3, "cluster"), (1, "cluster"), (3, "fused")])
def test_host_synchronised_loop_of_one_process(tmp_path, groups, sweep):
    """TTX_PIPELINE=0 with one process on a whole-sweep path: the plain loop, one launch of the sweep kernel and one readback per
    sweep, gives what the pipelined loop gives, and the cluster kernel's barriers hold (no fallback)."""
    env = {} if sweep == "cluster" else {"TTX_SWEEP": sweep}
    pipe = _worker(tmp_path, f"c8_{sweep}_g{groups}_pipe", None, *C8, groups, env=env)
    host = _worker(tmp_path, f"c8_{sweep}_g{groups}_host", None, *C8, groups, env=dict(env, TTX_PIPELINE="0"))
    for x in (pipe, host):
        assert x["path_before"][0] == x["path_after"][0] == sweep and int(x["cluster_fallbacks"][0]) == 0
    _same_bytes(pipe, host)


def test_tail_without_a_quadrature(tmp_path):
    """no quadrature weights: the one-launch tail with k_sweep_end behind it and nothing forked, against the launches it replaces"""
    old, new = (_worker(tmp_path, "c8_noquad", t, *C8, 3, noquad=True) for t in (0, 1))
    assert old["path_after"][0] == new["path_after"][0] == "cluster"
    _same_bytes(old, new)


@pytest.mark.parametrize("case,groups,env,acc,pipelined,tail", [
    ("default", 3, {}, "default", True, True),
    ("tail_on_the_main_stream", 3, {"TTX_TAIL_SIDE": "0"}, "default", True, True),
    ("no_tail", 3, {"TTX_TAIL": "0"}, "default", True, False),
    ("one_group", 1, {}, "default", True, False),
    ("fused", 3, {"TTX_SWEEP": "fused"}, "default", True, False),
    ("host_synchronised", 3, {"TTX_PIPELINE": "0"}, "default", False, False),
    ("three_strikes", 3, {}, 1e-3, True, True),
    ("rule_off", 3, {}, -1.0, True, True),
])
def test_launch_counts_per_kind(tmp_path, case, groups, env, acc, pipelined, tail):
    """What a whole-sweep run launches per kind, in closed form from the brackets of the driver as it stood before the loop plan
    (S sweeps, R = maxrank, G groups): 4 launches of the initial cross and 2 of the finalisation; one sweep kernel per sweep, plus
    the speculative one of the pipelined loop unless the last sweep was R - 1; the end of a sweep as one exchange launch with the
    tail, else max-apply and (cluster: packed by the sweep kernel) pack or boundary -- 2, and the boundary launch on top with
    neighbours; the quadrature as build and chain, and the tree with several groups.  So the switch a case sets selects the form
    that runs."""
    R, G = C8[2], groups
    x = _worker(tmp_path, "c8_" + case, None, *C8, groups, acc=acc, env=env)
    S = int(x["nsweeps"][0]) - 1
    assert 1 <= S <= R - 1 and x["path_after"][0] == env.get("TTX_SWEEP", "cluster")
    if case == "three_strikes":
        assert S < R - 1
    if case == "rule_off":
        assert S == R - 1
    got = {k[len("launches_"):]: int(v[0]) for k, v in x.items() if k.startswith("launches_")}
    assert got == {"lottery": 0, "accept": 0, "other": 6,
                   "halfstep": S + (1 if S < R - 1 else 0) if pipelined else S,
                   "exchange": S if tail else S * (2 + (1 if G > 1 else 0)),
                   "quad": S * (3 if G > 1 else 2)}
