"""The ordered residual sums of the cluster sweep kernel (cl_ordered_sum, ttx_cluster_rules.h) against the oracle, bit for bit.

A residual sum over the r1 factor entries of a bond is taken in batches (16 terms, then pieces of 8, 4, 2 and 1 by the bits of
the remainder; 8 / 4 / 2 / 1 in the lottery), so the runs here let the rank of every interior bond climb by one per sweep from 1
to 36: every length r1 = 1 .. 35 occurs, that is every residue modulo 16 and the edges 15 / 16 / 17 and 31 / 32 / 33.  That the
oracle really runs 35 sweeps and ends at rank 36 is checked without a GPU, so a change in the drivers cannot silently empty the
coverage.  The helper itself -- each term once, in ascending order, no operand loaded that is not used, sums equal to the plain
loop's bit for bit -- is checked by a host program (tests/cluster_resid_main.cpp), once more under the sanitizers.

TTX_ARITH=fast shares the helper; it has no exact yardstick of its own and rests on the existing fast-arithmetic tests."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = "default"      # the driver's own accuracy
# (m, n, r, piv, bond groups), accuracy
CASES = [((10, 9, 36, 2, 1), DEFAULT), ((10, 9, 36, 2, 2), 0.0), ((12, 7, 36, 1, 1), 0.0), ((8, 17, 36, 2, 1), 0.0)]
IDS = [f"C{c[0]}_n{c[1]}_r{c[2]}_p{c[3]}_g{c[4]}" for c, _ in CASES]
SWEEPS, MAXRANK = 35, 36

_oracle_runs = {}


def _oracle(case, acc):
    """One oracle run per case, shared by the tests and left unchanged."""
    if (case, acc) not in _oracle_runs:
        m, n, r, piv, ng = case
        s = D.ising_setup("c", m, n)
        a = s["acc"] if acc == DEFAULT else acc
        _oracle_runs[(case, acc)] = (s, a, O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=a, quad=s["quad"], tru=s["tru"], nproc=ng))
    return _oracle_runs[(case, acc)]


@pytest.mark.parametrize("case,acc", CASES, ids=IDS)
def test_oracle_ranks_pass_through_every_length(case, acc):
    _, _, oo = _oracle(case, acc)
    assert len(oo["sweeps"]) - 1 == SWEEPS
    # the rank of a bond grows by at most one per sweep from 1: a bond that ends at 36 after 35 sweeps held every length 1 .. 35
    assert int(np.max(oo["r"])) == MAXRANK


def _identical(tt, oo):
    gs, os_ = tt.sweeps(), oo["sweeps"]
    assert len(gs) == len(os_) == SWEEPS + 1
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d]), "pivot tapes differ"
    for a, b in zip(gs, os_):
        assert a["neval"] == b["neval"] and a["erank"] == b["erank"], f"sweep {a['it']}"
        assert a["val"] == b["val"], f"sweep {a['it']}: val {a['val']!r} vs {b['val']!r}"
        assert a["amax"] == b["amax"] and a["pivotmax"] == b["pivotmax"], f"sweep {a['it']}"
    assert tt.neval == oo["neval"] and np.array_equal(tt.ranks(), oo["r"])
    for k in range(1, tt.d + 1):
        assert np.array_equal(tt.core(k), oo["cores"][k - 1]), f"core {k} differs"


def _run(case, acc):
    _, _, r, piv, ng = case
    s, a, oo = _oracle(case, acc)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=a, quad=s["quad"], tru=s["tru"], nproc=ng)
    assert tt.sweep_path() == "cluster" and tt.arith == "exact"
    tt.run()
    assert tt.sweep_path() == "cluster" and tt.cluster_fallbacks == 0
    _identical(tt, oo)
    assert tt.quad(s["quad"]) == oo["value"]
    return tt


@pytest.mark.gpu
@pytest.mark.parametrize("pad", ["0", "1"])
@pytest.mark.parametrize("case,acc", CASES[:2], ids=IDS[:2])
def test_cluster_residual_sums_bit_exact_both_evaluators(monkeypatch, case, acc, pad):
    monkeypatch.setenv("TTX_SWEEP", "cluster")
    monkeypatch.setenv("TTX_CL_PAD", pad)
    tt = _run(case, acc)
    assert tt.cluster_eval() == {"0": "predicated", "1": "chunks"}[pad]


@pytest.mark.gpu
@pytest.mark.parametrize("case,acc", CASES[2:], ids=IDS[2:])
def test_cluster_residual_sums_bit_exact(monkeypatch, case, acc):
    monkeypatch.setenv("TTX_SWEEP", "cluster")
    monkeypatch.delenv("TTX_CL_PAD", raising=False)
    _run(case, acc)


def _host(tmp_path, name, extra, env=None):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "ttcross_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cluster_resid_main.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad, nchk = (int(x) for x in out.stdout.strip().splitlines()[-1].split())
    assert bad == 0
    assert nchk == 2 * 71 * 3 + 200 * 71 * 2 * 3      # order, load count, term count per (n, batch); three sums per (data set, n, batch)


def test_ordered_sum_helper_on_the_host(tmp_path):
    _host(tmp_path, "cluster_resid", [])


def test_ordered_sum_helper_under_address_and_undefined_sanitizers(tmp_path):
    _host(tmp_path, "cluster_resid_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
          dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
