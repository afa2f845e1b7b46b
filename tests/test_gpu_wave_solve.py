"""The append's two triangular wave solves (ttx_wave_solve.h: roles C and D of every sweep kernel) against the oracle, bit for bit.

Ising C with accuracy 0.0 and a rank limit of 64, so the sweeps run until no bond grows any more: the interior ranks climb by one
per sweep from 1 to about 45.  Every solve length from 1 upwards occurs, the change of packing at 32 / 33 (two solves of 32 lanes
in a wave up to rank 32, one of 64 above) and bonds whose two neighbours are packed differently (ranks 9 and 42).  With n = 9 over
the eight workgroups of a cluster a slice holds one or two solves, so the half-empty wave occurs; the run with two bond groups
takes the boundary blocks between the sweeps through the same solves.  That the oracle's runs really reach these ranks is checked
without a GPU, so a change in the drivers cannot silently empty the coverage.  The helper itself -- results equal to the plain
substitution, every LU index inside the packed block, every entry used once -- is checked by a host program
(tests/wave_solve_main.cpp), once more under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (m, n, r, piv, bond groups), all with accuracy 0.0
CASES = [(10, 9, 64, 2, 1), (10, 9, 64, 2, 2), (8, 17, 64, 2, 1)]
IDS = [f"C{c[0]}_n{c[1]}_r{c[2]}_p{c[3]}_g{c[4]}" for c in CASES]

_oracle_runs = {}


def _oracle(case):
    """One oracle run per case, shared by the tests and left unchanged."""
    if case not in _oracle_runs:
        m, n, r, piv, ng = case
        s = D.ising_setup("c", m, n)
        _oracle_runs[case] = (s, O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=0.0, quad=s["quad"], tru=s["tru"], nproc=ng))
    return _oracle_runs[case]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_oracle_ranks_cross_the_packing_change(case):
    _, oo = _oracle(case)
    r = np.asarray(oo["r"]).ravel()
    r = r[r > 0]
    assert int(r.max()) >= 40
    # a bond whose solves take the LU of a neighbour of the other packing: one side at most 32, the other above
    assert any(min(a, b) <= 32 < max(a, b) for a, b in zip(r[:-2], r[2:]))


def _identical(tt, oo):
    gs, os_ = tt.sweeps(), oo["sweeps"]
    assert len(gs) == len(os_)
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d]), "pivot tapes differ"
    for a, b in zip(gs, os_):
        assert a["neval"] == b["neval"] and a["erank"] == b["erank"], f"sweep {a['it']}"
        assert a["val"] == b["val"], f"sweep {a['it']}: val {a['val']!r} vs {b['val']!r}"
        assert a["amax"] == b["amax"] and a["pivotmax"] == b["pivotmax"], f"sweep {a['it']}"
    assert tt.neval == oo["neval"] and np.array_equal(tt.ranks(), oo["r"])
    for k in range(1, tt.d + 1):
        assert np.array_equal(tt.core(k), oo["cores"][k - 1]), f"core {k} differs"


def _run(case, path):
    _, _, r, piv, ng = case
    s, oo = _oracle(case)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=0.0, quad=s["quad"], tru=s["tru"], nproc=ng)
    assert tt.sweep_path() == path and tt.arith == "exact"
    tt.run()
    assert tt.sweep_path() == path
    if path == "cluster":
        assert tt.cluster_fallbacks == 0
    _identical(tt, oo)
    assert tt.quad(s["quad"]) == oo["value"]
    return tt


@pytest.mark.gpu
@pytest.mark.parametrize("pad", ["0", "1"])
def test_wave_solves_bit_exact_cluster_both_evaluators(monkeypatch, pad):
    monkeypatch.setenv("TTX_SWEEP", "cluster")
    monkeypatch.setenv("TTX_CL_PAD", pad)
    tt = _run(CASES[0], "cluster")
    assert tt.cluster_eval() == {"0": "predicated", "1": "chunks"}[pad]


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["chain", "fused"])
def test_wave_solves_bit_exact_chain_and_fused(monkeypatch, path):
    monkeypatch.setenv("TTX_SWEEP", path)
    monkeypatch.delenv("TTX_CL_PAD", raising=False)
    _run(CASES[0], path)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES[1:], ids=IDS[1:])
def test_wave_solves_bit_exact_cluster(monkeypatch, case):
    monkeypatch.setenv("TTX_SWEEP", "cluster")
    monkeypatch.delenv("TTX_CL_PAD", raising=False)
    _run(case, "cluster")


def _host(tmp_path, name, extra, env=None):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "ttcross_amd", "csrc"),
                    os.path.join(ROOT, "tests", "wave_solve_main.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad, nchk = (int(x) for x in out.stdout.strip().splitlines()[-1].split())
    assert bad == 0
    assert nchk == 4 * (64 + 3 * 32) * 6      # data sets x (ranks 1..64 alone + ranks 1..32 with three second solves) x (bits, uses, bounds) x (L, U)


def test_wave_solve_helper_on_the_host(tmp_path):
    _host(tmp_path, "wave_solve", [])


def test_wave_solve_helper_under_address_and_undefined_sanitizers(tmp_path):
    _host(tmp_path, "wave_solve_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
          dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
