"""The rule part of ttx_bondstep.h (rook turn, pivot taking, acceptance, pivot range, traffic: what all sweep kernels
share) as a stand-alone host program, tests/bondstep_main.cpp:
  * rook sequence: piv 0..5, both directions, the arg-max repeating the pivot at every subset of the residual half-steps
    -- (type, residual, stop) and the pivot of every turn against the reference's loop shape (lib/dmrgg.f90:492-582)
    restated in the program; the GPU parity shapes do not reach the later stops of piv 4 and 5;
  * pivot taking at r0 = 1, n2 = 1, the last position and INT_MAX (every residual a NaN) -> (1, 1);
  * acceptance: equality and NaN refused, pivotmax_prev = -1 of a first sweep;
  * pivot range: first value, then max / min; traffic against the formula.
The same program runs once more under -fsanitize=address,undefined."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "ttcross_amd", "csrc"),
                    os.path.join(ROOT, "tests", "bondstep_main.cpp"), "-o", str(exe)], check=True)
    return exe


def _check(out):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad, nseq, nchk = (int(x) for x in out.stdout.strip().splitlines()[-1].split())
    assert bad == 0
    # 3 shapes x 2 directions x (1 + 4 + 16 + 64 + 256 + 1024) repeat patterns for piv = 0..5
    assert nseq == 3 * 2 * 1365
    assert nchk >= 3 * nseq + 30


def test_bondstep_rules(tmp_path):
    _check(subprocess.run([str(_build(tmp_path, "bondstep", []))], capture_output=True, text=True))


def test_bondstep_rules_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path, "bondstep_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    _check(subprocess.run([str(exe)], capture_output=True, text=True, env=env))
