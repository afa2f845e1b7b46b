"""The two rules of ttx_bondstep.h behind the end of a sweep, as a stand-alone host program (tests/sweep_tail_main.cpp):
  * stop_rule -- the one function k_sweep_end and the host loop decide with -- against a plain restatement of lib/dmrgg.f90:1011-1019
    over generated runs: every pattern of up to six sweeps of {pivot above the bound, at or below it, NaN pmax, NaN amax}, repeated,
    with the rule off (accuracy < 0), accuracy 0 and two positive ones, rank limits that end the run before, at and after the third
    strike; strike resets, the sweep it + 1 == maxrank and both NaN kinds are asserted on their own as well;
  * boundary_neval -- what the apply block of k_exch_tail adds to a group's evaluation count -- against the conditions of
    k_exch_boundary's corner blocks over all combinations of neighbour present / its flag / the own boundary bond's flag.
The same program runs once more under -fsanitize=address,undefined."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "ttcross_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sweep_tail_main.cpp"), "-o", str(exe)], check=True)
    return exe


def _check(out):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad, nrun, nsweep, nbnd = (int(x) for x in out.stdout.strip().splitlines()[-1].split())
    assert bad == 0
    assert nrun == (4 + 16 + 64 + 256 + 1024 + 4096) * 4 * 5      # patterns x accuracies x rank limits
    assert nsweep >= 3 * nrun // 2                                 # a run is at least one sweep, most are several
    assert nbnd == 64 * (1 + 2 + 3 * 3)                            # flag combinations x the mode sizes that fit NM = 1, 2, 9


def test_sweep_tail_rules(tmp_path):
    _check(subprocess.run([str(_build(tmp_path, "sweep_tail", []))], capture_output=True, text=True))


def test_sweep_tail_rules_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path, "sweep_tail_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    _check(subprocess.run([str(exe)], capture_output=True, text=True, env=env))
