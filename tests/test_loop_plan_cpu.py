"""The form of the sweep loop (ttcross_amd/csrc/ttx_loop_plan.h) as a stand-alone host program (tests/loop_plan_main.cpp):
loop_plan() over every combination of its inputs -- whole-sweep kernel none / fused / cluster, the six booleans (profile,
TTX_PIPELINE off, quadrature, host-pass integrand, the two tail switches), W in {1, 2}, nproc in {1, 2, 3}, maxrank in {1, 2, 5} --
against a plain restatement of the expressions the driver had before the plan (`head` against its new rule: it implies `pipe`);
the implications side -> tail -> pipe, forkq -> pipe, head -> pipe, profile mode -> all false; and the named configurations (the
bench default, one group, fused, two processes, TTX_PIPELINE=0 with one process).
The same program runs once more under -fsanitize=address,undefined."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "ttcross_amd", "csrc"),
                    os.path.join(ROOT, "tests", "loop_plan_main.cpp"), "-o", str(exe)], check=True)
    return exe


def _check(out):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad, ncomb = (int(x) for x in out.stdout.strip().splitlines()[-1].split())
    assert bad == 0
    assert ncomb == 3 * 2 ** 6 * 2 * 3 * 3      # kernels x booleans x W x nproc x maxrank


def test_loop_plan(tmp_path):
    _check(subprocess.run([str(_build(tmp_path, "loop_plan", []))], capture_output=True, text=True))


def test_loop_plan_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path, "loop_plan_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    _check(subprocess.run([str(exe)], capture_output=True, text=True, env=env))
