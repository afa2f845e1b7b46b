"""The rules by which the cluster sweep kernel carries state from launch to launch (ttcross_amd/csrc/ttx_cluster_rules.h) as a
stand-alone host program, tests/cluster_entry_main.cpp: the compile-time table of generator powers against ttx_minstd_pow, the
generator step made from it and the carried word against ttx_minstd_pow(2 rngpos + 1) over sequences of bond steps below 64, from
64 and from 512 candidates, and the validity rules of the carried word and of the carried pivot lists.  Once more under
-fsanitize=address,undefined.  The switches TTX_CL_POWTAB, TTX_CL_WORD and TTX_CL_LISTS in create_plan: on by default, each
turned off by =0 alone, the lists only where the kernel keeps them in LDS at all."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ttcross_amd", "csrc")


def _build(tmp_path, name, src, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", CSRC, str(src), "-o", str(exe)], check=True)
    return exe


def _check(out):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad, nchk = (int(x) for x in out.stdout.strip().splitlines()[-1].split())
    assert bad == 0
    # table 256 + entry 64; 3000 + 25 exponents of the constexpr rule; 1201 steps; four checks per bond step of the four sequences;
    # five cases of the word's rule; 40 x 42 + 1 of the lists' rule
    assert nchk == 257 + 3025 + 1201 + 4 * (8 * 200 + 10 * 100 + 6 * 100 + 9 * 100) + 5 + 40 * 42 + 1


def test_carried_state_rules_on_the_host(tmp_path):
    exe = _build(tmp_path, "cluster_entry", os.path.join(ROOT, "tests", "cluster_entry_main.cpp"), [])
    _check(subprocess.run([str(exe)], capture_output=True, text=True))


def test_carried_state_rules_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path, "cluster_entry_san", os.path.join(ROOT, "tests", "cluster_entry_main.cpp"), ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    _check(subprocess.run([str(exe)], capture_output=True, text=True, env=env))


def test_switches_reach_the_plan(tmp_path):
    exe = _build(tmp_path, "entry_plan", os.path.join(ROOT, "tests", "cluster_entry_plan_main.cpp"), [])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout[-2000:] + out.stderr[-2000:]
