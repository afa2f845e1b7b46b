"""The host side of the stretch between two sweeps as a stand-alone program, tests/sweep_gap_main.cpp: the rule that says which
workgroup of a cluster packs which part at the exit of a launch (cl_pack_block, ttcross_amd/csrc/ttx_cluster_rules.h) for every
cluster size 1 .. TTX_CLMAX -- each part exactly once, red[] with the right-going message on workgroup 0 -- and the parsing of
TTX_TAIL_EVENT, TTX_TAIL_LEAN and TTX_CL_PACK2 in create_plan.  Once more under -fsanitize=address,undefined."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ttcross_amd", "csrc")
# 16 cluster sizes x split off / on x (two parts once each + the two placements); 3 x 2 environments x 4; three words x 3 + the refusal's 2
NCHK = 16 * 2 * 4 + 3 * 2 * 4 + 3 * 3 + 2


@pytest.mark.parametrize("extra", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_pack_rule_and_switches(tmp_path, extra):
    exe = tmp_path / "sweep_gap"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", CSRC, os.path.join(ROOT, "tests", "sweep_gap_main.cpp"),
                    "-o", str(exe)], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert out.stdout.split() == ["0", str(NCHK)]
