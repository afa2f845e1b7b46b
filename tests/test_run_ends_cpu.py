"""What decides the form of the two ends of a run, as a stand-alone host program (tests/run_ends_main.cpp): head_direct, fin_early,
fin_skip_exch and final_exchange() of ttcross_amd/csrc/ttx_loop_plan.h; the switches TTX_HEAD_DIRECT, TTX_INIT_WIDE, TTX_INIT_WAVE,
TTX_FIN_EARLY, TTX_FIN_SKIP_EXCH and TTX_QUAD_LDS, init_samples_plan() and quad_tree_lds() of ttx_create_plan.h.
loop_plan() runs over every combination of its inputs -- whole-sweep kernel none / fused / cluster, the nine booleans, W in {1, 2},
nproc in {1, 2, 3}, maxrank in {1, 2, 5} -- against the rules in plain words: the new switches move none of the old fields; the
summary goes straight to the pinned slot only in the single-process pipelined loop with a sweep to run; the finalisation runs early
only beside a forked quadrature; the final exchange stays for one process without a sweep, for several processes and with the
switch off, and never exists with one group.  Then the named configurations, the switches as create_env_from reads them, the
launch of k_init_samples (threads, LDS, form) over dimensions and sample counts, and the LDS of the quadrature's tree.
The same program runs once more under -fsanitize=address,undefined."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "ttcross_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "run_ends_main.cpp"), "-o", str(exe)], check=True)
    return exe


def _check(out):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad, ncomb = (int(x) for x in out.stdout.strip().splitlines()[-1].split())
    assert bad == 0
    assert ncomb > 3 * 2 ** 9 * 2 * 3 * 3       # kernels x booleans x W x nproc x maxrank, then the sample launches


def test_run_ends(tmp_path):
    _check(subprocess.run([str(_build(tmp_path, "run_ends", []))], capture_output=True, text=True))


def test_run_ends_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path, "run_ends_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    _check(subprocess.run([str(exe)], capture_output=True, text=True, env=env))
