"""The two value rules of the cluster sweep kernel that need no GPU (ttcross_amd/csrc/ttx_cluster_rules.h) as a stand-alone
host program, tests/cluster_diet_main.cpp:
  * the integer key under which the kernel takes wave maxima (high word as a signed int, then low word as an unsigned one)
    orders and equates exactly like < and == on doubles and gives back the double's bits: 0.0, the smallest denormal, pairs
    that differ only in the low / only in the high word, 1.0, DBL_MAX, +inf, the start value -1.0 and 10^6 random non-negative
    doubles, each against its neighbour, a special value, a value of the same high word and one of the same low word; the two
    integer maxima over 64 lanes give the bits of the plain maximum;
  * the slice bounds equal floor(c n / NB) for NB = 2..16, n = 1..200, c = 0..NB and tile [0, n) without gap or overlap.
The same program runs once more under -fsanitize=address,undefined."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "ttcross_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cluster_diet_main.cpp"), "-o", str(exe)], check=True)
    return exe


def _check(out):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad, ncmp, ntab, nchk = (int(x) for x in out.stdout.strip().splitlines()[-1].split())
    assert bad == 0
    assert ncmp == 14 * 14 + 4 * 10**6          # the special values pairwise, four partners per random value
    assert ntab == 15 * 200
    assert nchk >= 4 * ncmp + 10**6 // 64 + ntab * 3


def test_cluster_key_and_slices(tmp_path):
    _check(subprocess.run([str(_build(tmp_path, "cluster_diet", []))], capture_output=True, text=True))


def test_cluster_key_and_slices_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path, "cluster_diet_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    _check(subprocess.run([str(exe)], capture_output=True, text=True, env=env))
