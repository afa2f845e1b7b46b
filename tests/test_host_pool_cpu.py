"""The worker threads of the host integrand (ttcross_amd/csrc/ttx_host_pool.h) as a stand-alone host program, built plain, under the
address and undefined-behaviour sanitizers and under the thread sanitizer (tests/host_pool_main.cpp; no GPU is touched).  Pools of
1, 2 and 5 threads run batches on both sides of the serial cut (31 and 32) and must visit every index exactly once, also with two
caller threads on one pool; the sizing rule of the process-wide pool (TTX_HOST_THREADS, then OMP_NUM_THREADS, then the hardware's
count up to 32) is held against literal lines."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LINES = [f"threads={nt} n={n}: 0 indices not visited exactly once" for nt in (1, 2, 5) for n in (0, 1, 31, 32, 33, 1000)] + [
    "threads=5 two callers, 50 batches of n=200 each: 0 indices not visited exactly once",
    "pools destroyed with idle workers",
    "TTX_HOST_THREADS=3 OMP_NUM_THREADS=unset hardware=8 -> 3 threads",
    "TTX_HOST_THREADS=unset OMP_NUM_THREADS=2 hardware=8 -> 2 threads",
    "TTX_HOST_THREADS=0 OMP_NUM_THREADS=7 hardware=8 -> 8 threads",      # a TTX_HOST_THREADS that is set decides alone: 0 is "the hardware's"
    "TTX_HOST_THREADS=unset OMP_NUM_THREADS=unset hardware=64 -> 32 threads",
    "TTX_HOST_THREADS=unset OMP_NUM_THREADS=unset hardware=1 -> 1 threads",
    "TTX_HOST_THREADS=unset OMP_NUM_THREADS=unset hardware=0 -> 1 threads",
    "host pool: ok",
]


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no host C++ compiler")
    return c


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], ["-fsanitize=thread"]],
                         ids=["plain", "sanitizers", "tsan"])
def test_host_pool(cxx, tmp_path, flags):
    exe = str(tmp_path / "host_pool_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "ttcross_amd", "csrc"), os.path.join(ROOT, "tests", "host_pool_main.cpp"), "-o", exe, "-pthread"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == LINES
