"""The node-local transport over POSIX shared memory (ttcross_amd/csrc/ttx_shm.h) as a stand-alone host program, built plain and under
the address and undefined-behaviour sanitizers (tests/shm_main.cpp; no GPU is touched).  The ranks are forked processes on segments
named after the program's pid: the ring exchange of the sweep (3 ranks, so that the middle one uses both of its boxes, and 2), the
all-reduce whose rank-order fold (1e16 + 1.0) + -1e16 must give exactly 0.0 on every rank, a segment that an earlier job left behind
with go set, and the three ways an attach fails, reached in a fraction of a second through ShmTransport::bound.  The messages are
the ones ttx_comm_init_shm hands to the caller, with the segment's name as NAME."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LINES = [
    "ring of 3 ranks, 5 rounds, messages of 0, 1, 64 and 17 of 64 bytes: ok",
    "close: the name is gone after the owner closed: ok",
    "ring of 2 ranks, 5 rounds, messages of 0, 1, 64 and 17 of 64 bytes: ok",
    "message of msz + 1 bytes: refused, nothing written: ok",
    "all-reduce of 3 ranks, sum, count 1: 1e16 + 1.0 + -1e16 is 0.0 on every rank: ok",
    "all-reduce of 3 ranks, sum, count redcap: 0.0 everywhere: ok",
    "all-reduce of 3 ranks, max: the maximum on every rank: ok",
    "all-reduce of redcap + 1: refused, the vector untouched: ok",
    "stale segment: a job of 2 ranks left without closing, the name is still there: ok",
    "stale segment: the next job under that name attached, exchanged a message and closed: ok",
    'rank 0 alone: TTX_EHIP "ttx_comm_init_shm: not all 2 ranks attached to NAME"',
    "rank 0 alone: the name is gone: ok",
    'rank 1 alone: TTX_EHIP "ttx_comm_init_shm: rank 0 did not create NAME (or never saw every rank)"',
    'rank 1 with another msz: TTX_EINVAL "ttx_comm_init_shm: the ranks disagree about the problem (or NAME belongs to another job)"',
    "rank 1 with another msz: rank 0 gave up and took the name away: ok",
    "shm: ok",
]


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no host C++ compiler")
    return c


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_shm(cxx, tmp_path, flags):
    exe = str(tmp_path / "shm_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "ttcross_amd", "csrc"), os.path.join(ROOT, "tests", "shm_main.cpp"), "-o", exe, "-pthread", "-lrt"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines() == LINES
