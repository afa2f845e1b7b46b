"""The record of the dynamic-LDS ceilings (ttcross_amd/csrc/ttx_lds.h) as a stand-alone host program under the address and
undefined-behaviour sanitizers: a smaller request after a larger one makes no runtime call, two devices keep separate records, two
host threads may ask at once (tests/lds_registry_main.cpp; a stub stands in for the runtime call, no GPU is touched)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lds_registry_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lds_registry_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
                    "-I", os.path.join(ROOT, "ttcross_amd", "csrc"), os.path.join(ROOT, "tests", "lds_registry_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lds registry: ok" in r.stdout, r.stdout + r.stderr
