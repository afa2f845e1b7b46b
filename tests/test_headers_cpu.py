"""Every header under ttcross_amd/csrc compiles on its own: a one-line file that includes only that header passes the compiler's
syntax check, for gfx950 with hipcc, or with g++ for the host-only headers that the stand-alone host programs (tests/*_main.cpp)
already build that way.  And nothing of the library proper depends on the test-only kernels of ttx_ktest.h."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "ttcross_amd", "csrc")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.h")))
HOST_ONLY = {"ttx_create_plan.h", "ttx_files.h", "ttx_host_pool.h", "ttx_lds.h", "ttx_loop_plan.h", "ttx_op_plan.h", "ttx_qr_plan.h",
             "ttx_shm.h"}
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(header, tmp_path):
    host = header in HOST_ONLY
    if not host and HIPCC is None:
        pytest.skip("no hipcc on this box")
    src = tmp_path / ("one.cpp" if host else "one.hip")
    src.write_text('#include "%s"\n' % header)
    cmd = (["g++", "-std=c++17", "-fsyntax-only"] if host else
           [HIPCC, "--offload-arch=gfx950", "-std=c++17", "--cuda-device-only", "-fsyntax-only"]) + ["-I", CSRC, str(src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_only_the_engine_includes_the_test_kernels():
    assert HOST_ONLY <= set(HEADERS) and "ttx_ktest.h" in HEADERS
    users = [f for f in sorted(os.listdir(CSRC))
             if re.search(r'#\s*include\s*"ttx_ktest\.h"', open(os.path.join(CSRC, f), errors="replace").read())]
    assert users == ["ttx_engine.hip"]
