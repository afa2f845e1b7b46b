"""The host side of the file formats (ttcross_amd/csrc/ttx_files.h) as a stand-alone host program, built plain and under the address
and undefined-behaviour sanitizers (tests/files_main.cpp; no GPU is touched): the stream file the genuine reference wrote
(tests/golden/ttio_5.tt) read, summed and written back; files the reader must refuse, each with the message dtt_read gives; the
verdicts of devfun_image_plausible on a table of images, which follow from the rules in its comments; a code-object file into
memory; the HDF5 round trip where libhdf5 is found.

The verdicts are those of the function as it stood in ttx_engine.hip (compiled on its own against the same table: no line
differs).  One case was added for a defect the move brought out: a header that promises cores of 8 TB made the reader ask for
that much memory before reading, and the failed allocation ended the process; it is refused as a short file now."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

REFUSALS = [
    'cut at 0 bytes: TTX_EINVAL "dtt_read: error reading header: FILE"',
    'cut at 127 bytes: TTX_EINVAL "dtt_read: error reading header: FILE"',
    'cut at 128 bytes: TTX_EINVAL "dtt_read: error reading lm: FILE"',
    'cut at 135 bytes: TTX_EINVAL "dtt_read: error reading lm: FILE"',
    'cut at 136 bytes: TTX_EINVAL "dtt_read: error reading nr: FILE"',
    'cut at 140 bytes: TTX_EINVAL "dtt_read: error reading nr: FILE"',
    'cut at 716 bytes: TTX_EINVAL "dtt_read: error reading cores: FILE"',
    'txt = XX: TTX_EINVAL "dtt_read: not TT header in file: FILE"',
    'ver(1) = 2: TTX_EINVAL "dtt_read: not correct version of TT file: FILE"',
    'l = 0: TTX_EINVAL "dtt_read: read strange l,m: FILE"',
    'm < l: TTX_EINVAL "dtt_read: read strange l,m: FILE"',
    'm = 2049: TTX_EINVAL "dtt_read: read strange l,m: FILE"',
    'n(1) = 0: TTX_EINVAL "dtt_read: tt structure has invalid size: FILE"',
    'n(1) = 32001: TTX_EINVAL "dtt_read: tt structure has invalid size: FILE"',
    'r(0) = 0: TTX_EINVAL "dtt_read: tt structure has invalid size: FILE"',
    'r(1) = 129: TTX_EINVAL "dtt_read: tt structure has invalid size: FILE"',
    '2048 cores of 128 x 32000 x 128 promised, none there: TTX_EINVAL "dtt_read: error reading cores: FILE"',
]
IMAGES = [
    "ELF, 63 bytes: false",
    "ELF, 64 bytes, class 1: false",
    "ELF, 64 bytes, both tables empty at 64: true",
    "ELF, phoff = nbytes + 1: false",
    "ELF, 2 program headers of 56 bytes up to the end: true",
    "ELF, 2 program headers of 56 bytes one byte past the end: false",
    "ELF, shoff = nbytes + 1: false",
    "ELF, 3 section headers of 64 bytes up to the end: true",
    "ELF, 3 section headers of 64 bytes one byte past the end: false",
    "ELF, 65535 section headers of 65535 bytes: false",
    "bundle, 0 entries: false",
    "bundle, 1025 entries: false",
    "bundle, one entry cut at 23 of its 24 bytes: false",
    "bundle, one complete entry: true",
    "bundle, entry offset + size one past the end: false",
    "bundle, entry offset past the end: false",
    "bundle, id length 2^64 - 1: false",
    "bundle, id one byte past the end: false",
    "CCOB, 23 bytes: false",
    "CCOB, 24 bytes: true",
    "3 bytes: false",
    "no bytes: false",
]
CODE_OBJECT_FILES = [
    'missing file: 1 "who: cannot read FILE: No such file or directory"',
    'empty file: 1 "who: FILE is empty"',
    'no path: 1 "who: path missing"',
    "70000 bytes in two chunks: read back equal",
]


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no host C++ compiler")
    return c


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_files(cxx, tmp_path, flags):
    exe = str(tmp_path / "files_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "ttcross_amd", "csrc"), os.path.join(ROOT, "tests", "files_main.cpp"), "-o", exe, "-ldl"], check=True)
    r = subprocess.run([exe, GOLDEN, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    # what the genuine reference's dtt_read printed for the same file
    reference = [ln for ln in open(os.path.join(GOLDEN, "ttio_5.txt")).read().splitlines() if ln.split()[0] in ("lm", "n", "r", "checksum")]
    assert len(reference) == 4
    assert lines[:4] == reference
    assert lines[4] == "written back: the bytes of the fixture"
    assert lines[5:-2] == REFUSALS + IMAGES + CODE_OBJECT_FILES
    assert lines[-2] in ("hdf5: round trip ok", "hdf5: not available")
    assert lines[-1] == "files: ok"
