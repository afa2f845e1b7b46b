"""The QR plan of the tt_lib utilities (ttcross_amd/csrc/ttx_qr_plan.h) as a stand-alone host program, built plain and under the
address and undefined-behaviour sanitizers (tests/qr_plan_main.cpp; no GPU is touched).  The program prints the whole plan of a
list of shapes, held here against literal lines, and checks every plan of a grid of shapes (1 <= n <= 128, fourteen row counts,
seven settings of the switches) against the work buffers and the device's LDS.

PARENT: recorded from the launch ladders this plan replaced (qr_own_shape / qr_own_launch / qr_tsqr / qr of ttx_engine.hip, compiled
on their own with the launches replaced by a recorder that printed kernel, grid, threads, LDS bytes and buffer offsets).  The plan
gave the same line as those ladders for all 25088 plans of the grid but 21: tall-skinny levels of 93..96 columns whose stacked
triangles would have run past the work buffer (1632 x 93..96 and 6528 x 96) -- BOUNDED holds the plan of one of them now."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARENT = [
    "1632x32 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> tsqr_reg | L0 own<4,2> rows=1632 P=7 rbs=234 thr=1024 lds=60176 M=A+0 Q=Wb+0 R=Wc+0 | top own<4,2> rows=224 thr=1024 lds=57616 M=Wc+0",
    "276x64 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> tsqr_reg | L0 own<4,4> rows=276 P=2 rbs=138 thr=1024 lds=71184 M=A+0 Q=Wb+0 R=Wc+0 | top own<2,4> rows=128 thr=1024 lds=66064 M=Wc+0",
    "10x2 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<2,1> rows=10 thr=1024 lds=192 M=A+0",
    "408x97 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> qr_stream | top qr<false> rows=408 thr=1024 lds=4072 M=A+0",
    "5x1 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<2,1> rows=5 thr=1024 lds=56 M=A+0",
    "5x1 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<2,1> rows=5 thr=1024 lds=56 M=A+0",
    "10x2 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<2,1> rows=10 thr=1024 lds=192 M=A+0",
    "9x2 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<2,1> rows=9 thr=1024 lds=176 M=A+0",
    "72x15 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<2,1> rows=72 thr=1024 lds=8768 M=A+0",
    "61x15 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<2,1> rows=61 thr=1024 lds=7448 M=A+0",
    "84x16 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<2,1> rows=84 thr=1024 lds=10896 M=A+0",
    "65x16 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<2,1> rows=65 thr=1024 lds=8464 M=A+0",
    "84x17 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<2,2> rows=84 thr=1024 lds=11568 M=A+0",
    "69x17 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<2,2> rows=69 thr=1024 lds=9528 M=A+0",
    "144x31 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<4,2> rows=144 thr=1024 lds=35968 M=A+0",
    "125x31 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<2,2> rows=125 thr=1024 lds=31256 M=A+0",
    "144x33 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<4,4> rows=144 thr=1024 lds=38288 M=A+0",
    "133x33 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<4,4> rows=133 thr=1024 lds=35384 M=A+0",
    "264x63 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> tsqr_reg | L0 own<4,4> rows=264 P=2 rbs=132 thr=1024 lds=67040 M=A+0 Q=Wb+0 R=Wc+0 | top own<2,4> rows=126 thr=1024 lds=64016 M=Wc+0",
    "253x63 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> one_reg | top own<4,4> rows=253 thr=1024 lds=128024 M=A+0",
    "276x64 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> tsqr_reg | L0 own<4,4> rows=276 P=2 rbs=138 thr=1024 lds=71184 M=A+0 Q=Wb+0 R=Wc+0 | top own<2,4> rows=128 thr=1024 lds=66064 M=Wc+0",
    "257x64 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> tsqr_reg | L0 own<4,4> rows=257 P=2 rbs=129 thr=1024 lds=66576 M=A+0 Q=Wb+0 R=Wc+0 | top own<2,4> rows=128 thr=1024 lds=66064 M=Wc+0",
    "276x65 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> tsqr_reg | L0 own<4,8> rows=276 P=2 rbs=138 thr=1024 lds=72288 M=A+0 Q=Wb+0 R=Wc+0 | top own<4,8> rows=130 thr=1024 lds=68128 M=Wc+0",
    "261x65 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> tsqr_reg | L0 own<4,8> rows=261 P=2 rbs=131 thr=1024 lds=68648 M=A+0 Q=Wb+0 R=Wc+0 | top own<4,8> rows=130 thr=1024 lds=68128 M=Wc+0",
    "396x96 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> tsqr_reg | L0 own<4,8> rows=396 P=2 rbs=198 thr=1024 lds=152848 M=A+0 Q=Wb+0 R=Wc+0 | top own<4,8> rows=192 thr=1024 lds=148240 M=Wc+0",
    "385x96 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> tsqr_reg | L0 own<4,8> rows=385 P=2 rbs=193 thr=1024 lds=149008 M=A+0 Q=Wb+0 R=Wc+0 | top own<4,8> rows=192 thr=1024 lds=148240 M=Wc+0",
    "408x97 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> qr_stream | top qr<false> rows=408 thr=1024 lds=4072 M=A+0",
    "389x97 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> qr_stream | top qr<false> rows=389 thr=1024 lds=3920 M=A+0",
    "528x127 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> qr_stream | top qr<false> rows=528 thr=1024 lds=5272 M=A+0",
    "509x127 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> qr_stream | top qr<false> rows=509 thr=1024 lds=5120 M=A+0",
    "528x128 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> qr_stream | top qr<false> rows=528 thr=1024 lds=5280 M=A+0",
    "513x128 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> qr_stream | top qr<false> rows=513 thr=1024 lds=5160 M=A+0",
    "1632x32 wa=1 own=0 tsqr=1 thr=1024 top=1024 panel=0 -> tsqr_lds | L0 panel rows=1632 P=3 rbs=544 thr=1024 lds=144128 M=A+0 Q=Wb+0 R=Wc+0 | top qr<true> rows=96 thr=1024 lds=25888 M=Wc+0",
    "1632x32 wa=1 own=1 tsqr=1 thr=512 top=1024 panel=64 -> tsqr_reg | L0 own<2,4> rows=1632 P=26 rbs=63 thr=512 lds=16400 M=A+0 Q=Wb+0 R=Wc+0 | L1 own<2,4> rows=832 P=13 rbs=64 thr=512 lds=16656 M=Wc+0 Q=Wd+0 R=Wc+26624 | L2 own<2,4> rows=416 P=7 rbs=60 thr=512 lds=15632 M=Wc+26624 Q=Wd+26624 R=Wc+39936 | top own<4,4> rows=224 thr=512 lds=57616 M=Wc+39936",
    "1632x32 wa=1 own=1 tsqr=0 thr=1024 top=1024 panel=0 -> qr_stream | top qr<false> rows=1632 thr=1024 lds=13344 M=A+0",
    "3000x40 wa=1 own=0 tsqr=0 thr=1024 top=1024 panel=0 -> qr_stream | top qr<false> rows=3000 thr=1024 lds=24352 M=A+0",
    "1632x32 wa=0 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> qr_stream | top qr<false> rows=1632 thr=1024 lds=13344 M=A+0",
    "20000x8 wa=1 own=1 tsqr=0 thr=1024 top=1024 panel=0 -> refused",
]
BOUNDED = [
    "1632x96 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> qr_stream | top qr<false> rows=1632 thr=1024 lds=13856 M=A+0",
    "4896x96 wa=1 own=1 tsqr=1 thr=1024 top=1024 panel=0 -> tsqr_reg | L0 own<4,8> rows=4896 P=25 rbs=196 thr=1024 lds=151312 M=A+0 Q=Wb+0 R=Wc+0 | L1 own<4,8> rows=2400 P=13 rbs=185 thr=1024 lds=142864 M=Wc+0 Q=Wd+0 R=Wc+230400 | L2 own<4,8> rows=1248 P=7 rbs=179 thr=1024 lds=138256 M=Wc+230400 Q=Wd+230400 R=Wc+350208 | L3 own<4,8> rows=672 P=4 rbs=168 thr=1024 lds=129808 M=Wc+350208 Q=Wd+350208 R=Wc+414720 | L4 own<4,8> rows=384 P=2 rbs=192 thr=1024 lds=148240 M=Wc+414720 Q=Wd+414720 R=Wc+451584 | top own<4,8> rows=192 thr=1024 lds=148240 M=Wc+451584",
]


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if c is None:
        pytest.skip("no host C++ compiler")
    return c


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_qr_plan(cxx, tmp_path, flags):
    exe = str(tmp_path / "qr_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror"] + flags +
                   ["-I", os.path.join(ROOT, "ttcross_amd", "csrc"), os.path.join(ROOT, "tests", "qr_plan_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[:-1] == PARENT + BOUNDED
    assert lines[-1] == "qr plan: ok (1792 shapes)"          # 128 column counts x 14 row counts, none left out
