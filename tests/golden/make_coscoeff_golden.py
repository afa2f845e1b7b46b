#!/usr/bin/env python3
"""Regenerates the COS-coefficient fixtures from the GENUINE reference (test infrastructure; needs the reference sources and
the toolchain of `make -C oracle ref`, which must have run first).  The reference's constants, s_vectors, funcs and coefficients
modules are compiled next to oracle/_ref/obj and linked with our driver ref_coscoeff.f90; only program OUTPUT is stored:
    coscoeff_values.txt      "d ind(1..d) value" for 2000 multi-indices, d in {2, 4, 6, 10}, n = 65, the driver's parameters
    coscoeff_6_65_20_1.txt   dtt_dmrgg's per-sweep log on calc_coefficient at the driver's defaults (time column blanked)
"""
import os
import re
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF", "/root/reference")
R = os.path.join(ROOT, "oracle", "_ref")
FC = ["amdflang", "-O2", "-fopenmp", "-I/opt/conda/include", "-module-dir", os.path.join(R, "mod"), "-I" + os.path.join(R, "mod")]
LIBS = ["-L/opt/conda/lib", "-lmpifort", "-lmpi", "-lmkl_rt", "-Wl,-rpath,/opt/conda/lib", "-Wl,-rpath,/opt/rocm/lib/llvm/lib"]
RMODS = "zero nan trans default timef say rnd ptype ort lr mat quad tt dmrgg mvn_pdf".split()
CMODS = ["constants", "s_vectors", "funcs", "coefficients"]


def build():
    objs = [os.path.join(R, "obj", m + ".o") for m in RMODS]
    missing = [o for o in objs if not os.path.exists(o)]
    if missing:
        sys.exit("run `make -C oracle ref` first (missing %s)" % missing[0])
    for m in CMODS:
        o = os.path.join(R, "obj", m + ".o")
        subprocess.run(FC + ["-c", os.path.join(REF, "lib", m + ".f90"), "-o", o], check=True)
        objs.append(o)
    exe = os.path.join(R, "ref_coscoeff")
    subprocess.run(FC + [os.path.join(HERE, "ref_coscoeff.f90")] + objs + ["-o", exe] + LIBS, check=True)
    return exe


def main():
    exe = build()
    env = dict(os.environ, OMP_NUM_THREADS="1", MKL_THREADING_LAYER="SEQUENTIAL")
    rng = np.random.default_rng(20261016)
    lines = []
    for d, cnt in ((2, 500), (4, 500), (6, 500), (10, 500)):
        # half of the indices small (slowly varying, large values), half anywhere in 1..65
        ind = np.concatenate([rng.integers(1, 6, size=(cnt // 2, d)), rng.integers(1, 66, size=(cnt - cnt // 2, d))])
        inp = "%d %d\n" % (d, cnt) + "".join(" ".join(map(str, row)) + "\n" for row in ind)
        out = subprocess.run([exe, "values"], input=inp, capture_output=True, text=True, check=True, env=env).stdout.split()
        assert len(out) == cnt
        lines += ["%d %s %s" % (d, " ".join(map(str, row)), v) for row, v in zip(ind, out)]
    open(os.path.join(HERE, "coscoeff_values.txt"), "w").write("\n".join(lines) + "\n")
    log = subprocess.run([exe, "sweep", "6", "65", "20", "1"], capture_output=True, text=True, check=True, env=env).stdout
    keep = [re.sub(r"time: +[0-9.E+-]+", "time: -", l) for l in log.splitlines() if "n_evals" in l or l.startswith("...with")]
    open(os.path.join(HERE, "coscoeff_6_65_20_1.txt"), "w").write("\n".join(keep) + "\n")
    for f in os.listdir("."):
        if f.endswith(".mod"):
            os.remove(f)


if __name__ == "__main__":
    main()
