"""The prologue of a bond step of the cluster sweep kernel (ttx_cluster.h) against the oracle, bit for bit: the staging of the
value tables XL / XR and of the neighbour LU factors GL / GU, the CDF segments fetched by the two idle waves, the generator step
taken from a lane exchange, and the paired lottery index (ttx_lottery_index2, checked on the host by test_lottery_pair_cpu.py).

The staging walks are the strided loops they were: a variant that requested a thread's share in batches of B = 2 (and 4) before
consuming it was measured and dropped (profiles/HISTORY.md).  The cases below were chosen for that variant and stay, because
they are the smallest at which a thread's share of a table -- floor(E / 256) or one more of its E entries -- takes the values
0, 1, 2, 3 and more than 4 for each of the four streams, i.e. every trip count of the walks that a short run can reach.  The
shares follow from the ranks, which follow from the oracle's pivot tapes (a rank grows by one where a pivot was accepted):

  * C_10, n = 9, r = 64: RM = 64 with short modes.  Ising C has no ranks up to 64 to give (the run ends at 46 with the accuracy
    target at zero), but the row strides and the LDS carve-up are those of RM = 64, and the factors reach 46 * 46 = 2116
    entries: shares of 0 .. 9 for GL / GU;
  * C_68, n = 9, r = 24: long rows (up to 72 staged dimensions) at ranks up to 17: table shares of 0 .. 5;
  * C_36, n = 9, r = 64 (two groups) and C_52, n = 9, r = 64 (one group): at these sizes the factors (C_36) and also the
    launch-long pivot lists (C_52) no longer fit the LDS budget next to the tables, so the kernel runs with cluster_ldsinv = 0
    and cluster_zkeep = 0 (checked below on the host with the engine's own plan);
  * C_17, n = 7, r = 8, piv 3, four groups: several groups at small ranks, bonds at either end of a group;
  * C_8, n = 65, r = 48 and C_5, n = 257, r = 8: 130 .. 224 and more than 512 lottery candidates per bond step, for the forms of
    the generator step (0 .. 3 modular products behind the lane exchange; the square-and-multiply loop from 512 candidates on).
Every case meets the first bond (no left rows) and the last (no right rows) and runs both sweep directions."""
import functools
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SB = GB = 2           # batch depth of the dropped variant: shares of 0, 1, B, B + 1 and more than 2 B must occur
CB = 256

# (m, n, r, piv, bond groups); the accuracy target is zero: the runs go on until no pivot is accepted any more
CASES = [(10, 9, 64, 1, 1), (68, 9, 24, 1, 2), (36, 9, 64, 2, 2), (52, 9, 64, 1, 1), (17, 7, 8, 3, 4), (8, 65, 48, 1, 1), (5, 257, 8, 2, 1)]
IDS = [f"C{c[0]}_n{c[1]}_r{c[2]}_p{c[3]}_g{c[4]}" for c in CASES]
EVAL = {"0": "predicated", "1": "chunks"}
# cluster_ldsinv, cluster_zkeep of the plan (ttx_create_plan.h) per case
PLAN = {IDS[0]: (1, 1), IDS[1]: (1, 1), IDS[2]: (0, 1), IDS[3]: (0, 0), IDS[4]: (1, 1), IDS[5]: (1, 1), IDS[6]: (1, 1)}


@functools.lru_cache(maxsize=None)
def _oracle(m, n, r, piv, ng):
    s = D.ising_setup("c", m, n)
    return O.dmrgg(s["n"], s["fun_id"], s["par"], r, piv=piv, accuracy=0.0, quad=s["quad"], tru=s["tru"], nproc=ng)


def _classes(entries):
    """Shares of a table of `entries` entries among CB threads."""
    return {entries // CB, -(-entries // CB)}


def _steps(m, oo):
    """(direction, p, candidates for r0, candidates for r2) of every bond step.  The rank of a neighbour bond is the one before
    the sweep, or one more if that bond was appended earlier in this sweep (which depends on the group it belongs to: both
    candidates are kept and a share counts as met only if both give it)."""
    d = m - 1
    rk = [1] * (d + 1)
    out = []
    for s, rec in enumerate(oo["sweeps"][1:]):
        tape = oo["tapes"][s]
        acc = [0] * (d + 2)
        for p in range(1, d):
            acc[p] = int(tape[p][0] != -1)
        for p in range(1, d):
            lo0 = [rk[p - 1]] if (rec["dir"] != 1 or p == 1) else [rk[p - 1], rk[p - 1] + acc[p - 1]]
            lo2 = [rk[p + 1]] if (rec["dir"] == 1 or p == d - 1) else [rk[p + 1], rk[p + 1] + acc[p + 1]]
            out.append((rec["dir"], p, lo0, lo2))
        for p in range(1, d):
            rk[p] += acc[p]
    assert rk == [int(x) for x in oo["r"]], "ranks rebuilt from the tapes"
    return out


def _met(m, oo):
    """Shares met per stream: tables left / right, factors left / right (the factors as if every bond had both neighbours in
    its group -- true for all inner bonds of a one-group case)."""
    d = m - 1
    VS = ((d + 7) & ~7) + 8
    met = {"XL": set(), "XR": set(), "GL": set(), "GU": set()}
    for _, p, c0, c2 in _steps(m, oo):
        AL, AR = min(VS, (p - 1 + 7) & ~7), min(VS, (d - p - 1 + 7) & ~7)
        met["XL"] |= set.intersection(*[_classes(r0 * AL) for r0 in c0])
        met["XR"] |= set.intersection(*[_classes(r2 * AR) for r2 in c2])
        if p > 1:
            met["GL"] |= set.intersection(*[_classes(r0 * r0) for r0 in c0])
        if p < d - 1:
            met["GU"] |= set.intersection(*[_classes(r2 * r2) for r2 in c2])
    return met


def test_cases_cover_every_form_of_the_generator_step():
    """48271^(2 nlot) is one lane exchange and nlot >> 6 modular products below 512 candidates, the square-and-multiply loop from
    there on: nlot = r0 + n1 + n2 + r2 must meet 0, 1, 2, 3 products and the loop."""
    met = set()
    for c in CASES:
        for _, p, c0, c2 in _steps(c[0], _oracle(*c)):
            met |= set.intersection(*[{(r0 + 2 * c[1] + r2) >> 6} for r0 in c0 for r2 in c2])
    assert {0, 1, 2, 3} <= met and max(met) >= 8, sorted(met)


def test_cases_cover_every_share_of_the_staging_walks():
    met = {k: set() for k in ("XL", "XR", "GL", "GU")}
    dirs, maxrank = set(), 0
    for cid, c in zip(IDS, CASES):
        oo = _oracle(*c)
        assert len(oo["sweeps"]) >= 3
        dirs |= {rec["dir"] for rec in oo["sweeps"][1:]}
        maxrank = max(maxrank, int(max(oo["r"])))
        for k, v in _met(c[0], oo).items():
            # the factors are staged with cluster_ldsinv only; where their group ends is known here for one group
            if k in ("XL", "XR") or (PLAN[cid][0] and c[4] == 1):
                met[k] |= v
    for stream, B in (("XL", SB), ("XR", SB), ("GL", GB), ("GU", GB)):
        assert {0, 1, B, B + 1} <= met[stream], (stream, sorted(met[stream]))
        assert max(met[stream]) > 2 * B, (stream, sorted(met[stream]))
    assert dirs == {1, 2}
    assert any(c[2] == 64 and c[1] <= 9 for c in CASES) and maxrank > 40
    assert {c[4] for c in CASES} >= {1, 2, 4}            # one group (its ends have no GL / no GU) and several
    # the first bond has no left rows, the last no right rows: every case has both (p = 1 and p = d - 1 are always walked)


def test_plan_switches_of_the_cases(tmp_path):
    """cluster_ldsinv and cluster_zkeep as the engine's plan decides them for the cases (host code only)."""
    src = tmp_path / "plan.cpp"
    src.write_text(r'''
#include "ttx_create_plan.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
int main(int argc, char **argv)
{
    for (int a = 1; a + 4 < argc; a += 5) {
        const int d = atoi(argv[a]), n = atoi(argv[a + 1]), r = atoi(argv[a + 2]), piv = atoi(argv[a + 3]), nproc = atoi(argv[a + 4]);
        std::vector<int32_t> nn(d, n);
        std::vector<double> par(2 * n + 1, 1.0 / n);
        for (int j = 0; j < n; j++) par[j] = (j + 0.5) / n;
        par[2 * n] = 1;
        ttx_config cfg{};
        cfg.d = d; cfg.n = nn.data(); cfg.fun_id = TTX_FUN_ISING; cfg.par = par.data(); cfg.npar = (int32_t)par.size();
        cfg.accuracy = 0.0; cfg.maxrank = r; cfg.pivoting = piv; cfg.nproc = nproc; cfg.world_size = 1; cfg.arith = TTX_ARITH_EXACT;
        const CreateEnv env = create_env_from([&](const char *name) -> const char * { return strcmp(name, "TTX_SWEEP") ? nullptr : "cluster"; });
        DevCaps caps; caps.ncu = 256; caps.coop = true;
        CreatePlan p = create_plan(cfg, false, env, caps);
        if (!p.err) create_admit(p, 8);
        printf("%d %d %d %d\n", p.err, p.cluster >= 2, p.cluster_ldsinv, p.cluster_zkeep);
    }
}
''')
    exe = tmp_path / "plan"
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "ttcross_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    args = [str(x) for c in CASES for x in (c[0] - 1, c[1], c[2], c[3], c[4])]
    out = subprocess.run([str(exe)] + args, capture_output=True, text=True, check=True).stdout.split("\n")
    for cid, line in zip(IDS, out):
        err, cluster, ldsinv, zkeep = (int(x) for x in line.split())
        assert err == 0 and cluster == 1, cid
        assert (ldsinv, zkeep) == PLAN[cid], cid
    assert {0, 1} == {v[0] for v in PLAN.values()} == {v[1] for v in PLAN.values()}


def _identical(tt, oo):
    gs, os_ = tt.sweeps(), oo["sweeps"]
    assert len(gs) == len(os_) and len(gs) >= 3, "two sweeps (one per direction) behind the initial one"
    assert np.array_equal(tt.tapes()[:, 1:tt.d], oo["tapes"][:, 1:tt.d]), "pivot tapes differ"
    for a, b in zip(gs, os_):
        assert a["neval"] == b["neval"] and a["erank"] == b["erank"], f"sweep {a['it']}"
        assert a["val"] == b["val"], f"sweep {a['it']}: val {a['val']!r} vs {b['val']!r}"
        assert a["amax"] == b["amax"] and a["pivotmax"] == b["pivotmax"], f"sweep {a['it']}"
    assert tt.neval == oo["neval"] and np.array_equal(tt.ranks(), oo["r"])
    for k in range(1, tt.d + 1):
        assert np.array_equal(tt.core(k), oo["cores"][k - 1]), f"core {k} differs"


@pytest.mark.gpu
@pytest.mark.parametrize("pad", ["0", "1"])
@pytest.mark.parametrize("m,n,r,piv,ng", CASES, ids=IDS)
def test_cluster_prologue_bit_exact(monkeypatch, m, n, r, piv, ng, pad):
    monkeypatch.setenv("TTX_SWEEP", "cluster")
    monkeypatch.setenv("TTX_CL_PAD", pad)
    s = D.ising_setup("c", m, n)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=0.0, quad=s["quad"], tru=s["tru"], nproc=ng)
    assert tt.sweep_path() == "cluster" and tt.arith == "exact" and tt.cluster_eval() == EVAL[pad]
    tt.run()
    assert tt.cluster_fallbacks == 0
    oo = _oracle(m, n, r, piv, ng)
    _identical(tt, oo)
    assert tt.quad(s["quad"]) == oo["value"]
