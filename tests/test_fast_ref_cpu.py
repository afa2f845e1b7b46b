"""tests/fast_ref.py, the reference of tests/test_gpu_fast_elements.py, checked without a GPU: it agrees with the oracle's exact-order
fp64 evaluation on every input of the GPU tests, its table references reproduce hand-computed cut counts, and on every compared
element the derived bound is at most 1e-10 |ref| (so a lost, doubled or misplaced range factor with an argument above 1e-9 cannot
hide) while |ref| >= 1e-250 (nothing near underflow, nothing left out).  Values the definition makes exactly 0 (a node equal to 1)
are compared absolutely and are the only exception to the second condition."""
import numpy as np
import pytest

import fast_ref as R
import oracle_lib as O

ISING = R.ising_cases()
MVN = R.mvn_cases()
ROUTES = ("lottery", "col", "row")


def _indices(c):
    return R.block_indices(c) + [tuple(ix) for ix in c["points"]]


@pytest.mark.parametrize("c", ISING, ids=[c["name"] for c in ISING])
def test_ising_reference_vs_oracle_and_conditions(c):
    d, n, p = c["d"], c["n"], c["p"]
    ind = _indices(c)
    nblk = len(ind) - len(c["points"])
    orc = O.fun(1, [n] * d, c["par"], np.array(ind, dtype=np.int32))
    nzero = 0
    for t, ix in enumerate(ind):
        det = R.ising_de_detail(c["par"], n, ix)
        ref = float(det["value"])
        with R.mp.workdps(R.DPS):
            assert abs(R.mp.mpf(float(orc[t])) - det["value"]) <= det["oracle_rel"] * abs(det["value"]), (c["name"], ix, orc[t], ref)
        if det["value"] == 0:
            assert c.get("zeros") and orc[t] == 0.0
            nzero += 1
            continue
        assert abs(ref) >= 1e-250, (c["name"], ix, ref)
        for mode in ("scratch", "chain"):
            for route in (ROUTES if t < nblk else ("point",)):
                assert R.ising_elem_bound(det, p - 1, d - p - 1, mode, route) <= 1e-10, (c["name"], ix, mode, route)
    assert (nzero > 0) == bool(c.get("zeros"))


@pytest.mark.parametrize("c", [c for c in ISING if "counts" in c], ids=[c["name"] for c in ISING if "counts" in c])
def test_cut_counts_by_hand(c):
    """near entries above 2^-54, t = 0 included: 2^-27 * 2^-27 = 2^-54 is dropped, 2^-53 is kept (pow2_*); c - 1 nodes 1/2 then 2^-40
    give c (reglimit_*); 0.6^67 > 2^-54 gives 68, (9/16)^t > 2^-54 up to t = 65 gives 66 (long_*)."""
    for sd, key in ((0, "left"), (1, "right")):
        for r, row in enumerate(c[key]):
            for mode in ("scratch", "chain"):
                pv = R.ising_pivot(c["par"], c["n"], list(row), sd, mode)
                assert pv["count"] == c["counts"][sd][r] and pv["count_safe"], (c["name"], sd, r, pv["count"])


@R.mp.workdps(R.DPS)
def test_cut_is_exact_at_powers_of_two():
    par = R._par([0.5, 2.0 ** -27, 2.0 ** -26], [1.0, 1.0, 1.0], 3)
    assert R.ising_pivot(par, 3, [1, 2, 2], 0)["count"] == 2          # from the bond: 2^-27, 2^-54 (dropped), ...
    assert R.ising_pivot(par, 3, [2, 2, 1], 1)["count"] == 2
    assert R.ising_pivot(par, 3, [1, 3, 2], 0)["count"] == 3          # 2^-27, 2^-53 (kept), 2^-54 (dropped)
    assert R.ising_pivot(par, 3, [2, 3, 1], 1)["count"] == 3
    pv = R.ising_pivot(par, 3, [1, 3, 2], 0)
    assert pv["near"][2] == R.mp.mpf(2) ** -53 and pv["F"] == R.mp.mpf(2) ** -54 and pv["S"] == R.mp.mpf(2) ** -27 + R.mp.mpf(2) ** -53 + R.mp.mpf(2) ** -54
    assert pv["P"] == R.mp.mpf(0.5) + R.mp.mpf(2) ** -27 + R.mp.mpf(2) ** -54


@pytest.mark.parametrize("c", ISING, ids=[c["name"] for c in ISING])
def test_table_bounds_are_tight(c):
    """every relative table bound of every pivot of the GPU tests is at most 1e-10"""
    for sd, key in ((0, "left"), (1, "right")):
        for row in c[key]:
            pv = R.ising_pivot(c["par"], c["n"], list(row), sd, "chain")
            assert pv["count_safe"]
            assert max(pv["T_rel"], pv["W_rel"], pv["F_rel"], max(pv["near_rel"])) <= 1e-10
            assert pv["S_abs"] <= 1e-10 * (1 + float(pv["S"])) and pv["P_abs"] <= 1e-10 * (1 + float(pv["P"]))


@pytest.mark.parametrize("c", MVN, ids=[c["name"] for c in MVN])
def test_mvn_reference_vs_oracle_and_conditions(c):
    d, n = c["d"], c["n"]
    aux = R.mvn_aux(c, O.mvn_init(d))
    M = R.Mvn(aux, d)
    par = R.mvn_nodes(c, aux)
    ind = _indices(c)
    orc = O.fun(3, [n] * d, par, np.array(ind, dtype=np.int32), aux)
    for t, ix in enumerate(ind):
        det = M.detail(par, ix)
        with R.mp.workdps(R.DPS):
            assert abs(R.mp.mpf(float(orc[t])) - det["value"]) <= det["oracle_rel"] * det["value"], (c["name"], ix)
        assert float(det["value"]) >= 1e-250 and det["rel"] <= 1e-10, (c["name"], ix, float(det["value"]), det["rel"])
    assert R.mvn(par, aux, ind[0]) == M.detail(par, ind[0])["value"]


@R.mp.workdps(R.DPS)
def test_definitions_on_a_case_small_enough_to_do_by_hand():
    """d = 2, nodes (1/2, 1/4): ranges {1/2}, {1/4}, {1/8}: rho = (1/3)(3/5)(7/9) = 7/45; v = 1 + 1/4 + 1/8, w = 1 + 1/2 + 1/8."""
    par = R._par([0.5, 0.25], [2.0, 3.0], 2)
    rho = R.mp.mpf(7) / 45
    assert abs(R.ising_de(par, 2, (1, 2)) - 2 * rho * rho * 6 / (R.mp.mpf(11) / 8 * R.mp.mpf(13) / 8)) < R.mp.mpf(10) ** -55
    par[4] = 3.0
    assert abs(R.ising_de(par, 2, (1, 2)) - 2 * rho * rho * 6) < R.mp.mpf(10) ** -55
