"""The table evaluators of TTX_ARITH=fast (ttcross_amd/csrc/ttx_fast.h) element by element against a plain mpmath reference
(tests/fast_ref.py), every value at its own derived rounding bound -- no tolerance is chosen here.

ttx_k_fast_block builds the tables of a hand-made bond (from scratch, or grown by the child update) and evaluates the whole block
[rL][n][n][rR] by the three routes of a bond step (lottery candidates, column fibers, row fibers) and full multi-indices by the
one-wave point evaluator, calling the device functions the sweep kernels call.  ttx_fast_tables returns the tables a real run left.
The inputs (fast_ref.ising_cases / mvn_cases) are chosen by the branch they reach: empty pivots at both ends, decay counts on
either side of the 24-entry register path, arguments exactly at 2^-54 and 2^-53, nodes 0 and 1, counts above 64 at d = 70.
Each test prints `RATIO <case> <what> <largest error / bound>` before it asserts (profiles/fast_elements_mi355x.txt).
"""
import numpy as np
import pytest

import fast_ref as R
import oracle_lib as O
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

pytestmark = pytest.mark.gpu

ISING = {c["name"]: c for c in R.ising_cases()}
MVN = {c["name"]: c for c in R.mvn_cases()}
_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


class Worst:
    """largest error / bound of a case; every comparison goes through here"""

    def __init__(self, case):
        self.case, self.ratio, self.bad = case, {}, []

    def check(self, what, got, ref, bound, where):
        got = float(got)
        assert np.isfinite(got), f"{self.case} {what} {where}: {got}"
        with R.mp.workdps(R.DPS):
            err = abs(float(R.mp.mpf(got) - ref))
        if bound == 0.0:
            ok, ratio = err == 0.0, (0.0 if err == 0.0 else np.inf)
        else:
            ratio = err / bound
            ok = ratio <= 1.0
        self.ratio[what] = max(self.ratio.get(what, 0.0), ratio)
        if not ok:
            self.bad.append(f"{what} {where}: got {got!r} ref {float(ref)!r} err {err:.3e} bound {bound:.3e}")

    def finish(self):
        for k, v in self.ratio.items():
            print(f"RATIO {self.case} {k} {v:.3f}")
        assert not self.bad, f"{self.case}: {len(self.bad)} values outside their bound, first: " + "; ".join(self.bad[:4])


def _ising_refs(c):
    return _memo(("ie", c["name"]), lambda: [R.ising_de_detail(c["par"], c["n"], ix) for ix in R.block_indices(c)])


def _ising_pivots(c, mode):
    return _memo(("ip", c["name"], mode), lambda: [[R.ising_pivot(c["par"], c["n"], list(row), sd, mode) for row in c[key]]
                                                    for sd, key in ((0, "left"), (1, "right"))])


def _check_ising_tables(w, tag, pivs, near, piv, counts=None):
    """near [FD][r], piv [8][r] of one side against the references pivs[r]"""
    for cidx, pv in enumerate(pivs):
        where = f"pivot {cidx}"
        assert pv["count_safe"], f"{w.case} {tag} {where}: a near entry sits at the cut, the count is not defined by the inputs"
        cnt = int(piv[5, cidx])
        assert piv[5, cidx] == pv["count"], f"{w.case} {tag} {where}: FP_N {piv[5, cidx]} != {pv['count']}"
        if counts is not None:
            assert cnt == counts[cidx], f"{w.case} {tag} {where}: FP_N {cnt} != hand-computed {counts[cidx]}"
        for t in range(cnt):
            w.check(f"{tag}.near", near[t, cidx], pv["near"][t], pv["near_rel"][t] * float(pv["near"][t]), f"{where} t {t}")
        w.check(f"{tag}.T", piv[0, cidx], pv["T"], pv["T_rel"] * abs(float(pv["T"])), where)
        w.check(f"{tag}.W", piv[1, cidx], pv["W"], pv["W_rel"] * abs(float(pv["W"])), where)
        w.check(f"{tag}.S", piv[2, cidx], pv["S"], pv["S_abs"], where)
        w.check(f"{tag}.P", piv[3, cidx], pv["P"], pv["P_abs"], where)
        w.check(f"{tag}.F", piv[4, cidx], pv["F"], pv["F_rel"] * abs(float(pv["F"])), where)


@pytest.mark.parametrize("mode", ["scratch", "chain"])
@pytest.mark.parametrize("name", list(ISING))
def test_ising_block_every_element_every_route(name, mode):
    """Tables, the whole block by the lottery, column-fiber and row-fiber routes at every cap, and the point route."""
    c = ISING[name]
    refs, pivs = _ising_refs(c), _ising_pivots(c, mode)
    rl, rr, n, d, p = len(c["left"]), len(c["right"]), c["n"], c["d"], c["p"]
    w = Worst(f"{name}/{mode}")
    prefs = [R.ising_de_detail(c["par"], n, tuple(ix)) for ix in c["points"]]
    nfar_seen = set()
    for cap in c["caps"]:
        o = E.k_fast_block(D.TTX_FUN_ISING, d, n, c["par"], p, c["left"], c["right"], cap, mode=mode, points=c["points"])
        if cap == c["caps"][0]:
            for sd, tag, r in ((0, "L", rl), (1, "R", rr)):
                _check_ising_tables(w, tag, pivs[sd], o["near"][sd][:, :r], o["piv"][sd][:, :r], c.get("counts", (None, None))[sd])
            for t, det in enumerate(prefs):
                w.check("point", o["point"][t], det["value"], R.ising_elem_bound(det, p - 1, d - p - 1, mode, "point") * abs(float(det["value"])), f"point {t}")
        nfar_seen |= set(o["nfar_col"].ravel().astype(int)) | set(o["nfar_row"].ravel().astype(int))
        for route in ("lottery", "col", "row"):
            got = o[route].ravel()
            for t, det in enumerate(refs):
                w.check(route, got[t], det["value"], R.ising_elem_bound(det, p - 1, d - p - 1, mode, route) * abs(float(det["value"])), f"cap {cap} element {t}")
    if c.get("need_nfar"):          # both fiber branches ran on this data: far vector in registers (<= 24 entries) and in LDS
        assert min(nfar_seen) <= 24 < max(nfar_seen), nfar_seen
    if c.get("zeros"):
        assert any(det["value"] == 0 for det in refs) and any(det["value"] != 0 for det in refs)
    w.finish()


def _mvn_setup(c):
    skew = bool(c.get("skew"))
    aux = _memo(("aux", c["d"], skew), lambda: R.mvn_aux(c, O.mvn_init(c["d"])))
    return aux, _memo(("M", c["d"], skew), lambda: R.Mvn(aux, c["d"])), R.mvn_nodes(c, aux)


@pytest.mark.parametrize("mode", ["scratch", "chain"])
@pytest.mark.parametrize("name", list(MVN))
def test_mvn_block_every_element_every_route(name, mode):
    """mvn: dv, Y = S dv and Q of every pivot, the block by the three routes and the point route (d = 70: rows beyond lane 63)."""
    c = MVN[name]
    aux, M, par = _mvn_setup(c)
    d, n, p = c["d"], c["n"], c["p"]
    refs = _memo(("me", name), lambda: [M.detail(par, ix) for ix in R.block_indices(c)])
    w = Worst(f"{name}/{mode}")
    o = E.k_fast_block(D.TTX_FUN_MVN, d, n, par, p, c["left"], c["right"], 0, mode=mode, aux=aux, points=c["points"])
    for sd, key, d0 in ((0, "left", 0), (1, "right", p + 1)):
        for cidx, row in enumerate(c[key]):
            pv = _memo(("mp", name, sd, cidx), lambda: M.pivot(par, row, d0))
            assert np.array_equal(o["dv"][sd][:len(row), cidx], pv["dv"]), f"{name} dv side {sd} pivot {cidx}"
            for r_ in range(d):
                w.check("Y", o["near"][sd][r_, cidx], pv["Y"][r_], pv["Y_abs"][r_], f"side {sd} pivot {cidx} row {r_}")
            w.check("Q", o["piv"][sd][0, cidx], pv["Q"], pv["Q_abs"], f"side {sd} pivot {cidx}")
    for route in ("lottery", "col", "row"):
        got = o[route].ravel()
        for t, det in enumerate(refs):
            w.check(route, got[t], det["value"], det["rel"] * float(det["value"]), f"element {t}")
    for t, ix in enumerate(c["points"]):
        det = M.detail(par, tuple(ix))
        w.check("point", o["point"][t], det["value"], det["rel"] * float(det["value"]), f"point {t}")
    w.finish()


RUNS = [("ising", "d", 12, 17, 8, 1), ("ising", "e", 9, 17, 8, 3), ("mvn", "", 9, 17, 8, 2)]


@pytest.mark.parametrize("fun,kind,m,n,r,nproc", RUNS, ids=[f"{c[0]}{c[1]}{c[2]}_np{c[5]}" for c in RUNS])
def test_tables_left_by_a_real_run(fun, kind, m, n, r, nproc):
    """Every table entry of every bond and group after a fast-mode run -- the rank-1 start, the incremental maintenance when a pivot
    is accepted, the neighbours' boundary pivots -- against the reference built from the index sets the engine itself returns."""
    s = D.ising_setup(kind, m, n) if fun == "ising" else D.box_setup("mvn", m, n)
    tt = E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=2, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], aux=s["aux"], nproc=nproc,
                   arith="fast").run()
    assert tt.arith == "fast"
    d, nn = tt.d, s["n"][0]
    w = Worst(f"run_{fun}{kind}{m}_np{nproc}")
    M = R.Mvn(s["aux"], d) if fun == "mvn" else None
    maxn, npiv = 0, 0
    for g in range(nproc):
        first, last = tt.fast_tables(g)
        for sd in (0, 1):
            for bond in range(first - 1 if sd == 0 else first, (last if sd == 0 else last + 1) + 1):
                t = tt.fast_tables(g, sd, bond, cols=r)
                ln = bond if sd == 0 else d - bond
                assert t["idx"].shape == (ln, t["r"]) and 1 <= t["r"] <= r
                assert ln == 0 or (t["idx"].min() >= 1 and t["idx"].max() <= nn)
                npiv += t["r"]
                tag = f"g{g}.{'LR'[sd]}{bond}"
                if fun == "mvn":
                    for cidx in range(t["r"]):
                        pv = M.pivot(s["par"], t["idx"][:, cidx], 0 if sd == 0 else bond)
                        assert np.array_equal(t["dv"][:ln, cidx], pv["dv"]), f"{tag} dv pivot {cidx}"
                        for r_ in range(d):
                            w.check("Y", t["near"][r_, cidx], pv["Y"][r_], pv["Y_abs"][r_], f"{tag} pivot {cidx} row {r_}")
                        w.check("Q", t["piv"][0, cidx], pv["Q"], pv["Q_abs"], f"{tag} pivot {cidx}")
                else:
                    pivs = [R.ising_pivot(s["par"], nn, list(t["idx"][:, cidx]), sd, "chain") for cidx in range(t["r"])]
                    _check_ising_tables(w, "LR"[sd], pivs, t["near"], t["piv"])
                    maxn = max(maxn, int(t["piv"][5].max()))
    assert npiv > 2 * (d - 1)           # the run grew ranks: child entries were made
    if fun == "ising":
        print(f"MAXFPN {w.case} {maxn}")
    w.finish()
