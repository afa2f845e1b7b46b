"""Which kernels the chain path launches (TTCross.plan, include/ttx.h: ttx_plan_describe).  All variants of a stage give the same
bits by design, so the parity tests cannot tell whether the variant an environment switch asks for is the one that ran: here the
selection itself is read back.  The expected strings are written out from the flag ladders of ttx_create and of the bond step as
they stood before the launch plan existed (commit 7493f19), not from the plan's builder.  Engines are only created, except for the
fault-hook run and the launch counts at the end."""
import pytest

from ttcross_amd import drivers as D
from ttcross_amd import engine as E

pytestmark = pytest.mark.gpu

DRAW3 = "k_lottery + %s + k_lottery"          # drawing launch, one wave (or DPP row) per candidate, scoring launch


def _teams(unit, a=256, b=1024, last="k_halfstep_de"):
    return f"k_halfstep_det<{unit},3>[<={a}], k_halfstep_det<{unit},1>[<={b}], {last}<{unit}>"


def _engine(s, r, piv, **kw):
    return E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], aux=s["aux"], **kw)


def _stages(tt):
    p = tt.plan()
    return p["tables"], p["lottery"], p["halfstep"]


ROWS_T, ROWS_F = "k_lottery_eval_de_rows<true,false>", "k_lottery_eval_de_rows<false,false>"
# Ising D_45, n = 9 (nodes in [0,1]), r = 6, piv = 2, one group: the shape of test_ising_de_kernel_variants_bit_exact
DE_CASES = [
    ({}, ("k_de_ctables", DRAW3 % "k_lottery_eval_decp", "k_halfstep_dec")),
    ({"TTX_DE_LOT_POINT": "0"}, ("k_de_ctables", DRAW3 % "k_lottery_eval_dec", "k_halfstep_dec")),
    ({"TTX_DE_LANE": "1"}, ("-", "k_lottery", "k_halfstep<ISING>")),
    ({"TTX_DE_V2": "0"}, ("k_de_ctables", "k_lottery", "k_halfstep<ISING>")),
    ({"TTX_DE_CUT": "0"}, ("k_de_tables", DRAW3 % ROWS_T, _teams("true"))),
    ({"TTX_DE_CUT": "0", "TTX_DE_FASTDIV": "0"}, ("k_de_tables", DRAW3 % ROWS_F, _teams("false"))),
    ({"TTX_DE_CUT": "0", "TTX_LOTTERY_ROWS": "2"}, ("k_de_tables", DRAW3 % "k_lottery_eval_de_rows<true,true>", _teams("true"))),
    ({"TTX_DE_CUT": "0", "TTX_LOTTERY_WAVE": "0"}, ("k_de_tables", "k_lottery", _teams("true"))),
    ({"TTX_DE_CUT": "0", "TTX_DE_V5": "1"}, ("k_de_tables", DRAW3 % ROWS_T, "k_halfstep_de5<true>")),
    ({"TTX_DE_CUT": "0", "TTX_DE_V2": "0"}, ("k_de_tables", "k_lottery", "k_halfstep<ISING>")),
    ({"TTX_DE_CUT": "0", "TTX_DE_TEAM": "0"}, ("k_de_tables", DRAW3 % ROWS_T, "k_halfstep_de<true>")),
    ({"TTX_DE_CUT": "0", "TTX_DE_TEAM_UNITS": "1000000"}, ("k_de_tables", DRAW3 % ROWS_T, _teams("true", a=1000000))),
    ({"TTX_DE_CUT": "0", "TTX_DE_TEAM_UNITS": "0", "TTX_DE_TEAM6_UNITS": "1000000"}, ("k_de_tables", DRAW3 % ROWS_T, _teams("true", a=0, b=1000000))),
]


@pytest.mark.parametrize("env,want", DE_CASES, ids=["+".join(f"{k[4:]}={v}" for k, v in c[0].items()) or "default" for c in DE_CASES])
def test_ising_de_variants_select_their_kernels(env, want, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tt = _engine(D.ising_setup("d", 45, 9), 6, 2)
    assert tt.plan()["path"] == "chain" == tt.sweep_path()
    assert _stages(tt) == want


def test_a_node_outside_the_unit_interval_takes_the_general_division():
    """No unit cut, so no compact tables: the full-table kernels with the IEEE division; fast arithmetic is not effective either."""
    s = D.ising_setup("d", 45, 9)
    s["par"] = s["par"].copy()
    s["par"][3] = 1.5
    want = ("k_de_tables", DRAW3 % ROWS_F, _teams("false"))
    assert _stages(_engine(s, 6, 2)) == want
    fast = _engine(s, 6, 2, arith="fast")
    assert fast.arith == "exact" and _stages(fast) == want


MVN_CASES = [({}, None, ("-", DRAW3 % "k_lottery_eval_mvn", "k_halfstep_mvn")),
             ({"TTX_MVN_V2": "0"}, None, ("-", "k_lottery", "k_halfstep<MVN>")),
             ({}, "fast", ("-", "k_lottery", "k_halfstep<MVN>")),
             ({"TTX_FAST_PERSIST": "0"}, "fast", ("k_fast_tables<MVN>", "k_lottery", "k_halfstep<MVN>"))]


@pytest.mark.parametrize("env,arith,want", MVN_CASES, ids=["exact", "lane_per_element", "fast", "fast_tables_per_step"])
def test_mvn_variants_select_their_kernels(env, arith, want, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tt = _engine(D.box_setup("mvn", 6, 9), 4, 2, arith=arith)
    assert tt.arith == (arith or "exact") and _stages(tt) == want


def test_ising_de_fast_arithmetic_runs_the_generic_kernels():
    tt = _engine(D.ising_setup("d", 45, 9), 6, 2, arith="fast")
    assert tt.arith == "fast" and _stages(tt) == ("-", "k_lottery", "k_halfstep<ISING>")


def test_path_line_agrees_with_sweep_path(monkeypatch):
    s = D.ising_setup("c", 6, 9)
    for want in ("chain", "fused", "cluster"):
        monkeypatch.setenv("TTX_SWEEP", want)
        tt = _engine(s, 4, 2)
        assert tt.plan()["path"] == tt.sweep_path()
        assert tt.sweep_path() == want or (want == "cluster" and tt.sweep_path() == "chain")     # no room for a cluster: the chain
        assert _stages(tt) == ("-", "k_lottery", "k_halfstep<ISING>")       # what the chain runs, also after a fallback


def test_full_pivoting_shapes(monkeypatch):
    s = D.ising_setup("c", 6, 9)
    p = _engine(s, 4, -1).plan()
    assert (p["lottery"], p["halfstep"], p["fullpiv"]) == ("-", "k_halfstep<ISING>", "plain")
    assert "fullpiv" not in _engine(s, 4, 2).plan()
    host = E.TTCross(s["n"], E.TTX_FUN_HOST, [], 4, pivoting=-1, accuracy=s["acc"], quad=s["quad"]).plan()
    assert (host["lottery"], host["halfstep"], host["fullpiv"]) == ("-", "k_halfstep<HOST>", "columns")
    monkeypatch.setenv("TTX_FULLPIV", "mfma")
    assert _engine(s, 4, -1).plan()["fullpiv"] == "mfma"


def test_a_team_fault_retires_the_team_tiers(monkeypatch):
    """The counted, handled condition of test_team_halfstep_fault_is_replayed_without_teams: the team launches of sweep 2 get a grid
    of one unit, k_halfstep_det counts the units it could not serve, ttx_run retires the teams and repeats the run."""
    monkeypatch.setenv("TTX_DE_CUT", "0")
    monkeypatch.setenv("TTX_DE_TEST_FAULT", "2")
    monkeypatch.setenv("TTX_DE_TEAM_UNITS", "1000000")
    tt = _engine(D.ising_setup("d", 20, 17), 8, 2)
    assert tt.plan()["halfstep"] == _teams("true", a=1000000)
    tt.run()
    assert tt.det_fallbacks == 1
    assert tt.plan()["halfstep"] == "k_halfstep_de<true>"


# Launches per kind of one run on the chain path with one bond group in one process, from the launch brackets of the bond step as
# they stood at 7493f19.  S sweeps (the records less the initial cross), B = d - 1 bond steps per sweep, H = 2 piv = 4 half-steps:
#   lottery   S B L        L = 3 (draw, candidates, score) where candidates get a launch of their own, else 1
#   halfstep  S B H
#   accept    S B
#   exchange  2 S          k_exch_pack and k_exch_max_apply (no transfer, no boundary corners with one group)
#   quad      2 S          k_quad_build and k_quad_chain (no tree with one group)
#   other     4 + T S B + 2     the initial cross (samples, fibers, factors, final), T table launches per bond step, the finalisation (two LU kernels)
COUNT_CASES = [("d", {}, 3, 1), ("d", {"TTX_DE_CUT": "0"}, 3, 1), ("mvn", {}, 3, 0)]


@pytest.mark.parametrize("kind,env,L,T", COUNT_CASES, ids=["ising_d_compact", "ising_d_full_tables", "mvn_exact"])
def test_launch_counts_per_kind(kind, env, L, T, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tt = (_engine(D.ising_setup("d", 45, 9), 6, 2) if kind == "d" else _engine(D.box_setup("mvn", 6, 9), 4, 2)).run()
    S, B = len(tt.sweeps()) - 1, tt.d - 1
    assert S >= 1 and B == (43 if kind == "d" else 5)
    got = {k: v["launches"] for k, v in tt.kernel_stats().items()}
    assert got == {"lottery": S * B * L, "halfstep": S * B * 4, "accept": S * B, "exchange": 2 * S, "quad": 2 * S, "other": 4 + T * S * B + 2}
