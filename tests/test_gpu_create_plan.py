"""What engine creation decides (ttcross_amd/csrc/ttx_create_plan.h), read back through the entry points an engine already has:
plan(), sweep_path(), cluster_eval(), arith and the error text.  tests/test_create_plan_cpu.py holds the whole plan of many more
configurations on the CPU; here a few of them are created on the device, at the limits that switch a variant off.  The
expectations are written out from the ladder of ttx_create as it stood before the plan existed (commit c9b06ee).  Engines are only
created, except for one small mvn run at the end: the buffers the plan sized are the buffers the kernels use."""
import numpy as np
import pytest

from ttcross_amd import drivers as D
from ttcross_amd import engine as E

pytestmark = pytest.mark.gpu

DRAW3 = "k_lottery + %s + k_lottery"


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ("TTX_SWEEP", "TTX_ARITH", "TTX_CL_PAD", "TTX_CLUSTER_NB", "TTX_DE_LOT_POINT", "TTX_DE_CUT", "TTX_DE_V2", "TTX_MVN_V2"):
        monkeypatch.delenv(name, raising=False)


def _engine(s, r, piv=2, **kw):
    return E.TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], aux=s["aux"], **kw)


C6 = D.ising_setup("c", 7, 9)       # Ising C, d = 6 cores, n = 9, nodes in [0,1]


def test_ising_c_takes_the_cluster_path_with_padded_rows():
    tt = _engine(C6, 4)
    assert tt.sweep_path() == "cluster" == tt.plan()["path"]
    assert tt.cluster_eval() == "chunks" and tt.arith == "exact"


def test_ising_c_above_rank_64_has_no_whole_sweep_kernel():
    tt = _engine(C6, 65)
    assert tt.sweep_path() == "chain" and tt.cluster_eval() == "none"


def test_fused_serves_two_groups_only_on_request(monkeypatch):
    assert _engine(C6, 4, nproc=2).sweep_path() != "fused"
    monkeypatch.setenv("TTX_SWEEP", "fused")
    assert _engine(C6, 4, nproc=2).sweep_path() == "fused"


def test_ising_c_fast_is_the_closed_form_of_the_cluster_kernel():
    tt = _engine(C6, 4, arith="fast")
    assert tt.arith == "fast" and tt.sweep_path() == "cluster" and tt.cluster_eval() == "closed"


def test_ising_d_with_more_units_than_partial_records_keeps_the_generic_kernels():
    """n = 257, r = 128: 128 * ceil(257 / 64) = 640 units of a wave-per-pivot half-step, more than the 512 partial records a group
    has; the compact tables stay (the nodes lie in [0,1]).  About 0.3 GB, created and not run."""
    p = _engine(D.ising_setup("d", 4, 257), 128).plan()
    assert (p["tables"], p["lottery"], p["halfstep"]) == ("k_de_ctables", "k_lottery", "k_halfstep<ISING>")


@pytest.mark.parametrize("d,kernel", [(160, "k_lottery_eval_decp"), (161, "k_lottery_eval_dec")])
def test_ising_d_lottery_candidates_leave_the_point_evaluator_above_160_dimensions(d, kernel):
    tt = _engine(D.ising_setup("d", d + 1, 9), 6)
    assert tt.d == d and tt.plan()["lottery"] == DRAW3 % kernel


def test_stdnorm_is_refused_where_the_lottery_rows_pass_their_budget():
    """n = 2, r = 128: the lottery stages 110 800 bytes at d = 200 and would need 131 280 at d = 240, against 120 KB."""
    par = np.array([-1.0, 1.0])
    E.TTCross([2] * 200, E.TTX_FUN_STDNORM, par, 128, pivoting=2)
    with pytest.raises(E.TTXError, match="too large for LDS staging"):
        E.TTCross([2] * 240, E.TTX_FUN_STDNORM, par, 128, pivoting=2)


def test_mvn_runs_in_the_buffers_the_plan_sized():
    """mvn, d = 6, n = 9, r = 4, default settings, run to completion: value, evaluations and ranks of the same run before the plan
    existed (commit c9b06ee on an MI355X; the oracle gives the same)."""
    s = D.box_setup("mvn", 6, 9)
    tt = _engine(s, 4).run()
    assert tt.plan()["halfstep"] == "k_halfstep_mvn"
    assert tt.quad(s["quad"]) == MVN_VALUE and tt.neval == MVN_NEVAL
    assert list(tt.ranks()) == MVN_RANKS


MVN_VALUE, MVN_NEVAL, MVN_RANKS = 15.833567226600309, 946, [1, 3, 3, 3, 3, 3, 1]
