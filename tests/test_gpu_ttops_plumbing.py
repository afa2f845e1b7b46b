"""The host plumbing of the tt_lib utilities (QR plan, scratch map, core moves, temporaries): both branches of svd_impl in one call
against tests/tt_ref.py, norm / lognrm leaving the train as it was, repeatable accchk / quad / zquad on one engine, and an engine
that goes on working after a refused call.  Small uploaded trains (d = 3, modes <= 13) and one tiny sweep.

TWO_BRANCH is the train of ranks [1, 6, 2, 1] and modes [2, 2, 5].  dtt_svd orthogonalises first, which cuts its first bond to
min(1 * 2, 6) = 2, so all its unfoldings are wide by the time they are decomposed; TALL ([1, 5, 12, 1] on modes [5, 3, 2]) keeps
a 12 x 2 unfolding of core 3 through the orthogonalisation and reaches the tall branch next to the wide one of core 2."""
import numpy as np
import pytest

import tt_ref as R
from test_ttops_ref_cpu import assert_round
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

pytestmark = pytest.mark.gpu

TWO_BRANCH = R.rand_train(7, [2, 2, 5], [1, 6, 2, 1])
TALL = R.rand_train(8, [5, 3, 2], [1, 5, 12, 1])
TOLS = [(1e-1, 0), (1e-8, 0), (1e-12, 1)]


def _cores(t):
    return [t.core(k) for k in range(1, t.d + 1)]


@pytest.mark.parametrize("c", [TWO_BRANCH, TALL], ids=["two_branch", "tall"])
def test_svd_branches(c):
    for tol, rmax in TOLS:
        ref = R.tt_svd_ref(c, tol, rmax)
        assert min(ref["margin"]) >= 1e-6, "the case sits on a chop threshold"
        t = E.TTCross.from_cores(c).svd(tol, rmax)
        assert_round(_cores(t), list(t.ranks()), c, tol, rmax, ref, f"tol {tol} rmax {rmax}", tol_rel=1e-11)


@pytest.mark.parametrize("tol", [None, 1e-8])
@pytest.mark.parametrize("c", [TWO_BRANCH, TALL], ids=["two_branch", "tall"])
def test_norm_and_lognrm_leave_the_train_untouched(c, tol):
    t = E.TTCross.from_cores(c)
    before, ranks = [x.tobytes() for x in _cores(t)], list(t.ranks())
    for f in (t.norm, t.lognorm):
        v = f(tol)
        assert [x.tobytes() for x in _cores(t)] == before and list(t.ranks()) == ranks
        assert f(tol) == v
    nrm = R.norm(c)
    assert abs(t.norm(tol) - nrm) <= 1e-12 * nrm


@pytest.fixture(scope="module")
def swept():
    s = D.ising_setup("c", 5, 17)
    return s, E.TTCross(s["n"], s["fun_id"], s["par"], 8, pivoting=2, accuracy=s["acc"], quad=s["quad"]).run()


def _zw(t, nf=2):
    x = np.arange(int(sum(t.core(k).shape[1] for k in range(1, t.d + 1))))
    return np.array([np.exp(1j * (k + 1) * 0.01 * x) / (1 + x) for k in range(nf)])


def test_repeatable_on_one_engine(swept):
    s, t = swept
    a, b = t.accchk(300), t.accchk(300)
    assert all(np.array_equal(a[k], b[k]) for k in ("einf", "efro", "ainf", "afro", "pivot"))
    assert t.quad(s["quad"]) == t.quad(s["quad"])
    assert t.zquad(_zw(t)).tobytes() == t.zquad(_zw(t)).tobytes()


def test_engine_survives_refused_calls(swept):
    s, t = swept
    acc, q, z = t.accchk(300), t.quad(s["quad"]), t.zquad(_zw(t))
    with pytest.raises(E.TTXError, match="nlot must be positive"):
        t.accchk(0)
    with pytest.raises(E.TTXError, match="ztt_quad: bad argument"):
        t.zquad(np.zeros((0, _zw(t).shape[1]), dtype=np.complex128))
    assert t.accchk(300)["einf"] == acc["einf"] and t.quad(s["quad"]) == q and t.zquad(_zw(t)).tobytes() == z.tobytes()
    x = E.TTCross.from_cores(R.rand_train(9, [3, 3, 3], [1, 2, 2, 1]))
    y = E.TTCross.from_cores(R.rand_train(10, [3, 3, 3], [1, 3, 3, 1]))
    xx, nx = x.dot(x), x.norm(1e-8)
    with pytest.raises(E.TTXError, match="ranks of y exceed the work space of x"):
        x.dot(y)
    assert x.dot(x) == xx and x.norm(1e-8) == nx
    assert abs(y.dot(x) - R.quad([np.einsum("ajb,cjd->acbd", p, q).reshape(p.shape[0] * q.shape[0], 1, -1) for p, q in zip(_cores(x), _cores(y))],
                                 [[1.0]] * 3)) <= 1e-12 * R.norm(_cores(x)) * R.norm(_cores(y))
