"""The operations on the resident train share one table of device work space, one table uploader and one set of timers per engine
(ttcross_amd/csrc/ttx_engine.hip: SC_*, OpMeta, OpTimer; what a call reserves and launches: ttx_op_plan.h).  Whatever ran before on an engine, and whatever size it left a slot at,
must not enter a result: every call of an interleaved sequence equals the same call on fresh engines bit for bit, and the figures
a family reports (contract_modesum, algebra_last, eval_last_mode) are those of its own last call.

Correctness against numpy is the business of test_gpu_tijk_batch / _contract / _algebra / _sample; the only bound here is the one
test_gpu_tijk_batch.py derives for mode "mfma", whose atomic bucket order the hardware is free to change from call to call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import test_gpu_tijk_batch as TB
import tt_ref as R
from ttcross_amd import engine as E

N = (3, 5, 4, 6)
CORES = R.rand_train(41, N, (1, 2, 3, 2, 1)), R.rand_train(42, N, (1, 3, 2, 2, 1))
NPTS = 150                                                              # chunks of 64, 64 and 22
KEEP = (1, 0, 1, 1)
FIXED = (0, 2, 0, 0)
COEF = (1.5, -0.25)
_rng = np.random.default_rng(43)
IND = np.ascontiguousarray((_rng.integers(0, 2 ** 31 - 1, (NPTS, len(N))) % np.asarray(N) + 1).astype(np.int32))
X = _rng.uniform(0.0, 1.0, (NPTS, 2))
U = _rng.random((NPTS, len(N)))
W = [_rng.uniform(0.5, 1.5, nk) for nk in N]


def _engines(cores=CORES):
    return [E.TTCross.from_cores(c) for c in cores]


def _take(tt):
    """the cores of a train an operation made, which is closed"""
    out = [tt.core(k) for k in range(1, tt.d + 1)]
    tt.close()
    return out


OPS = {
    "exact": lambda a, b, m: a.tijk_batch(IND[:m], "exact"),
    "mfma": lambda a, b, m: a.tijk_batch(IND[:m], "mfma"),
    "value": lambda a, b, m: a.value_batch(X[:m], "exact"),
    "marginals": lambda a, b, m: a.marginals(),
    "contract": lambda a, b, m: _take(a.contract(KEEP, W)),
    "lincomb": lambda a, b, m: _take(E.TTCross.lincomb(COEF, [a, b])),
    "hadamard": lambda a, b, m: _take(a.hadamard(b)),
    "sample": lambda a, b, m: a.sample(U[:m], W, FIXED),
}
# sizes that make the slots grow between their uses: the staging blocks go from 7 points to a chunk of 64, the tables of one
# family follow those of another
SEQUENCE = [("exact", 7), ("mfma", 7), ("sample", NPTS), ("marginals", 0), ("exact", NPTS), ("mfma", NPTS), ("contract", 0), ("sample", 7),
            ("hadamard", 0), ("value", NPTS), ("lincomb", 0), ("marginals", 0)]


@pytest.fixture(scope="module")
def fresh():
    """every operation at full size, each on engines of its own; computed once, read-only"""
    mp = pytest.MonkeyPatch()
    mp.setenv("TTX_IJK_CHUNK", "64")
    mp.setenv("TTX_SAMPLE_CHUNK", "64")
    out = {}
    for name, op in OPS.items():
        a, b = _engines()
        out[name] = op(a, b, NPTS)
        a.close()
        b.close()
    mp.undo()
    return out


def _arrays(res):
    if isinstance(res, dict):
        return [res[k] for k in ("ind", "logq", "val")]
    return list(res) if isinstance(res, list) else [res]


def _assert_same(name, got, want, m):
    """bit for bit; the first m points of a batched result (a point depends neither on its batch nor on its neighbours)"""
    if name == "mfma":
        bound = TB._bound(list(CORES[0]), IND[:m])
        assert np.all(np.abs(got - want["exact"][:m]) <= bound)
        return
    g, w = _arrays(got), _arrays(want[name])
    assert len(g) == len(w)
    for x, y in zip(g, w):
        y = y[:m] if name in ("exact", "value", "sample") else y
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name


def test_interleaved_calls_equal_fresh_ones_and_figures_stay_per_operation(fresh, monkeypatch):
    monkeypatch.setenv("TTX_IJK_CHUNK", "64")
    monkeypatch.setenv("TTX_SAMPLE_CHUNK", "64")
    a, b = _engines()
    for rep in range(2):
        for name, m in SEQUENCE:
            _assert_same(name, OPS[name](a, b, m), fresh, m)
    assert a.eval_last_mode == "exact"                                  # the value_batch of the sequence
    # a family's figures are those of its own last call; bytes of the mode sums: 8 r(k-1) n(k) r(k) over the contracted modes
    OPS["contract"](a, b, 0)
    ct = a.contract_modesum()
    assert ct[1] == 8.0 * 2 * 5 * 3
    _assert_same("sample", OPS["sample"](a, b, NPTS), fresh, NPTS)
    assert a.contract_modesum() == ct                                   # the same bytes and the same ms
    OPS["hadamard"](a, b, 0)
    alg = a.algebra_last()
    assert alg[1] > 0.0 and alg[2] > 0.0
    OPS["mfma"](a, b, 7)
    _assert_same("marginals", OPS["marginals"](a, b, 0), fresh, 0)
    assert a.contract_modesum()[1] == 8.0 * (1 * 3 * 2 + 2 * 5 * 3 + 3 * 4 * 2 + 2 * 6 * 1)
    _assert_same("sample", OPS["sample"](a, b, 7), fresh, 7)
    assert a.algebra_last() == alg
    assert a.eval_last_mode == "mfma"


def test_a_refused_lincomb_leaves_the_next_one_as_it_would_have_been():
    """ranks 3 + 70 + 70 on both bonds: refused with the "add up to" text; 3 + 70 on the same engines afterwards: as on fresh ones"""
    n = (3, 4, 3)
    cores = [R.rand_train(51, n, (1, 3, 3, 1)), R.rand_train(52, n, (1, 70, 70, 1)), R.rand_train(53, n, (1, 70, 70, 1))]
    small, big, big2 = _engines(cores)
    with pytest.raises(E.TTXError, match="add up to 143"):
        E.TTCross.lincomb((1.0, 1.0, 1.0), [small, big, big2])
    got = _take(E.TTCross.lincomb(COEF, [small, big]))
    f_small, f_big = _engines(cores[:2])
    want = _take(E.TTCross.lincomb(COEF, [f_small, f_big]))
    assert [c.shape for c in got] == [(1, 3, 73), (73, 4, 73), (73, 3, 1)]
    assert all(np.array_equal(x, y) for x, y in zip(got, want))
