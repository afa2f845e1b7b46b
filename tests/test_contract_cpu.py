"""Partial contraction (ttx_contract, ttx_marginals): what can be checked without a GPU -- the C-ABI as declared and as
exported, the Python methods, and the numpy reference of tests/contract_ref.py against np.einsum on dense tensors."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

import contract_ref as C
import tt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_both_prototypes():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        h = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))
    assert "int ttx_contract(ttx_engine *h, const int32_t *keep, const double *w, ttx_engine **out);" in h
    assert "int ttx_marginals(ttx_engine *h, const double *w, double *out);" in h


def test_library_exports_both_symbols_and_keeps_version_3():
    import __graft_entry__ as g
    L = ctypes.CDLL(g.build_lib())
    for sym in ("ttx_contract", "ttx_marginals", "ttx_contract_modesum"):
        assert hasattr(L, sym), sym
    L.ttx_version.restype = ctypes.c_int
    assert L.ttx_version() == 3


def test_engine_class_has_the_methods():
    from ttcross_amd import engine as E
    assert callable(E.TTCross.contract) and callable(E.TTCross.marginals)


TRAINS = {
    "d3": ([5, 7, 4], [1, 3, 2, 1]),
    "d5_modes_of_size_1_rank_1_bond": ([4, 1, 6, 1, 5], [1, 3, 5, 1, 4, 1]),
    "d6": ([3, 2, 4, 3, 2, 3], [1, 2, 4, 3, 5, 2, 1]),
}


def _dense(cores):
    t, e = R.scaled_dense(cores)
    return np.ldexp(t, e)


def _patterns(d):
    return [kp for kp in itertools.product((0, 1), repeat=d) if sum(kp) >= 2]


@pytest.mark.parametrize("name", sorted(TRAINS))
@pytest.mark.parametrize("ones", [False, True])
def test_reference_agrees_with_einsum_on_the_dense_tensor(name, ones):
    n, r = TRAINS[name]
    d = len(n)
    cores = R.rand_train(len(name), n, r)
    rng = np.random.default_rng(d)
    w = None if ones else [rng.standard_normal(nk) for nk in n]
    wv = [np.ones(nk) for nk in n] if ones else w
    full = _dense(cores)
    letters = "abcdefgh"[:d]
    for keep in _patterns(d):
        ops, subs = [full], [letters]
        for k in range(d):
            if not keep[k]:
                ops.append(wv[k])
                subs.append(letters[k])
        want = np.einsum(",".join(subs) + "->" + "".join(letters[k] for k in range(d) if keep[k]), *ops)
        got_cores = C.contract_cores(cores, keep, w)
        assert C.ranks(got_cores) == C.stated_ranks(cores, keep)
        assert [c.shape[1] for c in got_cores] == [n[k] for k in range(d) if keep[k]]
        got = _dense(got_cores)
        # the reference and the dense tensors each carry N u B; einsum's sum over the dense contracted modes adds T u B, T its terms
        terms = int(np.prod([n[k] for k in range(d) if not keep[k]]))
        bound = (3.0 * C.count(cores, keep) + terms) * C.U * _dense(C.abs_bound(cores, keep, w))
        assert got.shape == want.shape and np.all(np.abs(got - want) <= bound), keep
    if not ones:                                                # keep-all is a copy
        for a, b in zip(C.contract_cores(cores, [1] * d, w), cores):
            assert np.array_equal(a, b)
    # marginals: every block against the dense sum over the other modes
    mg = C.marginals(cores, w)
    ab = C.marginals_abs(cores, w)
    for k in range(d):
        ops, subs = [full], [letters]
        for j in range(d):
            if j != k:
                ops.append(wv[j])
                subs.append(letters[j])
        want = np.einsum(",".join(subs) + "->" + letters[k], *ops)
        keep = [int(j == k) for j in range(d)]
        terms = int(np.prod([n[j] for j in range(d) if j != k]))
        assert np.all(np.abs(mg[k] - want) <= (3.0 * C.count(cores, keep) + terms) * C.U * ab[k]), k


def test_reference_gives_the_stated_ranks():
    n, r = [3, 5, 2, 7, 4, 6, 3, 5], [1, 3, 17, 64, 65, 9, 128, 2, 1]
    cores = R.rand_train(1, n, r)
    for kept, want in (((0, 7), [1, 3, 1]), ((3, 4), [1, 65, 1]), ((1, 6), [1, 17, 1]), ((2, 5), [1, 64, 1]), ((0, 1, 2, 5), [1, 3, 17, 64, 1]),
                       (range(8), r)):
        keep = [int(k in kept) for k in range(8)]
        assert C.stated_ranks(cores, keep) == want
        assert C.ranks(C.contract_cores(cores, keep)) == want
