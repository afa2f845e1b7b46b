"""The integer cases of tests/exact_cases.py on the references alone, without a GPU: the conditions that keep
tests/test_gpu_exact_decisions.py from passing vacuously.  Top-K: the arithmetic is exact, the cut of every real selection falls
inside a group of equal scores, the tie groups cross chunks of 4096 positions where the case is meant to, and the final ordering
meets ties in |val|.  Sampling: the arithmetic is exact, every t lies exactly on an edge of the CDF, the reference's draw is the closed
form, and sample_ref.verify -- the checker of test_gpu_sample.py -- calls more than 90 % of these samples undecided: it cannot
see what the device does there, which is why the GPU file compares indices for equality instead."""
import numpy as np
import pytest

import exact_cases as X
import sample_ref as S
import topk_ref as R


def _rows(ind):
    return sorted(map(tuple, np.asarray(ind).tolist()))


# ---- top-K -----------------------------------------------------------------------------------------------------------------------
def test_the_generators_build_what_they_say():
    for name, c in X.TOPK.items():
        cores, q = X.topk_case(name), c["q"]
        assert [g.shape for g in cores] == [(c["r"][k], c["n"][k], c["r"][k + 1]) for k in range(len(c["n"]))]
        for g in cores:
            assert np.array_equal(g, np.rint(g)) and g.min() >= c["lo"] and g.max() <= c["hi"]
            assert np.all(np.abs(g).sum(axis=(0, 2)) > 0)                       # no slice is all zero
            assert np.array_equal(g[:, q:, :], -g[:, :-q, :])                   # the sign flips by period
    for name, c in X.SAMPLE.items():
        (cores, u), q = X.sample_case(name), c["q"]
        for g in cores:
            assert np.array_equal(g, np.rint(g)) and g.min() == 0 and g.max() <= 2
            assert np.array_equal(g[:, q:, :], g[:, :-q, :])
            dead = np.isin(np.arange(g.shape[1]) % q, c["zero"])
            assert not g[:, dead, :].any() and np.all(g[0, ~dead, :] > 0) and np.all(g[:, ~dead, 0] > 0)
        assert u.shape == (X.NPTS, len(c["n"])) and (u == 0.0).any() and (u == 1.0).any() and u.min() >= 0.0 and u.max() <= 1.0
        reps = np.array(c["n"]) // q
        assert np.array_equal(u * reps, np.rint(u * reps))


@pytest.mark.parametrize("name", list(X.TOPK))
def test_topk_is_exact_and_every_cut_falls_inside_a_tie_group(name):
    cores = X.topk_case(name)
    for K in X.TOPK[name]["K"]:
        ind, modes = X.cut_trace(cores, K, check=True)                          # exact_check's walk, with the cuts it met
        ref = X.topk_search(name, K)
        assert not ref["nan"] and ref["nfound"] == K
        assert _rows(ind) == _rows(ref["ind"])                                  # the threshold walk keeps the rows of the stable argsort
        assert modes, (name, K, "no real selection")
        for k, m in modes.items():
            print(f"{name} K={K} mode {k}: M {m['M']} T {m['T']:g} need {m['need']} equal {m['equal'].size}")
            assert m["need"] >= 1 and m["equal"].size > m["need"], (name, K, k, m["need"], m["equal"].size)
        if name == "full_sheet":
            assert modes[1]["M"] == 2 ** 24 and K * max(X.TOPK[name]["n"]) == 2 ** 24
        if name == "full_sheet" or (name == "ties_chunks" and K in (1000, 4096)):
            eq, need = modes[1]["equal"], modes[1]["need"]
            kept = eq[:need]
            print(f"{name} K={K}: kept ties in chunks {kept[0] // X.CHUNK} .. {kept[-1] // X.CHUNK}, {eq.size - need} ties not kept")
            assert kept[-1] // X.CHUNK > kept[0] // X.CHUNK                     # the kept tied keys span at least two chunks
            assert eq.size > need and eq[need] > kept[-1]                       # and tied keys that are not kept follow them
    assert X.exact_check(cores, K=X.TOPK[name]["K"][0])                         # the entry the issue names, once


def test_the_chunk_counts_of_ties_chunks():
    """mode 1 of ties_chunks is a sheet of 4 / 16 / 64 chunks at K = 256 / 1000 / 4096 (the second one partly filled)"""
    n = X.TOPK["ties_chunks"]["n"]
    assert [-(-K * n[0] // X.CHUNK) for K in X.TOPK["ties_chunks"]["K"]] == [4, 16, 64]


@pytest.mark.parametrize("name,K", X.WHICH_CASES)
def test_the_ordering_meets_ties_in_abs_val(name, K):
    by = {w: X.topk_search(name, K, w) for w in ("abs", "max", "min")}
    assert _rows(by["abs"]["ind"]) == _rows(by["max"]["ind"]) == _rows(by["min"]["ind"])
    val = by["abs"]["val"]
    assert np.unique(np.abs(val)).size < val.size                               # ties in |val|
    assert set(val[val > 0]) & set(-val[val < 0])                               # a pair of rows with val = +-v
    for w in ("max", "min"):
        assert np.unique(by[w]["val"]).size < val.size                          # and ties in val itself
    # inside a run of equal keys the rows ascend lexicographically
    for w, key in (("abs", np.abs(val)), ("max", by["max"]["val"]), ("min", by["min"]["val"])):
        rows = by[w]["ind"].tolist()
        runs = [j for j in range(1, len(rows)) if key[j] == key[j - 1]]
        assert runs and all(rows[j - 1] < rows[j] for j in runs)


def test_the_fixed_case_cuts_inside_tie_groups_too():
    name, K, fixed = X.FIXED_CASE
    ind, modes = X.cut_trace(X.topk_case(name), K, fixed, check=True)
    ref = X.topk_search(name, K, "abs", fixed)
    assert _rows(ind) == _rows(ref["ind"]) and np.all(ref["ind"][:, 1] == 3)
    assert modes
    for k, m in modes.items():
        assert m["need"] >= 1 and m["equal"].size > m["need"], (k, m["need"], m["equal"].size)


def test_the_refusal_case_lies_one_mode_size_beyond_the_sheet():
    cores = X.refusal_train()
    assert [g.shape[1] for g in cores] == [3, 4097]
    assert 4096 * 4097 == 2 ** 24 + 4096 and 4095 * 4097 <= 2 ** 24
    assert X.cut_trace(cores, 4095, check=True)[1]                              # K = 4095 is a real selection, and exact


# ---- sampling --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(X.SAMPLE))
def test_sampling_is_exact_and_every_t_lies_on_an_edge(name):
    c = X.SAMPLE[name]
    cores, u = X.sample_case(name)
    n, q = c["n"], c["q"]
    assert X.exact_check(cores, u=u)
    assert X.exact_check(cores, u=X.below(u))
    ind, logq, val, failed = S.draw(cores, u)
    assert not failed.any()
    assert np.array_equal(ind, X.edge_closed_form(n, q, c["zero"], u))
    walk_ind, modes = X.sample_walk(cores, u)
    assert np.array_equal(walk_ind, ind)
    rows = np.arange(X.NPTS)
    at64, beyond = 0, 0
    for k, nk in enumerate(n):
        reps = nk // q
        j = np.rint(u[:, k] * reps).astype(np.int64)
        m = modes[k + 1]
        edge = np.where(j > 0, m["c"][rows, np.maximum(q * j - 1, 0)], 0.0)     # c(q j - 1), c(-1) = 0
        assert np.array_equal(m["t"], edge)
        inner = (j > 0) & (j < reps)
        at64 += int((inner & ((q * j) % 64 == 0)).sum())
        beyond += int((inner & (q * j > 1024)).sum())
        if 0 in c["zero"]:                                                      # p = 0 right after every edge
            assert not m["p"][:, ::q].any()
    res = S.verify(cores, u, None, None, ind)
    print(name, "undecided for sample_ref.verify", res["undecided"], "of", X.NPTS, "edges at a multiple of 64:", at64, "beyond 1024:", beyond)
    assert res["undecided"] > 0.9 * X.NPTS
    if max(n) > 64:
        assert at64 >= 1
    if name == "edge_long":
        assert beyond >= 1


def test_the_weighted_case_is_exact():
    cores, u = X.sample_case(X.WEIGHTED)
    w = X.weights(X.WEIGHTED)
    for q in w:
        assert set(q) == {0.0, 0.5, 1.0, 2.0}
        assert not np.array_equal(q[8:], q[:-8])
    assert X.exact_check(cores, u=u, w=w)
    ind, logq, val, failed = S.draw(cores, u, w)
    assert not failed.any()
    for k, q in enumerate(w):
        assert np.all(q[ind[:, k] - 1] > 0.0)                                   # an index of weight 0 is never drawn
