"""ttx_lincomb_round without a device: the generator, the reference's two evaluations against the allowance, the conditions on the
truncation cases, and the C-ABI surface (header lines, symbols, refusals with null engines)."""
import ctypes
import os
import re

import numpy as np
import pytest

import roundsum_ref as RS
from ttcross_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def test_omega_entries_are_multiples_of_2_to_minus_52_inside_the_open_interval():
    v = E.roundsum_omega(12345, 3, (16, 7, 16)).ravel(order="F")
    assert v.dtype == np.float64 and np.all(np.abs(v) < 1.0)
    j = v * 2.0 ** 52
    assert np.array_equal(j, np.round(j)) and np.all(np.abs(j) <= 2.0 ** 52 - 1)


def test_omega_mean_and_variance():
    """N = 10^6 draws of uniform(-1, 1): the mean has deviation sqrt(1 / 3N), the sample variance sqrt(4 / 45N) (the fourth
    central moment of the distribution is 1 / 5); five deviations each"""
    N = 10 ** 6
    v = E.roundsum_omega(7, 2, (100, 100, 100)).ravel(order="F")
    assert v.size == N
    assert abs(v.mean()) <= 5.0 * np.sqrt(1.0 / (3.0 * N))
    assert abs(v.var() - 1.0 / 3.0) <= 5.0 * np.sqrt(4.0 / (45.0 * N))
    # cores and seeds are streams of their own
    assert abs(np.corrcoef(v, E.roundsum_omega(7, 3, (100, 100, 100)).ravel(order="F"))[0, 1]) <= 5.0 / np.sqrt(N)
    assert abs(np.corrcoef(v, E.roundsum_omega(8, 2, (100, 100, 100)).ravel(order="F"))[0, 1]) <= 5.0 / np.sqrt(N)


def _omega_by_hand(seed, k, x):
    """the recipe of include/ttx.h in Python integers"""
    M = 2 ** 64
    z = (seed + 0x9E3779B97F4A7C15 * ((k << 40) + x + 1)) % M
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % M
    z = z ^ (z >> 31)
    mag = ((z >> 11) & (2 ** 52 - 1)) / 2.0 ** 52
    return -mag if z >> 63 else mag


def test_omega_first_values_are_pinned():
    v = E.roundsum_omega(0, 1, (2, 3, 2))
    assert v.shape == (2, 3, 2)
    flat = v.ravel(order="F")
    assert flat.tolist() == [_omega_by_hand(0, 1, x) for x in range(12)]
    assert flat[:4].tolist() == PINNED
    big = E.roundsum_omega(2 ** 64 - 1, 255, (3, 2, 2)).ravel(order="F")
    assert big.tolist() == [_omega_by_hand(2 ** 64 - 1, 255, x) for x in range(12)]
    assert v[1, 2, 1] == flat[1 + 2 * (2 + 3 * 1)]                              # a + l0 (i + n b)


PINNED = [j * 2.0 ** -52 for j in (887180520247730, 408896150279600, 2236591560848092, -1925309063778172)]     # seed 0, core 1, x = 0 .. 3


# ---- the two evaluations and the allowance -----------------------------------------------------------------------------------------
def _cases():
    out = [("fails_today",) + RS.case_fails_today() + (16, True)]
    for name, (coefs, names, L, exact) in RS.EDGE.items():
        out.append((name, coefs, [RS.edge_train(x) for x in names], L, exact))
    out.append(("d2", RS.D2[0], RS.d2_trains(), RS.D2[2], RS.D2[3]))
    for L in RS.DECAY_RANKS:
        out.append((f"decay_{L}",) + RS.decay_terms(RS.DECAY_SEED) + (L, False))
    return out


CASES = _cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_two_evaluations_agree_within_a_quarter_of_the_allowance(case):
    name, coefs, trains, L, exact = case
    a, b = RS.roundsum(coefs, trains, L, RS.SKETCH_SEED), RS.roundsum_mgs(coefs, trains, L, RS.SKETCH_SEED)
    allow = RS.allowance(coefs, trains, a, exact)
    da, db = RS.dense(a["cores"]), RS.dense(b["cores"])
    assert a["l"] == b["l"] == RS.ranks(a["cores"]) and np.isfinite(allow)
    diff = float(np.linalg.norm(da - db))
    print(name, "l", a["l"], "cond", RS.cond_max(a), "|a - b|", diff, "allowance", allow)
    assert diff <= 0.25 * allow
    if exact:
        S = RS.dense_sum(coefs, trains)
        assert np.linalg.norm(da - S) <= 0.25 * allow and np.linalg.norm(db - S) <= 0.25 * allow


@pytest.mark.parametrize("L", RS.DECAY_RANKS)
def test_truncation_cases_are_decided_and_the_reference_is_near_tt_svd(L):
    coefs, trains = RS.decay_terms(RS.DECAY_SEED)
    ref = RS.roundsum(coefs, trains, L, RS.SKETCH_SEED)
    S = RS.dense_sum(coefs, trains)
    allow = RS.allowance(coefs, trains, ref, False)
    err, best = float(np.linalg.norm(RS.dense(ref["cores"]) - S)), float(np.linalg.norm(RS.dense(RS.tt_svd(S, ref["l"])) - S))
    print("decay", L, "allowance / |S|", allow / np.linalg.norm(S), "cond", RS.cond_max(ref), "error / TT-SVD", err / best)
    assert allow <= 1e-9 * np.linalg.norm(S)
    assert best > 0.0 and err <= 10.0 * best


@pytest.mark.parametrize("name", RS.MULTI_TILE)
def test_multi_tile_cases_depend_on_every_tile_of_the_sketch(name):
    """The cases that truncate a sum of true rank 98 at l = 17, 40, 72 are there to see the 16-column tiles of W and of the new
    cores beyond the first.  They do: with the columns from 16 on of every W zeroed, or replaced by other numbers, the reference's
    own result moves by more than a thousand allowances.  The allowance is below 1e-7 of the norm of the sum, while a wrong tile
    moves the result at the scale of the truncation error, a tenth of the norm and more."""
    coefs, names, L, exact = RS.EDGE[name]
    trains = [RS.edge_train(x) for x in names]
    ref = RS.roundsum(coefs, trains, L, RS.SKETCH_SEED)
    S = RS.dense_sum(coefs, trains)
    allow = RS.allowance(coefs, trains, ref, exact)
    assert not exact and max(ref["l"]) == L > 16 and allow <= 1e-7 * np.linalg.norm(S)

    def zeroed(w):
        w = w.copy()
        w[:, 16:] = 0.0
        return w

    def other(w):
        w = w.copy()
        w[:, 16:] = np.cos(np.arange(w[:, 16:].size, dtype=np.float64)).reshape(w[:, 16:].shape)
        return w

    good = RS.dense(ref["cores"])
    for edit in (zeroed, other):
        moved = float(np.linalg.norm(RS.dense(RS.roundsum(coefs, trains, L, RS.SKETCH_SEED, w_edit=edit)["cores"]) - good))
        print(name, edit.__name__, "moves the result by", moved / allow, "allowances,", moved / np.linalg.norm(S), "of the norm")
        assert moved >= 1e3 * allow


def test_sketch_ranks_follow_the_rule():
    assert RS.sketch_ranks([4] * 6, [12, 144, 144, 144, 144, 144, 12], 16) == [1, 4, 16, 16, 16, 4, 1]
    assert RS.sketch_ranks(RS.EDGE_N, [5] + [89] * 6 + [5], 128) == [1, 7, 21, 89, 89, 14, 7, 1]
    assert RS.sketch_ranks(RS.EDGE_N, [3] + [143] * 6 + [3], 128) == [1, 7, 21, 98, 98, 14, 7, 1]
    assert RS.sketch_ranks([2, 1, 1, 50], [2, 9, 9, 9, 2], 128) == [1, 2, 2, 2, 1]      # the left-to-right cap
    assert RS.sketch_ranks([200, 200], [2, 300, 2], 128) == [1, 128, 1]
    for n, S, L in (([3, 5, 2, 7, 1, 4], [4, 6, 40, 41, 9, 9, 4], 17), ([2] * 12, [2] + [500] * 11 + [2], 128)):
        l = RS.sketch_ranks(n, S, L)
        assert all(l[k] <= l[k - 1] * n[k - 1] and l[k - 1] <= n[k - 1] * l[k] for k in range(1, len(n) + 1))


def test_a_long_train_overflows_without_the_power_of_two():
    coefs, trains = RS.long_train()
    n = [4] * len(trains[0])
    l = RS.sketch_ranks(n, RS.rank_sums(trains), 8)
    om = RS.omegas(RS.SKETCH_SEED, n, l)
    with np.errstate(over="ignore", invalid="ignore"):
        plain, scaled = RS._sketch_pass(trains, om, False), RS._sketch_pass(trains, om, True)
    assert not all(np.all(np.isfinite(w)) for w in plain[1])
    assert all(np.all(np.isfinite(w)) and np.any(w != 0.0) for ws in scaled[1:] for w in ws)
    assert all(0.5 <= max(np.max(np.abs(w)) for w in ws) < 1.0 for ws in scaled[1:-1])


# ---- the C-ABI surface --------------------------------------------------------------------------------------------------------------
def test_header_lines_and_symbols():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "ttx.h")).read())
    assert ("int ttx_lincomb_round(int32_t m, const double *coef, ttx_engine *const *x, int32_t rsketch, double tol, int32_t rmax, "
            "uint64_t seed, int32_t mode, ttx_engine **out);") in text
    assert ("int ttx_roundsum_last(const ttx_engine *h, double *ms /* [4]: sketch, gemm, qr, advance */, double *flops, "
            "int32_t *lsk /* [d+1] */, int32_t *mode_ran);") in text
    assert "int ttx_version(void) { return 3; }" in open(os.path.join(ROOT, "ttcross_amd", "csrc", "ttx_engine.hip")).read()
    if not os.path.exists(E.lib_path()):
        pytest.skip("libttx.so has not been built here")
    L = E.load_library()
    assert L.ttx_lincomb_round and L.ttx_roundsum_last and L.ttx_version() == 3


def test_refusals_come_before_any_device_call():
    if not os.path.exists(E.lib_path()):
        pytest.skip("libttx.so has not been built here")
    L = E.load_library()
    hs = (ctypes.c_void_p * 300)()
    cf = np.ones(300)
    out = ctypes.c_void_p(12345)
    nan = float("nan")
    for (m, rank, tol, rmax, mode), text in (((2, 129, -1.0, 0, 2), b"sketch rank 129"), ((2, -1, -1.0, 0, 2), b"sketch rank -1"), ((2, 16, -1.0, -1, 2), b"rmax"),
                                             ((2, 16, nan, 0, 2), b"not a number"), ((2, 16, -1.0, 0, 3), b"unknown mode 3"), ((2, 16, -1.0, 0, -1), b"unknown mode -1"),
                                             ((257, 16, -1.0, 0, 2), b"257 terms"), ((0, 16, -1.0, 0, 2), b"0 terms"), ((2, 16, -1.0, 0, 2), b"null engine")):
        out.value = 12345
        rc = L.ttx_lincomb_round(m, E._dp(cf), hs, rank, tol, rmax, 0, mode, ctypes.byref(out))
        assert rc == 1 and not out.value and text in L.ttx_last_error(), (m, rank, tol, rmax, mode, L.ttx_last_error())
    assert L.ttx_lincomb_round(2, None, hs, 16, -1.0, 0, 0, 2, ctypes.byref(out)) == 1 and b"null argument" in L.ttx_last_error()
    assert L.ttx_lincomb_round(2, E._dp(cf), hs, 16, -1.0, 0, 0, 2, None) == 1 and b"null argument" in L.ttx_last_error()
    assert L.ttx_roundsum_last(None, None, None, None, None) == 1
    with pytest.raises(ValueError):
        E.TTCross.lincomb_round([1.0], [], rank=4)
