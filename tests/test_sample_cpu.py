"""The sampling reference (tests/sample_ref.py) against dense tensors, without a GPU: exp(logq) is the dense density at the drawn
index (an identity, not a statistic), every cell with positive density is reached and no cell with zero density is, fixed modes
give the dense conditional density, and the reference alone meets the cap on undecided samples for the cases the GPU tests use."""
import itertools

import numpy as np
import pytest

import sample_ref as S

SMALL = {
    "d3": ([3, 4, 2], [1, 2, 3, 1]),
    "d4_mode_of_size_1": ([3, 1, 4, 2], [1, 2, 2, 3, 1]),
}


def _train(name, seed=0):
    n, r = SMALL[name]
    rng = np.random.default_rng(sum(map(ord, name)) + seed)
    return [rng.uniform(0.0, 1.0, (r[k], n[k], r[k + 1])) for k in range(len(n))], [rng.uniform(0.5, 1.5, nk) for nk in n]


def _grid(n, m):
    """a fine grid of u: m midpoints per mode"""
    g = (np.arange(m) + 0.5) / m
    return np.array(list(itertools.product(*[g] * len(n))))


@pytest.mark.parametrize("name", sorted(SMALL))
def test_exp_logq_is_the_dense_density_at_the_drawn_index(name):
    cores, w = _train(name)
    u = np.random.default_rng(1).random((500, len(cores)))
    ind, logq, val, failed = S.draw(cores, u, w)
    assert not failed.any()
    rho = S.dense_density(cores, w)
    want = rho[tuple((ind - 1).T)]
    assert np.all(np.abs(np.exp(logq) - want) <= 1e-12 * want)
    assert np.all(np.abs(val - S.dense(cores)[tuple((ind - 1).T)]) <= 1e-12 * np.abs(val))


@pytest.mark.parametrize("name", sorted(SMALL))
def test_every_positive_cell_is_reached_and_no_zero_cell(name):
    cores, w = _train(name)
    cores[0][:, 0, :] = 0.0                                            # a slab of zero density
    n = [c.shape[1] for c in cores]
    rho = S.dense_density(cores, w)
    assert np.all(rho[0] == 0.0) and np.all(rho[1:] > 0.0)
    ind, logq, _, failed = S.draw(cores, _grid(n, 24 if len(n) == 3 else 12), w)
    assert not failed.any()
    seen = np.zeros(rho.shape, bool)
    seen[tuple((ind - 1).T)] = True
    assert np.array_equal(seen, rho > 0.0)


def test_fixed_modes_give_the_dense_conditional_density():
    cores, w = _train("d3", 5)
    fixed = [0, 3, 0]
    u = np.random.default_rng(2).random((400, 3))
    ind, logq, _, failed = S.draw(cores, u, w, fixed)
    assert not failed.any() and np.all(ind[:, 1] == 3)
    rho = S.dense_density(cores, w, fixed)
    want = rho[ind[:, 0] - 1, 0, ind[:, 2] - 1]
    assert np.all(np.abs(np.exp(logq) - want) <= 1e-12 * want)
    w2 = [w[0], 7.0 * w[1], w[2]]                                      # the weight of a fixed mode does not enter
    assert np.array_equal(S.draw(cores, u, w2, fixed)[1], logq)


def test_edges_of_u_and_failed_samples():
    cores, w = _train("d3")
    n = [c.shape[1] for c in cores]
    u = np.random.default_rng(3).random((6, 3))
    u[0], u[1], u[2] = 0.0, np.nextafter(1.0, 0.0), 1.0
    u[3, 1], u[4, 2] = np.nan, -0.5
    ind, logq, val, failed = S.draw(cores, u, w)
    assert failed.tolist() == [False, False, False, True, True, False]
    assert ind[0].tolist() == [1, 1, 1] and ind[1].tolist() == n and ind[2].tolist() == n
    assert np.all(ind[3:5] == 0) and np.all(np.isnan(logq[3:5])) and np.all(val[3:5] == 0.0)
    zero = [np.zeros_like(c) for c in cores]
    assert S.draw(zero, u, w)[3].all()


@pytest.mark.parametrize("name,signed", [(k, False) for k in S.CASES] + [(k, True) for k in S.SIGNED])
def test_the_reference_alone_meets_the_cap_on_the_gpu_tests_cases(name, signed):
    """at most 0.1 % of a test's samples may be undecided: here with draw's own indices, for exactly the (cores, u) of test_gpu_sample.py"""
    cores, u, w = S.case(name, signed)
    ind, logq, _, failed = S.draw(cores, u, w)
    assert not failed.any()
    res = S.verify(cores, u, w, None, ind)
    print(name, "signed" if signed else "non-negative", "N", res["N"], "undecided", res["undecided"], "of", S.NPTS)
    assert res["undecided"] <= S.NPTS // 1000
    assert np.array_equal(res["logq"], logq)
