"""GPU tests of pulled-back integrands (TTX_FUN_PULLBACK, ttcross_amd/csrc/ttx_pullback.h): fun(i) = h(x, logq, val) at the grid point
of i pulled back through resident squared-train transports.  The transport kernel does, with one wave per point, the operations of
ttx_sample_sq_real's exact mode with the same device functions, so points are compared BIT FOR BIT against the chain of public
sample_sq_real(.., mode="exact") calls on the layers' own engines (pullback_util.chain), and whole runs against the host-callback
engine walking a dense table of the same values (tests/pullback_ref.c)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pullback_grid_worker as W
import pullback_util as P
import trainfun_util as T
from conftest import ROOT
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

pytestmark = pytest.mark.gpu

ACC = 500 * D.EPS
GRID239 = [np.array([0.0, 1.0]), np.array([0.0, 0.375, 1.0]), P.unit_nodes(9, seed=1)]      # 2, 3 and 9 nodes with both ends


def _close(tt, layers):
    tt.close()
    for y in {id(y[0]): y[0] for y in layers}.values():
        y.close()


def _check_points(tt, layers, ref, ind):
    x, lq, v = tt.pullback_points(ind)
    rx, rlq, rv = P.chain(layers, P.ref_points(ref, ind))
    assert P.same_bits(x, rx) and P.same_bits(lq, rlq) and P.same_bits(v, rv)
    return x, lq, v


# ---- 1. the points -------------------------------------------------------------------------------------------------------------
# (name, layer mode sizes, layer ranks, gammas, reference grid)
POINTS = [
    # one layer: mode sizes 2, 5, 17, 65 (the lane stride and the search's rounds of 64 are crossed), ranks 1, 3, 17, 65 (two rows per lane above 64)
    ("m1_edges", [[65, 17, 5, 2]], [[1, 65, 17, 3, 1]], [0.0], [P.unit_nodes(9)] * 2 + GRID239[:2]),
    ("m2_gamma", [[65, 2, 17], [5, 65, 2]], [[1, 17, 65, 1], 3], [0.25, 0.0], GRID239),
    ("m3", [[5, 17, 9], [9, 4, 6], [3, 7, 5]], [3, [1, 5, 2, 1], 4], [0.0, 0.125, 0.5], GRID239[::-1]),
    ("d17", [[5] * 17, [5] * 17], [4, 4], [0.0, 0.0625], [P.unit_nodes(3)] * 17),
]


@pytest.mark.parametrize("name,ns,ranks,gammas,ref", POINTS, ids=[c[0] for c in POINTS])
def test_points_equal_the_chain_of_public_sampler_calls(name, ns, ranks, gammas, ref):
    layers = P.make_layers(E, ns, ranks, gammas, seed=len(name))
    n = [len(r) for r in ref]
    tt = E.TTCross.pullback(layers, ref, None, 2, pivoting=1)
    for npts in (1, 63, 64, 65, 1000):
        ind = P.random_indices(n, npts, seed=npts)
        x, lq, v = _check_points(tt, layers, ref, ind)
        last = tt.pullback_last()
        assert last["elements"] == npts and last["launches"] == 1 and last["failed"] == int(np.isnan(lq).sum())
    assert np.isfinite(x).all() and np.isfinite(lq).all()                       # random trains with these gammas do not fail
    # the ends 0 and 1 of the reference grid: the zero edge and the u >= 1 rule
    ind = np.array([[1] * len(n), n], dtype=np.int32)
    x, _, _ = _check_points(tt, layers, ref, ind)
    lo, hi = np.array([t[0] for t in layers[0][1]]), np.array([t[-1] for t in layers[0][1]])
    assert np.all(x >= lo) and np.all(x <= hi)
    _close(tt, layers)


def test_the_same_engine_as_layers_1_and_2():
    n = [5, 17, 4]
    y = E.TTCross.from_cores(T.random_cores(n, 3, seed=2))
    nodes = [P.unit_nodes(nk, seed=k) for k, nk in enumerate(n)]
    layers = [(y, nodes, 0.125), (y, [t.copy() for t in nodes], 0.125)]
    tt = E.TTCross.pullback(layers, GRID239, None, 2, pivoting=1)
    _check_points(tt, layers, GRID239, P.random_indices([2, 3, 9], 200, seed=1))
    # other nodes or another gamma for one engine: both layers would read one head -- refused, and the good set stays
    with pytest.raises(E.TTXError, match="layers 1 and 2 are one engine"):
        tt.set_integrand_pullback([(y, nodes, 0.125), (y, nodes, 0.25)], GRID239)
    _check_points(tt, layers, GRID239, P.random_indices([2, 3, 9], 20, seed=2))
    _close(tt, layers)


# ---- 2. independence -----------------------------------------------------------------------------------------------------------

def test_a_list_repeats_whatever_the_grid_the_order_and_the_call(tmp_path):
    layers, ref, ind = W.build(E, P)
    tt = E.TTCross.pullback(layers, ref, None, 2, pivoting=1)
    x, lq, v = _check_points(tt, layers, ref, ind)
    x2, lq2, v2 = tt.pullback_points(ind)                                       # twice
    assert P.same_bits(x, x2) and P.same_bits(lq, lq2) and P.same_bits(v, v2)
    xr, lqr, vr = tt.pullback_points(ind[::-1])                                 # in reverse order
    assert P.same_bits(x, xr[::-1]) and P.same_bits(lq, lqr[::-1]) and P.same_bits(v, vr[::-1])
    out = str(tmp_path / "grid1.npz")                                           # one workgroup strides over the whole list, in a fresh process
    env = dict(os.environ, TTX_PB_GRID="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pullback_grid_worker.py"), "grid", out], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0 and "pullback_grid_worker OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
    z = np.load(out)
    assert str(z["grid"]) == "1"
    assert P.same_bits(x, z["x"]) and P.same_bits(lq, z["lq"]) and P.same_bits(v, z["v"])
    _close(tt, layers)


# ---- 3. failed samples and NaN ---------------------------------------------------------------------------------------------------

def test_failed_samples_give_the_failed_row_and_are_counted():
    """A layer with a NaN core entry, and a layer of all zeros with gamma = 0, fail: x NaN, logq NaN, val 0.0, counted in failed.
    Through the list entry only.  The head pass of the sampler factors ALL indices of a mode together (a QR per mode), so a NaN in a
    core reaches every conditional of its layer: with this sampler there is no row of a list whose chain does not touch the NaN
    slice.  What stays comparable is checked instead: the rows equal the chain of public calls on the same layers, and a transport
    through the clean layers alone (the NaN layer taken out) equals the clean run's bits."""
    n = [5, 7, 4]
    ind = P.random_indices([2, 3, 9], 130, seed=5)
    clean = P.make_layers(E, [n, n], [3, 2], [0.0, 0.0], seed=9)
    tt = E.TTCross.pullback(clean, GRID239, None, 2, pivoting=1)
    x0, lq0, v0 = _check_points(tt, clean, GRID239, ind)
    assert tt.pullback_last()["failed"] == 0
    # a NaN entry in one slice of the inner layer's second core
    cores = T.random_cores(n, 2, seed=9 + 11)
    cores[1][0, 3, 1] = np.nan
    bad = E.TTCross.from_cores(cores)
    zero = E.TTCross.from_cores([np.zeros_like(c) for c in cores])
    for spoiled, at in ((bad, 1), (zero, 1), (zero, 0)):
        layers = list(clean)
        layers[at] = (spoiled, clean[at][1], 0.0)
        tt.set_integrand_pullback(layers, GRID239)
        x, lq, v = _check_points(tt, layers, GRID239, ind)
        assert np.isnan(x).all() and np.isnan(lq).all() and np.all(v == 0.0) and not np.any(np.signbit(v))
        assert tt.pullback_last() == dict(tt.pullback_last(), failed=130, elements=130)
    # the zero layer with gamma > 0 is the uniform: nothing fails
    layers = [clean[0], (zero, clean[1][1], 0.5)]
    tt.set_integrand_pullback(layers, GRID239)
    x, lq, v = _check_points(tt, layers, GRID239, ind)
    assert np.isfinite(x).all() and tt.pullback_last()["failed"] == 0
    # the clean layers again, after all that: the clean run's bits
    tt.set_integrand_pullback(clean, GRID239)
    x, lq, v = tt.pullback_points(ind)
    assert P.same_bits(x, x0) and P.same_bits(lq, lq0) and P.same_bits(v, v0)
    bad.close()
    zero.close()
    _close(tt, clean)


# ---- 4. the combiner -----------------------------------------------------------------------------------------------------------

def test_eval_device_is_the_example_combiner_on_the_pulled_back_points():
    """examples/devfun/pullback_tempered.hip uses exp, which is not an IEEE operation: the device library's and glibc's are each within
    one unit in the last place of the true value, their results differ by at most 2 ulp, relative 2 * 2^-52; the square root halves
    a relative difference and rounds once on each side (2^-53 each): 2 * 2^-52 in all, taken as 3 * 2^-52 because a relative bound of
    one ulp depends on where in the binade the value lies.  Everything before the exp is IEEE, in the same order on both sides.
    A failed row gives exactly 0.0."""
    layers = P.make_layers(E, [[9, 5, 17], [6, 7, 5]], [3, 4], [0.0, 0.25], seed=3, box=(-1.0, 1.8))
    ref = [P.unit_nodes(9)] * 3
    tt = E.TTCross.pullback(layers, ref, (P.tempered_object(), "pullback_tempered"), 2, pivoting=1, par=P.TEMPERED_PAR)
    ind = P.all_indices([9, 9, 9])
    got = tt.eval_device(ind)
    assert tt.pullback_last()["elements"] == 729
    x, lq, _ = tt.pullback_points(ind)
    want = P.tempered_host(x, lq)
    err = np.abs(got - want) / want
    print("pullback_tempered: largest relative difference device / host", err.max() / 2.0 ** -52, "x 2^-52")
    assert np.all(want > 0.0) and np.all(np.abs(got - want) <= 3 * 2.0 ** -52 * want)
    zero = E.TTCross.from_cores([np.zeros((1, 6, 1)), np.zeros((1, 7, 1)), np.zeros((1, 5, 1))])
    tt.set_integrand_pullback([layers[0], (zero, layers[1][1], 0.0)], ref, (P.tempered_object(), "pullback_tempered"), P.TEMPERED_PAR)
    got = tt.eval_device(ind[:70])
    assert np.all(got == 0.0) and tt.pullback_last()["failed"] == 70
    zero.close()
    _close(tt, layers)


# ---- 5. a whole run ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nproc", [1, 2])
@pytest.mark.parametrize("piv", [1, 3])
@pytest.mark.parametrize("d", [3, 4])
def test_runs_bit_exact_vs_the_host_callback_over_the_dense_table(d, piv, nproc):
    """tapes, sweep records, ranks, cores and integral of the TTX_FUN_PULLBACK engine = those of a TTX_FUN_HOST engine whose callback
    looks the value up in the table eval_device returned for all 9^d indices; no value crosses to the host during the device run."""
    n = [9] * d
    layers = P.make_layers(E, [[7] * d, [5] * d], [3, 2], [0.0, 0.125], seed=d, box=(-1.0, 1.8))
    ref, quad = [P.unit_nodes(9)] * d, T.box_quad(n)
    fun = (P.tempered_object(), "pullback_tempered")
    tt = E.TTCross.pullback(layers, ref, fun, 6, accuracy=ACC, pivoting=piv, quad=quad, nproc=nproc, par=P.TEMPERED_PAR)
    tab = np.ascontiguousarray(tt.eval_device(P.all_indices(n)))
    P.set_table(tab)
    tt.run()
    hh = E.TTCross(n, E.TTX_FUN_HOST, [], 6, pivoting=piv, accuracy=ACC, quad=quad, nproc=nproc)
    hh.set_integrand_host(P.lookup_addr(), [0.0]).run()
    T.same_run(tt, T.as_result(hh, d, quad), d, quad)
    assert tt.host_calls == 0 and tt.fun_id == E.TTX_FUN_PULLBACK
    last = tt.pullback_last()
    assert last["elements"] == hh.host_calls and last["launches"] > 0 and last["failed"] == 0
    hh.close()
    _close(tt, layers)


# ---- 6. state ------------------------------------------------------------------------------------------------------------------

def test_layers_are_looked_at_again_for_every_run():
    """run, round a layer so that its ranks drop, run again: the second run equals a fresh engine's on the layer as it is now; and
    the layer's own sampler and its way back return the same bits before and after the pullback engine's runs"""
    d, n = 3, [9] * 3
    layers = P.make_layers(E, [[7] * d, [5] * d], [4, 3], [0.0, 0.125], seed=6, box=(-1.0, 1.8))
    ref, quad = [P.unit_nodes(9)] * d, T.box_quad(n)
    fun = (P.tempered_object(), "pullback_tempered")
    u = np.random.default_rng(1).random((200, d))
    y, nodes, g = layers[0]
    before = y.sample_sq_real(u, nodes, gamma=g, mode="exact")
    back = y.rosenblatt_sq_real(before["x"], nodes, gamma=g, mode="exact")
    tt = E.TTCross.pullback(layers, ref, fun, 6, accuracy=ACC, pivoting=2, quad=quad, par=P.TEMPERED_PAR).run()
    first = T.as_result(tt, d, quad)
    after = y.sample_sq_real(u, nodes, gamma=g, mode="exact")
    back2 = y.rosenblatt_sq_real(before["x"], nodes, gamma=g, mode="exact")
    assert all(P.same_bits(before[k], after[k]) for k in before) and all(P.same_bits(back[k], back2[k]) for k in back)
    layers[1][0].svd(1e-3, 2)
    assert max(layers[1][0].ranks()) == 2
    tt.run()
    fresh = E.TTCross.pullback(layers, ref, fun, 6, accuracy=ACC, pivoting=2, quad=quad, par=P.TEMPERED_PAR).run()
    T.same_run(tt, T.as_result(fresh, d, quad), d, quad)
    assert not all(np.array_equal(a, b) for a, b in zip(first["cores"], T.as_result(tt, d, quad)["cores"]))
    _check_points(tt, layers, ref, P.random_indices(n, 100, seed=1))
    fresh.close()
    _close(tt, layers)


def test_calls_out_of_order_answer_estate():
    d = 3
    layers = P.make_layers(E, [[7] * d], [3], [0.0], seed=6)
    ref = [P.unit_nodes(9)] * d
    tt = E.TTCross([9] * d, E.TTX_FUN_PULLBACK, [], 4, pivoting=1)
    L = E.load_library()
    e4 = [ctypes.c_double() for _ in range(4)]
    for what in ("run", "eval", "points", "accchk"):
        with pytest.raises(E.TTXError, match="ttx_set_integrand_pullback") as ei:
            {"run": tt.run, "eval": lambda: tt.eval_device([[1, 1, 1]]), "points": lambda: tt.pullback_points([[1, 1, 1]]),
             "accchk": lambda: E._check(L.ttx_accchk(tt._h, 10, *[ctypes.byref(v) for v in e4], None))}[what]()
        assert ei.value.args and "first" in str(ei.value)
    tt.set_integrand_pullback(layers, ref)                                      # the layers only
    _check_points(tt, layers, ref, P.random_indices([9] * d, 30, seed=1))
    for call in (tt.run, lambda: tt.eval_device([[1, 1, 1]]), lambda: E._check(L.ttx_accchk(tt._h, 10, *[ctypes.byref(v) for v in e4], None))):
        with pytest.raises(E.TTXError, match="with a combiner first"):
            call()
    assert L.ttx_run(tt._h) == 4 and L.ttx_eval_device(tt._h, 0, None, None) == 4
    with pytest.raises(E.TTXError, match="one process"):
        tt.comm_init_shm("ttx_pullback_test")
    with pytest.raises(E.TTXError, match="outside 1..9"):
        tt.pullback_points([[1, 10, 1]])
    _close(tt, layers)


def test_refusals_leave_the_engine_as_it_was():
    L = E.load_library()
    d, n = 3, [7, 5, 6]
    layers = P.make_layers(E, [n, n], [3, 2], [0.0, 0.125], seed=2)
    ref = [P.unit_nodes(9)] * d
    ind = P.random_indices([9] * d, 50, seed=3)
    fun = (P.tempered_object(), "pullback_tempered")
    tt = E.TTCross.pullback(layers, ref, fun, 4, pivoting=1, par=P.TEMPERED_PAR)
    good = tt.eval_device(ind)
    (a, an, ag), (b, bn, bg) = layers

    def refused(ls, rf=ref, f=None, match="", par=None):
        with pytest.raises(E.TTXError, match=match) as ei:
            tt.set_integrand_pullback(ls, rf, f, par)
        assert "ttx_set_integrand_pullback" in str(ei.value)

    # an engine of another kind
    other_kind = E.TTCross([9] * d, E.TTX_FUN_TRAINS, [], 4, pivoting=1)
    with pytest.raises(E.TTXError, match="TTX_FUN_PULLBACK"):
        other_kind.set_integrand_pullback(layers, ref)
    with pytest.raises(E.TTXError, match="TTX_FUN_PULLBACK"):
        other_kind.pullback_points(ind)
    # m
    refused([], match="0 layers")
    refused([layers[0]] * 9, match=r"9 layers \(1\.\.8 expected\)")
    # a null layer, the engine itself, a layer without a train, with another d
    arr = (E._Layer * 2)()
    arr[0].x, arr[0].nodes, arr[0].gamma = a._h, ctypes.cast(a._node_rows(an, "t")[1], ctypes.POINTER(ctypes.POINTER(ctypes.c_double))), 0.0
    refp = tt._node_rows(ref, "t")[1]
    assert L.ttx_set_integrand_pullback(tt._h, 2, arr, refp, None, 0, None, None, 0) == 1 and b"layer 2 is null" in L.ttx_last_error()
    assert L.ttx_set_integrand_pullback(tt._h, 1, None, refp, None, 0, None, None, 0) == 1 and b"layer list missing" in L.ttx_last_error()
    assert L.ttx_set_integrand_pullback(tt._h, 1, arr, None, None, 0, None, None, 0) == 1 and b"reference rows missing" in L.ttx_last_error()
    arr[0].nodes = None
    assert L.ttx_set_integrand_pullback(tt._h, 1, arr, refp, None, 0, None, None, 0) == 1 and b"layer 1: node rows missing" in L.ttx_last_error()
    arr[0].x = tt._h
    assert L.ttx_set_integrand_pullback(tt._h, 1, arr, refp, None, 0, None, None, 0) == 1 and b"layer 1 is the engine itself" in L.ttx_last_error()
    refused([(other_kind, [P.unit_nodes(9)] * d, 0.0)], match="layer 1 holds no tensor train")
    short = E.TTCross.from_cores(T.random_cores([7, 5], 2, seed=1))
    arr[0].x, arr[0].nodes = short._h, ctypes.cast(a._node_rows(an, "t")[1], ctypes.POINTER(ctypes.POINTER(ctypes.c_double)))
    assert L.ttx_set_integrand_pullback(tt._h, 1, arr, refp, None, 0, None, None, 0) == 1 and b"layer 1 has 2 modes, the engine 3" in L.ttx_last_error()
    # a mode of one index
    one = E.TTCross.from_cores(T.random_cores([7, 1, 6], 2, seed=1))
    refused([(one, [an[0], np.array([0.5]), an[2]], 0.0)], match="layer 1: mode 2 has one index")
    # the node rows: not finite, not ascending, and for layers 2 and up the ends
    t = bn[1].copy(); t[2] = np.nan
    refused([layers[0], (b, [bn[0], t, bn[2]], bg)], match="layer 2, mode 2: the node row .*finite")
    t = an[2].copy(); t[1] = t[2]
    refused([(a, [an[0], an[1], t], ag)], match="layer 1, mode 3: the node row .*ascending")
    t = bn[0].copy(); t[0] = 1e-9
    refused([layers[0], (b, [t, bn[1], bn[2]], bg)], match="layer 2, mode 1: the node row ends at .*exactly 0 and 1")
    refused([layers[0], (b, an, bg)], match="layer 2, mode 1: the node row ends at")     # layer 1's box is no unit box
    # the reference grid
    r = P.unit_nodes(9); r[8] = np.nextafter(1.0, 2.0)
    refused(layers, rf=[ref[0], r, ref[2]], match="mode 2: the reference row entry 9")
    r = P.unit_nodes(9); r[0] = np.nan
    refused(layers, rf=[r, ref[1], ref[2]], match="mode 1: the reference row entry 1")
    # gamma
    refused([(a, an, -0.5)], match="layer 1: gamma is -0.5")
    refused([layers[0], (b, bn, float("inf"))], match="layer 2: gamma")
    # the combiner's refusals, after the layers' (a layer error comes before the code object is looked at)
    refused(layers, f=(T.comb_object(), "nosuch"), par=[0.0], match="no combiner 'nosuch'")
    refused(layers, f=(b"x" * 5000, "pullback_tempered"), match="neither a complete code object")
    refused([(a, an, -0.5)], f=(b"x" * 5000, "pullback_tempered"), match="layer 1: gamma")
    arr[0].x, arr[0].gamma = a._h, 0.0
    with pytest.raises(E.TTXError, match="par missing"):
        E._check(L.ttx_set_integrand_pullback(tt._h, 1, arr, refp, b"x" * 5000, 5000, b"pullback_tempered", None, 3))
    # a rank above 128 cannot be loaded at all; more LDS per wave than a workgroup has: with ranks up to 4 and d = 3 a wave needs
    # 2 n + 13 doubles, a workgroup has 19200: a layer mode of 9594 nodes and up
    with pytest.raises(E.TTXError):
        E.TTCross.from_cores(T.random_cores(n, [1, 129, 2, 1], seed=1))
    nbig = [9594, 2, 2]
    big = E.TTCross.from_cores(T.random_cores(nbig, 1, seed=1))
    refused([(big, [P.box_nodes(nk, 0.0, 1.0) for nk in nbig], 0.0)], match=r"one wave needs \d+ bytes of LDS")
    fits = E.TTCross.from_cores(T.random_cores([9593, 2, 2], 1, seed=1))
    tt.set_integrand_pullback([(fits, [P.box_nodes(nk, 0.0, 1.0) for nk in (9593, 2, 2)], 0.0)], ref)     # one wave per workgroup, all but 8 bytes of the budget
    _check_points(tt, [(fits, [P.box_nodes(nk, 0.0, 1.0) for nk in (9593, 2, 2)], 0.0)], ref, ind[:5])
    # the good set again: the engine gives the first set's values
    tt.set_integrand_pullback(layers, ref, fun, P.TEMPERED_PAR)
    refused([(a, an, -0.5)], match="gamma")
    assert P.same_bits(tt.eval_device(ind), good)
    for e in (other_kind, short, one, big, fits):
        e.close()
    _close(tt, layers)


# ---- 7. the helpers ------------------------------------------------------------------------------------------------------------

def test_transport_helpers_compose_the_layers_on_the_device(tmp_path):
    """transport_sample on a device tensor of the reference points = pullback_points at the same indices, bit for bit.
    transport_rosenblatt(layers, x) returns u close to the reference points: no bound is derived anywhere for a composition, so the
    distance allowed is measured on the same machine -- the largest per-layer round trip rosenblatt_sq_real(sample_sq_real(u)) of the
    same layers at the points the chain feeds them, times m, plus one unit roundoff for the sum
    (figures: profiles/pullback_mi355x.txt).  In a child process: torch initialises its device before the engine's library does."""
    out = str(tmp_path / "dev.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pullback_grid_worker.py"), "dev", out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "pullback_grid_worker OK" in p.stdout, (p.stdout + p.stderr)[-3000:]
    z = np.load(out)
    assert bool(z["is_cuda"])
    for a, b in (("xs", "x"), ("lqs", "lq"), ("vs", "v"), ("hx", "x"), ("hlq", "lq"), ("hv", "v")):
        assert P.same_bits(z[a], z[b]), (a, b)
    assert P.same_bits(z["vb"], z["v"])                                         # val of layer 1 at the same x
    m = 3
    dist = np.abs(z["ub"] - z["u"]).max()
    bound = z["per_layer"].max() * m + 2.0 ** -53
    print("transport_rosenblatt: per-layer round trips (m .. 1)", z["per_layer"].tolist(), "composed", dist, "allowed", bound)
    assert dist <= bound
