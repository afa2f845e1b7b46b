"""GPU tests of integrands of resident trains (TTX_FUN_TRAINS, ttcross_amd/csrc/ttx_trainfun.h): fun(i) = g(x_1(i), .., x_m(i)).
The slot kernel evaluates every operand with the chain of ttx_ijk_batch's exact mode and the combiners are single IEEE operations,
so everything is compared BIT FOR BIT: elements against tijk_batch and the host twin (tests/trainfun_ref.c), whole runs against the
host-callback engine and the oracle, both calling the twin."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import trainfun_util as T
from conftest import ROOT
from ttcross_amd import drivers as D
from ttcross_amd import engine as E

pytestmark = pytest.mark.gpu

ACC = 500 * D.EPS
EDGE_N, EDGE_R = [3, 5, 2, 7, 4, 6, 3, 5], [1, 3, 17, 64, 65, 9, 128, 2, 1]   # 64 / 65: two rows per lane; 128: the cap


def _apply(op, v, ind=None, par=None):
    if op == "product":
        p = v[0]
        for t in range(1, len(v)):
            p = p * v[t]
        return p
    if op == "ratio":
        return v[0] / v[1]
    if op == "sqrtabs":
        return np.sqrt(np.abs(v[0]))
    return v[0] / (1.0 + v[1] * v[1]) + par[0] * ind[:, 0]


def _engine(ops, op, maxrank, par=None, **kw):
    if op == "comb_rational":
        return E.TTCross.of_trains(ops, None, maxrank, combiner=(T.comb_object(), "comb_rational"), par=par, **kw)
    return E.TTCross.of_trains(ops, op, maxrank, **kw)


def _close(*es):
    for e in es:
        e.close()


# ---- elements ------------------------------------------------------------------------------------------------------------------

ELEMENTS = [
    ("d2", [5, 4], [[1, 3, 1]], "sqrtabs", False),
    ("d2_ratio", [5, 4], [[1, 3, 1], [1, 2, 1]], "ratio", True),
    ("d3_m3", [3, 9, 2], [2, 3, 2], "product", False),
    ("d3_m8", [3, 9, 2], [2, 1, 3, 2, 2, 3, 1, 2], "product", False),
    ("rank1", [4, 3, 5, 2], [1, 1], "product", False),
    ("edge_64_65_128", EDGE_N, [EDGE_R], "product", False),
    ("edge_unlike_ranks", EDGE_N, [EDGE_R, 2], "product", False),
    ("edge_comb", EDGE_N, [EDGE_R, 3], "comb_rational", False),
    ("d300", [5] * 300, [2, 2], "ratio", True),
]


@pytest.mark.parametrize("name,n,ranks,op,positive", ELEMENTS, ids=[e[0] for e in ELEMENTS])
def test_elements_equal_tijk_batch_and_the_twin(name, n, ranks, op, positive):
    """eval_device of a TTX_FUN_TRAINS engine = the op applied to tijk_batch(x_t, ind, "exact") = the host twin, as bytes"""
    cores = [T.random_cores(n, r, seed=100 + t, positive=positive) for t, r in enumerate(ranks)]
    ops = [E.TTCross.from_cores(c) for c in cores]
    ind = T.random_indices(n, 300, seed=len(n))
    par = [0.125]
    tt = _engine(ops, op, 2, par=par, pivoting=1)
    got = tt.eval_device(ind)
    vals = [x.tijk_batch(ind, "exact") for x in ops]
    T.twin_set(cores)
    for t, v in enumerate(vals):
        assert v.tobytes() == T.twin_element(t, ind).tobytes(), t
    assert got.tobytes() == _apply(op, vals, ind, par).tobytes()
    assert got.tobytes() == T.twin_eval(op, n, ind, par).tobytes()
    last = tt.trainfun_last()
    assert last["elements"] == ind.shape[0] and last["launches"] == 1
    _close(tt, *ops)


def test_the_same_train_given_twice():
    cores = T.random_cores([3, 9, 2], 3, seed=5)
    x = E.TTCross.from_cores(cores)
    ind = T.random_indices([3, 9, 2], 300, seed=1)
    tt = E.TTCross.of_trains([x, x], "product", 2, pivoting=1)
    v = x.tijk_batch(ind, "exact")
    assert tt.eval_device(ind).tobytes() == (v * v).tobytes()
    # more points than the 8192 waves of the capped grid: the list kernel strides
    ind = T.random_indices([3, 9, 2], 9001, seed=2)
    v = x.tijk_batch(ind, "exact")
    assert tt.eval_device(ind).tobytes() == (v * v).tobytes()
    assert tt.trainfun_last()["elements"] == 9001
    _close(tt, x)


def test_eval_device_refuses_an_index_outside_the_modes():
    x = E.TTCross.from_cores(T.random_cores([5, 5, 5], 2, seed=1))
    tt = E.TTCross.of_trains([x], "sqrtabs", 2, pivoting=1)
    with pytest.raises(E.TTXError, match="outside 1..5"):
        tt.eval_device([[1, 6, 1]])
    with pytest.raises(E.TTXError, match="outside 1..5"):
        tt.eval_device([[0, 1, 1]])
    _close(tt, x)


# ---- whole runs ----------------------------------------------------------------------------------------------------------------
# (n, maxrank, piv, groups, op, operand ranks, positive)
RUNS = [
    ("d5_product", [17] * 5, 10, 2, 1, "product", [4, 3], False),
    ("d6_ratio_g3", [13] * 6, 8, 1, 3, "ratio", [3, 2], True),
    ("d4_sqrtabs_lottery", [9] * 4, 6, 0, 1, "sqrtabs", [3], False),
    ("d4_product3_fullpiv", [7] * 4, 5, -1, 1, "product", [2, 2, 2], False),
    ("d5_comb_fullpiv_g2", [5] * 5, 4, -1, 2, "comb_rational", [2, 3], False),
    ("unequal_modes_g2", [9, 5, 11, 7, 6], 6, 2, 2, "product", [3, 2], False),
    # 3 * 64 * 65 = 12480 slots, more than the 8192 waves of the capped grid: a wave's ballot holds several slots (the second and
    # third group's runs lie behind slot 8192) and the kernel strides
    ("more_slots_than_waves_g3", [65] * 4, 64, 2, 3, "product", [3, 2], False),
]


def _three_ways(n, r, piv, nproc, op, cores, ops, par=(0.125,)):
    d, quad, par = len(n), T.box_quad(n), list(par)
    tt = _engine(ops, op, r, par=par, accuracy=ACC, pivoting=piv, quad=quad, nproc=nproc).run()
    T.twin_set(cores)
    addr = T.twin_addr(op)
    oo = O.dmrgg(n, 4, par, r, piv=piv, accuracy=ACC, quad=quad, nproc=nproc, user=addr)
    T.same_run(tt, oo, d, quad)
    hh = E.TTCross(n, E.TTX_FUN_HOST, [], r, pivoting=piv, accuracy=ACC, quad=quad, nproc=nproc)
    hh.set_integrand_host(addr, par).run()
    T.same_run(tt, T.as_result(hh, d, quad), d, quad)
    assert tt.host_calls == 0 and tt.fun_id == E.TTX_FUN_TRAINS
    last = tt.trainfun_last()
    assert last["elements"] == hh.host_calls and last["launches"] > 0
    return tt, hh


@pytest.mark.parametrize("name,n,r,piv,nproc,op,ranks,positive", RUNS, ids=[c[0] for c in RUNS])
def test_runs_bit_exact_vs_host_callback_and_oracle(name, n, r, piv, nproc, op, ranks, positive):
    """tapes, sweep records, every core and the integral: the engine on trains = the host-callback engine with the twin = the oracle
    with the twin.  Rook, lottery-only and full pivoting, one to three bond groups, unequal modes, every combiner."""
    cores = [T.random_cores(n, rk, seed=200 + 7 * t + len(n), positive=positive) for t, rk in enumerate(ranks)]
    ops = [E.TTCross.from_cores(c) for c in cores]
    tt, hh = _three_ways(n, r, piv, nproc, op, cores, ops)
    _close(tt, hh, *ops)


def test_run_on_the_result_train_of_an_ising_run():
    """an operand that comes from a sweep (Ising C_6, n = 17, its own layout: maxrank 6) times a loaded random train"""
    s = D.ising_setup("c", 6, 17)
    x = E.TTCross(s["n"], s["fun_id"], s["par"], 6, pivoting=2, accuracy=s["acc"], quad=s["quad"]).run()
    yc = T.random_cores(s["n"], 3, seed=9)
    y = E.TTCross.from_cores(yc)
    tt, hh = _three_ways(list(s["n"]), 10, 2, 1, "product", [T.cores_of(x), yc], [x, y])
    _close(tt, hh, x, y)


def test_accchk_equals_the_host_callback_engine():
    n = [17] * 5
    cores = [T.random_cores(n, 4, seed=1), T.random_cores(n, 3, seed=2)]
    ops = [E.TTCross.from_cores(c) for c in cores]
    tt, hh = _three_ways(n, 10, 2, 1, "product", cores, ops)
    a, b = tt.accchk(3000), hh.accchk(3000)
    for k in ("einf", "efro", "ainf", "afro"):
        assert a[k] == b[k], k
    assert np.array_equal(a["pivot"], b["pivot"])
    _close(tt, hh, *ops)


def test_operand_blocks_are_rebuilt_for_every_run():
    """run, round an operand so that its ranks drop, run again: the second run is the twin's on the operand's NEW cores"""
    n = [9] * 5
    cores = [T.random_cores(n, 5, seed=3), T.random_cores(n, 2, seed=4)]
    ops = [E.TTCross.from_cores(c) for c in cores]
    tt, hh = _three_ways(n, 8, 2, 1, "product", cores, ops)
    first = T.as_result(tt, 5, T.box_quad(n))
    ops[0].svd(1e-3, 3)
    assert max(ops[0].ranks()) == 3
    new = [T.cores_of(ops[0]), cores[1]]
    tt.run()
    T.twin_set(new)
    hh.run()
    T.same_run(tt, T.as_result(hh, 5, T.box_quad(n)), 5, T.box_quad(n))
    assert not all(np.array_equal(a, b) for a, b in zip(first["cores"], T.as_result(tt, 5, T.box_quad(n))["cores"]))
    ind = T.random_indices(n, 200, seed=2)
    assert tt.eval_device(ind).tobytes() == (ops[0].tijk_batch(ind, "exact") * ops[1].tijk_batch(ind, "exact")).tobytes()
    _close(tt, hh, *ops)


def test_the_square_that_hadamard_refuses():
    """rank 12: x.hadamard(x) would need rank 144 > 128 and is refused; the cross run on [x, x] works and is the oracle's bit for
    bit.  Rank 4: the distance between the cross result and x.hadamard(x), relative to its norm, is printed, not asserted -- the GPU
    result is the oracle's, whose error is a property of the method (profiles/trainfun_mi355x.txt)."""
    n = [13] * 4
    cores = T.random_cores(n, 12, seed=6)
    x = E.TTCross.from_cores(cores)
    with pytest.raises(E.TTXError, match="144"):
        x.hadamard(x)
    tt, hh = _three_ways(n, 16, 2, 1, "product", [cores, cores], [x, x])
    _close(tt, hh, x)
    c4 = T.random_cores(n, 4, seed=7)
    y = E.TTCross.from_cores(c4)
    tt, hh = _three_ways(n, 16, 2, 1, "product", [c4, c4], [y, y])
    z = y.hadamard(y)
    print("rank 4 square: ranks", tt.ranks().tolist(), "dist(cross, hadamard) / norm(hadamard) =", tt.dist(z) / z.norm())
    _close(tt, hh, y, z)


def test_repetition_and_fast_arithmetic_give_identical_bytes(monkeypatch):
    n = [9] * 4
    cores = [T.random_cores(n, 3, seed=1, positive=True), T.random_cores(n, 2, seed=2, positive=True)]
    ops = [E.TTCross.from_cores(c) for c in cores]
    quad = T.box_quad(n)
    tt = E.TTCross.of_trains(ops, "ratio", 6, accuracy=ACC, pivoting=2, quad=quad).run()
    a = T.as_result(tt, 4, quad)
    T.same_run(tt.run(), a, 4, quad)
    monkeypatch.setenv("TTX_ARITH", "fast")
    ff = E.TTCross.of_trains(ops, "ratio", 6, accuracy=ACC, pivoting=2, quad=quad).run()
    assert ff.arith == "exact"
    T.same_run(ff, a, 4, quad)
    _close(tt, ff, *ops)


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_engine_usable():
    L = E.load_library()
    n = [9] * 4
    cores = [T.random_cores(n, 3, seed=1), T.random_cores(n, 2, seed=2)]
    x, y = (E.TTCross.from_cores(c) for c in cores)
    other = E.TTCross.from_cores(T.random_cores([9, 9, 8, 9], 2, seed=3))
    short = E.TTCross.from_cores(T.random_cores([9] * 3, 2, seed=3))
    quad = T.box_quad(n)

    def rc_msg(rc):
        return rc, L.ttx_last_error().decode()

    def hs(*es):
        return (ctypes.c_void_p * len(es))(*[e._h if e is not None else None for e in es])

    # an engine of another kind
    s = D.ising_setup("c", 5, 9)
    ii = E.TTCross(s["n"], s["fun_id"], s["par"], 4, pivoting=1)
    rc, msg = rc_msg(L.ttx_set_integrand_trains(ii._h, 1, hs(x), E.TTX_TOP_SQRTABS))
    assert rc == 4 and "TTX_FUN_TRAINS" in msg
    ii.close()

    tt = E.TTCross(n, E.TTX_FUN_TRAINS, [], 6, pivoting=2, accuracy=ACC, quad=quad)
    # nothing set yet
    with pytest.raises(E.TTXError, match="ttx_set_integrand_trains first"):
        tt.run()
    with pytest.raises(E.TTXError, match="ttx_set_integrand_trains first"):
        tt.eval_device([[1, 1, 1, 1]])
    e4 = [ctypes.c_double() for _ in range(4)]
    rc, msg = rc_msg(L.ttx_accchk(tt._h, 10, *[ctypes.byref(v) for v in e4], None))
    assert rc == 4 and "ttx_set_integrand_trains first" in msg
    # several processes are out of scope
    with pytest.raises(E.TTXError, match="one process"):
        tt.comm_init_shm("ttx_trainfun_test")
    buf = (ctypes.c_uint8 * 128)()
    rc, msg = rc_msg(L.ttx_comm_init(tt._h, buf))
    assert rc == 4 and "one process" in msg
    cb = (E._SENDRECV(lambda *a: 0), E._ALLREDUCE(lambda *a: 0))
    tr = E._Transport(None, cb[0], cb[1])
    rc, msg = rc_msg(L.ttx_set_transport(tt._h, ctypes.byref(tr)))
    assert rc == 4 and "ttx_set_transport" in msg and "one process" in msg
    # the loaded combiner has its own entry
    rc, msg = rc_msg(L.ttx_set_integrand_trains(tt._h, 2, hs(x, y), E.TTX_TOP_DEVICE))
    assert rc == 1 and "ttx_set_integrand_trains_device" in msg
    # m and op
    for m, op in ((0, 1), (9, 1), (1, 2), (2, 3), (3, 2), (2, 0), (2, 5), (2, 4)):
        rc, msg = rc_msg(L.ttx_set_integrand_trains(tt._h, m, hs(*([x] * max(m, 1))), op))
        assert rc == 1, (m, op, msg)
    # operands: null, without a train, other modes, other d, the engine itself
    rc, msg = rc_msg(L.ttx_set_integrand_trains(tt._h, 2, hs(x, None), 1))
    assert rc == 1 and "operand 2" in msg
    empty = E.TTCross(n, E.TTX_FUN_TRAINS, [], 4, pivoting=1)
    rc, msg = rc_msg(L.ttx_set_integrand_trains(tt._h, 2, hs(x, empty), 1))
    assert rc == 4 and "operand 2" in msg and "no tensor train" in msg
    rc, msg = rc_msg(L.ttx_set_integrand_trains(tt._h, 3, hs(x, y, other), 1))
    assert rc == 1 and "operand 3" in msg and "mode 3" in msg
    rc, msg = rc_msg(L.ttx_set_integrand_trains(tt._h, 1, hs(short), 3))
    assert rc == 1 and "operand 1" in msg
    rc, msg = rc_msg(L.ttx_set_integrand_trains(tt._h, 2, hs(x, tt), 1))
    assert rc == 1 and "operand 2" in msg and "itself" in msg
    # a code object without the combiner symbols, and one that is no code object
    import devfun_util as U
    with pytest.raises(E.TTXError, match="no combiner 'rational'"):
        tt.set_integrand_trains([x, y], (U.code_object("rational"), "rational"), [0.125])
    with pytest.raises(E.TTXError, match="no combiner 'nosuch'"):
        tt.set_integrand_trains([x, y], (T.comb_object(), "nosuch"), [0.125])
    with pytest.raises(E.TTXError, match="neither a complete code object"):
        tt.set_integrand_trains([x, y], (b"x" * 5000, "comb_rational"), [0.125])
    # an operand error comes before the code object is looked at
    with pytest.raises(E.TTXError, match="operand 2.*mode 3"):
        tt.set_integrand_trains([x, other], (b"x" * 5000, "comb_rational"), [0.125])
    # still nothing set, and still usable: a valid run gives the reference bits
    with pytest.raises(E.TTXError, match="ttx_set_integrand_trains first"):
        tt.run()
    tt.set_integrand_trains([x, y], "product").run()
    T.twin_set(cores)
    oo = O.dmrgg(n, 4, [0.0], 6, piv=2, accuracy=ACC, quad=quad, user=T.twin_addr("product"))
    T.same_run(tt, oo, 4, quad)
    # a refusal after a good set keeps the good one
    rc, msg = rc_msg(L.ttx_set_integrand_trains(tt._h, 2, hs(x, other), 1))
    assert rc == 1
    T.same_run(tt.run(), oo, 4, quad)
    _close(tt, empty, x, y, other, short)


# ---- non-finite values ---------------------------------------------------------------------------------------------------------

def test_ratio_with_exact_zeros_ends_like_the_host_callback():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "trainfun_nan_worker.py"), "2", "1"], capture_output=True, text=True, timeout=300)
    blob = p.stdout + p.stderr
    assert "Memory access fault" not in blob and "core dump" not in blob.lower(), blob[-3000:]
    assert p.returncode == 0 and " OK" in p.stdout, blob[-3000:]


# ---- accchk leaves the figures of the last run ------------------------------------------------------------------------------

def test_accchk_leaves_the_figures_of_the_last_run():
    n = [9] * 4
    ops = [E.TTCross.from_cores(T.random_cores(n, 3, seed=1)), E.TTCross.from_cores(T.random_cores(n, 2, seed=2))]
    tt = E.TTCross.of_trains(ops, "product", 6, accuracy=ACC, pivoting=2, quad=T.box_quad(n)).run()
    a = tt.trainfun_last()
    tt.accchk(500)
    assert tt.trainfun_last() == a and a["elements"] > 0
    _close(tt, *ops)


# ---- Fortran -------------------------------------------------------------------------------------------------------------------

def test_fortran_dtt_dmrgg_trains():
    """the drop-in dmrgg_lib: dtt_dmrgg_trains(z, [x, x], TTX_TOP_PRODUCT).  Rank-1 operand with entries +-2^e: every operation of
    the sweep is exact, the elements of the result are those of tijk(x)**2 digit for digit and the ranks are x's.  Rank-2 operand:
    x*x has rank 3 on every bond; elements to 1e-12 of the element scale, the tolerance of the Fortran algebra and contract tests."""
    from conftest import fortran_exe
    exe = fortran_exe("test_tt_compose")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and p.stdout.strip().endswith("done"), p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.split()]
    ranks = {ln[1]: [int(v) for v in ln[2:]] for ln in lines if ln[0] == "ranks"}
    assert ranks == {"rank1": [1, 1, 1, 1, 1], "rank2": [1, 3, 3, 3, 1]}, ranks
    el = {c: [ln[3:] for ln in lines if ln[0] == "elem" and ln[1] == c] for c in ("rank1", "rank2")}
    assert len(el["rank1"]) == 30 and len(el["rank2"]) == 30
    assert all(a == b for a, b in el["rank1"]), el["rank1"]
    assert len({b for _, b in el["rank1"]}) > 5
    v = np.array([[float(a), float(b)] for a, b in el["rank2"]])
    scale = np.abs(v[:, 1]).max()
    assert scale > 0.1 and np.all(np.abs(v[:, 0] - v[:, 1]) <= 1e-12 * scale)
