"""ttx_sample_real: what can be checked without a GPU -- the reference against itself (tests/sample_real_ref.py: verify(draw) on
every case, logq against log(val / Z), the draws of a 2-mode train against the dense interpolant's conditional CDFs), the C-ABI as
declared and exported, ttx_basis_host against the reference's hat row on the drawn points, engine.trapezoid_weights, and the
host-callable part of ttcross_amd/csrc/ttx_sample_real.h as a stand-alone program (tests/sample_real_main.cpp), plain and under
-fsanitize=address,undefined."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import sample_real_ref as SR
import sample_ref as S
from ttcross_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = SR.U
ALL = [(k, False) for k in SR.CASES] + [(k, True) for k in SR.SIGNED]
IDS = [k + ("_signed" if s else "") for k, s in ALL]
ENTRIES = ("ttx_sample_real", "ttx_sample_real_dev", "ttx_sample_real_last")


@functools.lru_cache(maxsize=None)
def _ref(name, signed=False):
    """(cores, u, nodes, the reference's draw) of a case: drawn once, shared, never modified"""
    cores, u, nodes = SR.case(name, signed)
    res = SR.draw(cores, nodes, u)
    for v in res:
        v.setflags(write=False)
    return cores, u, nodes, res


@pytest.mark.parametrize("name,signed", ALL, ids=IDS)
def test_the_reference_passes_its_own_check(name, signed):
    cores, u, nodes, (x, cell, logq, val, failed) = _ref(name, signed)
    assert not failed.any()
    chk = SR.verify(cores, nodes, u, None, x, cell)
    print(name, "N", chk["N"], "worst |CDF - T| / tol", chk["worst"])
    assert np.array_equal(chk["val"], val)
    assert np.all(np.abs(chk["logq"] - logq) <= chk["logq_bound"])
    for k, t in enumerate(nodes):                                      # a mode of one node is held: cell 0, x at the node
        if t.size == 1:
            assert np.all(cell[:, k] == 0) and np.all(x[:, k] == t[0])
        else:
            assert np.all((cell[:, k] >= 1) & (cell[:, k] <= t.size - 1)) and len(np.unique(x[:, k])) > SR.NPTS // 2


@pytest.mark.parametrize("name", list(SR.CASES))
def test_logq_is_log_of_val_over_z_on_trains_without_sign_changes(name):
    cores, u, nodes, (x, cell, logq, val, failed) = _ref(name)
    chk = SR.verify(cores, nodes, u, None, x, cell)
    bound = chk["logq_bound"] + 4.0 * chk["N"] * U
    rel = np.abs(np.exp(logq) * chk["Z"] - val) / val
    print(name, "max |exp(logq) Z - val| / val", float(rel.max()), "bound", float(bound.min()))
    assert np.all(val > 0.0) and np.all(rel <= bound)
    assert np.all(np.abs(logq - np.log(val / chk["Z"])) <= bound + 4.0 * U * (1.0 + np.abs(logq)))   # the division and the two logs on top


def test_draws_of_a_two_mode_train_invert_the_dense_interpolants_conditional_cdfs():
    """d2: mode 2 is drawn first from the marginal sum_i1 om_1(i1) T(i1, .), then mode 1 from the conditional sum_i2 T(., i2)
    phi_i2(x_2), both formed from the DENSE tensor.  Inverse-transform sampling means CDF(x_k) = u_k CDF(end) sample by sample, which
    pins the empirical CDF of the 2000 draws without a statistical threshold.  The tolerance is verify's with the dense sums."""
    cores, u, nodes, (x, cell, logq, val, failed) = _ref("d2")
    T = S.dense(cores)
    N = SR.count(cores)

    def cdf(p, t, xk):
        h = np.diff(t)
        A = 0.5 * (p[:-1] + p[1:]) * h
        C = np.concatenate([[0.0], np.cumsum(A)])
        j = min(max(int(np.searchsorted(t, xk, side="right")) - 1, 0), t.size - 2)
        lam = (xk - t[j]) / h[j]
        return C[j] + h[j] * (p[j] * lam + (p[j + 1] - p[j]) * 0.5 * lam * lam), C[-1], max(p[j], p[j + 1]) * h[j], max(p[j], p[j + 1])

    om1 = SR.trapezoid(nodes[0])
    worst = 0.0
    for s in range(SR.NPTS):
        for k, p in ((1, om1 @ T), (0, T @ SR.hat_row(nodes[1], x[s, 1]))):
            c, tot, ph, pm = cdf(p, nodes[k], x[s, k])
            tol = 6.0 * N * U * tot + 16.0 * U * ph + U * pm * np.abs(nodes[k]).max()
            worst = max(worst, abs(c - u[s, k] * tot) / tol)
    print("worst |CDF(x) - u CDF(end)| / tol", worst)
    assert worst <= 1.0
    assert np.all(np.abs(SR.dense_interpolant(cores, nodes, x) - val) <= 4.0 * N * U * val)


def test_held_modes_and_failures_of_the_reference():
    cores, u, nodes, base = _ref("d3")
    cond = [np.nan, float(nodes[1][2]), np.nan]                        # on a node
    x, cell, logq, val, failed = SR.draw(cores, nodes, u[:200], cond)
    assert np.all(x[:, 1] == cond[1]) and np.all(cell[:, 1] == 0) and not failed.any()
    SR.verify(cores, nodes, u[:200], cond, x, cell)
    held = [0.5 * (t[0] + t[1]) for t in nodes]                        # every mode held: val is the interpolant there, logq = 0
    x, cell, logq, val, failed = SR.draw(cores, nodes, u[:3], held)
    assert np.all(cell == 0) and np.all(logq == 0.0) and np.all(x == np.array(held)[None, :])
    assert np.all(np.abs(val - SR.dense_interpolant(cores, nodes, x)) <= 4.0 * SR.count(cores) * U * val)
    v = u[:8].copy()
    v[2, 1], v[5, 0] = np.nan, -0.25
    x, cell, logq, val, failed = SR.draw(cores, nodes, v)
    assert failed.tolist() == [False, False, True, False, False, True, False, False]
    assert np.all(np.isnan(x[failed])) and np.all(cell[failed] == 0) and np.all(np.isnan(logq[failed])) and np.all(val[failed] == 0.0)
    assert all(np.array_equal(a[~failed], b[:8][~failed]) for a, b in zip((x, cell, logq, val), base))
    zero = SR.draw([np.zeros_like(c) for c in cores], nodes, u[:5])
    assert zero[4].all() and np.all(np.isnan(zero[0]))


def _header():
    with open(os.path.join(ROOT, "include", "ttx.h")) as f:
        return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))


def test_header_declares_and_library_exports_the_entry_points():
    h = _header()
    for decl in ("int ttx_sample_real (ttx_engine *h, int64_t npts, const double *u , const double *const *nodes , const double *cond , double *x , int32_t *cell , double *logq, double *val);",
                 "int ttx_sample_real_dev(ttx_engine *h, int64_t npts, const double *u, const double *const *nodes, const double *cond, double *x, int32_t *cell, double *logq, double *val);",
                 "int ttx_sample_real_last(const ttx_engine *h, double *ms_head, double *bytes_head, double *ms_draw, int64_t *nfailed);"):
        assert decl in h, decl
    L = E.load_library()
    for name in ENTRIES:
        assert hasattr(L, name), name
    for name in ("sample_real", "sample_real_last"):
        assert callable(getattr(E.TTCross, name))


def test_basis_host_equals_the_references_hat_row_on_the_drawn_points():
    for name in ("d3", "long_modes"):
        cores, u, nodes, (x, cell, logq, val, failed) = _ref(name)
        for k, t in enumerate(nodes):
            pts = np.concatenate([x[:300, k], t, [t[0] - 1.0, t[-1] + 1.0]])
            phi = E.basis_table(("linear", t), t.size, pts)
            i, f0, f1 = SR.hat(t, pts)
            want = np.zeros_like(phi)
            want[np.arange(pts.size), i] = f0
            want[np.arange(pts.size), i + 1] += f1
            assert np.array_equal(phi, want), (name, k)


def test_trapezoid_weights():
    rng = np.random.default_rng(3)
    t = np.cumsum(rng.uniform(0.1, 1.0, 17)) - 4.0
    om = E.trapezoid_weights(t)
    assert np.array_equal(om, SR.trapezoid(t)) and abs(om.sum() - (t[-1] - t[0])) <= 17 * U * np.abs(t).max()
    assert om[0] == 0.5 * (t[1] - t[0]) and om[-1] == 0.5 * (t[-1] - t[-2]) and om[5] == 0.5 * (t[6] - t[4])
    both = E.trapezoid_weights([t, np.array([2.5])])
    assert isinstance(both, list) and np.array_equal(both[0], om) and both[1].tolist() == [1.0]
    with pytest.raises(ValueError):
        E.trapezoid_weights(np.zeros((2, 2)))


def _build(tmp_path, name, extra):
    exe = tmp_path / name
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "ttcross_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sample_real_main.cpp"), "-o", str(exe)], check=True)
    return exe


def _check(out):
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    bad, ninv, nchk = (int(v) for v in out.stdout.strip().splitlines()[-1].split())
    assert bad == 0 and ninv > 200000 and nchk > 2 * ninv


def test_inversion_and_weights_as_a_host_program(tmp_path):
    _check(subprocess.run([str(_build(tmp_path, "sample_real", []))], capture_output=True, text=True))


def test_inversion_and_weights_under_address_and_undefined_sanitizers(tmp_path):
    exe = _build(tmp_path, "sample_real_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    _check(subprocess.run([str(exe)], capture_output=True, text=True, env=env))


@pytest.mark.parametrize("method, entry, extra", [("sample_real", "ttx_sample_real", ()), ("sample_sq_real", "ttx_sample_sq_real", (0.125, "exact"))])
def test_node_rows_made_for_the_call_live_through_it(monkeypatch, method, entry, extra):
    """Nodes given as lists (or float32, or a strided view) become new float64 arrays whose addresses go to the C entry in a ctypes
    pointer array, and a ctypes array holds addresses only.  The entry, a stand-in here, must find every such array alive and its
    numbers in place; once the call is over they are released."""
    import gc
    import types
    import weakref
    nodes = [[0.0, 0.25, 1.0], np.array([0.0, 2.0], dtype=np.float32), np.linspace(0.0, 3.0, 7)[::2]]
    refs, seen = [], []
    rows_of = E.TTCross._node_rows

    def spy(self, nd, who):
        rows, rowp = rows_of(self, nd, who)
        refs.extend(weakref.ref(r) for r in rows)
        return rows, rowp

    def stand_in(h, npts, u, rowp, cond, *rest):
        gc.collect()
        seen.append([r() is not None for r in refs])
        seen.append([[rowp[k][j] for j in range(len(nodes[k]))] for k in range(3)])
        return 0

    monkeypatch.setattr(E.TTCross, "_node_rows", spy)
    monkeypatch.setattr(E, "load_library", lambda: types.SimpleNamespace(**{entry: stand_in, entry + "_dev": stand_in}))
    tt = object.__new__(E.TTCross)
    tt.d, tt._n, tt._h = 3, [3, 2, 4], None
    out = getattr(tt, method)(np.full((2, 3), 0.5), nodes, None, *extra)
    assert seen[0] == [True] * 3 and seen[1] == [[0.0, 0.25, 1.0], [0.0, 2.0], [0.0, 1.0, 2.0, 3.0]]
    assert sorted(out) == ["cell", "logq", "val", "x"] and out["x"].shape == (2, 3)
    gc.collect()
    assert [r() for r in refs] == [None] * 3
