"""Host-side mirror of the reference's command-line drivers (test_crs_ising.f90, test_crs_stdnorm.f90,
test_crs_mvn.f90): same positional arguments, same parameter set-up, same report lines; the sweep itself
runs on the GPU through ttcross_amd.engine.  Usage:

    python -m ttcross_amd.drivers ising KIND INDEX N RANK PIV [NGROUPS]
    python -m ttcross_amd.drivers stdnorm D N RANK PIV [NGROUPS]
    python -m ttcross_amd.drivers mvn D N RANK PIV [NGROUPS]
    python -m ttcross_amd.drivers coscoeff D N RANK PIV [NGROUPS]
    python -m ttcross_amd.drivers devfun D N RANK PIV [NGROUPS] [device|host|wave] [SOURCE.hip NAME]
    python -m ttcross_amd.drivers tijk WORKLOAD NPTS MODE      (batched element evaluation: c64 | d64 | rand256 | r16d64 | a file of dtt_write)
    python -m ttcross_amd.drivers algebra WORKLOAD [REPS]      (x + x, x - x, x o w, x o x, dist on the device and by the host route)
    python -m ttcross_amd.drivers roundsum WORKLOAD M [RANK] [MODE] (rounded sum of M terms made from the workload's train: lincomb_round)
    python -m ttcross_amd.drivers compose WORKLOAD OP [MAXRANK] (cross approximation of product | ratio | sqrtabs of the workload's train)
    python -m ttcross_amd.drivers samplereal WORKLOAD NPTS[,NPTS...] (real-valued samples from the interpolant of the workload's train: sample_real)
    python -m ttcross_amd.drivers samplesq WORKLOAD NPTS [MODE] [REPEATS] (samples from the square of the workload's train: sample_sq; WORKLOAD signed: importance weights)
    python -m ttcross_amd.drivers samplesqreal WORKLOAD NPTS [MODE] [REPEATS] (real-valued samples from the square of the interpolant: sample_sq_real; WORKLOAD signed: importance weights)
    python -m ttcross_amd.drivers rosenblatt WORKLOAD NPTS [MODE] [REPEATS] (the way back: rosenblatt_sq_real at sample_sq_real's own points, timed next to it)
    python -m ttcross_amd.drivers dirt D N R NLAYERS           (a layered transport over a beta ladder: layer 1 a device integrand, layers 2 and up pulled back on the device)

devfun: the rational example integrand (examples/devfun/rational.hip) as a LOADED device integrand (TTX_FUN_DEVICE), in its
wave form, or -- host -- its C twin through the host callback (TTX_FUN_HOST; needs gcc); SOURCE.hip NAME loads another
integrand over the same box set-up.
"""
import math
import sys

import numpy as np

import os

from .engine import (DEVFUN_DIR, TTX_FUN_COSCOEFF, TTX_FUN_DEVICE, TTX_FUN_HOST, TTX_FUN_ISING, TTX_FUN_MVN, TTX_FUN_STDNORM, TTCross,
                     TTXError, compile_device_fun, transport_sample)

EPS = 2.220446049250313e-16
TPI = 6.283185307179586476925286766559

# Ising integrals C_m, D_m, E_m (Bailey, Borwein & Crandall 2006) -- the table of test_crs_ising.f90:71-100
ISING_TRU = {
    ("c", 2): 1.0, ("c", 3): 0.78130241289648629687, ("c", 4): 0.70119986017642999982,
    ("c", 5): 0.66575980019993742832, ("c", 6): 0.64863420903100707526, ("c", 8): 0.63548402675916322614,
    ("c", 16): 0.63050394617323726351, ("c", 32): 0.63047350420733980638, ("c", 64): 0.63047350337438679649,
    ("c", 128): 0.63047350337438679612, ("c", 256): 0.63047350337438679612, ("c", 512): 0.63047350337438679612,
    ("c", 1024): 0.63047350337438679612,
    ("d", 2): 1.0 / 3, ("d", 5): 0.0024846057623403154800, ("d", 6): 0.00048914170018803477510,
    ("e", 5): 0.0034936537117295217407, ("e", 6): 0.00068783287182640943700,
}


def lgwt(n):
    """Gauss-Legendre nodes/weights on [-1,1] (lib/quad.f90:97-131)."""
    x = np.zeros(n)
    w = np.zeros(n)
    small = 5 * EPS
    for i in range(1, (n + 1) // 2 + 1):
        z = math.cos((TPI * (4 * i - 1)) / (8 * n + 4))
        while True:
            p1, p2 = 1.0, 0.0
            for j in range(1, n + 1):
                p3, p2 = p2, p1
                p1 = ((2 * j - 1) * z * p2 - (j - 1) * p3) / j
            pp = n * (z * p1 - p2) / (z * z - 1)
            z1 = z
            z = z1 - p1 / pp
            if abs(z - z1) <= small:
                break
        x[i - 1], x[n - i] = -z, z
        w[i - 1] = w[n - i] = 2.0 / ((1 - z * z) * pp * pp)
    return x, w


def ising_setup(kind, m, n):
    """test_crs_ising.f90:40,60-69,102-144 -> dict(n, par, quad, tru, acc, rescale)."""
    kind = kind.lower()
    if n % 2 == 0:
        n += 1
    x, w = lgwt(n)
    par = np.zeros(2 * n + 1)
    par[2 * n] = {"c": 1.0, "d": 2.0, "e": 3.0}[kind]
    par[n:2 * n] = 0.5 * w
    par[:n] = (x + 1.0) / 2
    rescale = kind in "de" and m >= 10
    val = float(n // 2)
    par[n:2 * n] = (5.0 * val if rescale else val) * par[n:2 * n]
    d = m - 1
    return dict(n=[n] * d, par=par, quad=[np.full(n, 1.0 / val)] * d, tru=ISING_TRU.get((kind, m)), acc=500 * EPS,
                rescale=rescale, fun_id=TTX_FUN_ISING, aux=None)


def mvn_init(d, r=0.0, T=1.0):
    """lib/mvn_pdf.f90:21-60: mean, inverse covariance and determinant of the driver's test distribution.
    Sigma = s2*((1-c) I + c 11') has the closed-form inverse/determinant used here (host set-up only)."""
    sigma, corr = 0.4, 0.5
    mu = np.full(d, math.log(100.0) + (r - 0.5 * sigma ** 2) * T)
    cov = (np.full((d, d), sigma * corr * sigma) + np.diag(np.full(d, sigma * sigma - sigma * corr * sigma))) * T
    inv = np.linalg.inv(cov)
    det = np.linalg.det(cov)
    return np.concatenate([mu, inv.ravel(order="F"), [det]])


def box_setup(kind, d, n):
    """test_crs_stdnorm.f90:70-112 / test_crs_mvn.f90:72-118."""
    if n % 2 == 0:
        n += 1
    x, w = lgwt(n)
    if kind == "stdnorm":
        a, b, acc, tru = -10.0, 10.0, 5 * EPS, math.sqrt(3.141592653589793238) ** d
    else:
        a, b, acc, tru = float(np.float32(0.525170)), float(np.float32(8.525170)), 500 * EPS, 1.0
    par = np.zeros(2 * n)
    par[:n] = 0.5 * ((b - a) * x + (a + b))
    par[n:] = (0.5 * (b - a)) * w
    return dict(n=[n] * d, par=par, quad=[par[n:].copy()] * d, tru=tru, acc=acc, rescale=False,
                fun_id=TTX_FUN_STDNORM if kind == "stdnorm" else TTX_FUN_MVN, aux=mvn_init(d) if kind == "mvn" else None)


COS_A, COS_B = 0.525170185988090843, 8.52517018598809173     # test_crs_coscoeff.f90: init_coefficients(lower=, upper=)


def coscoeff_setup(d, n, sigma=0.4, corr=0.5, X0=math.log(100.0), rate=0.0, T=1.0, a=COS_A, b=COS_B):
    """test_crs_coscoeff.f90:75-168: the mean and covariance of the log-prices, [a, b], acc = 500 eps; the integrand is
    calc_coefficient (TTX_FUN_COSCOEFF) with aux = [mu, Sigma column-major, a, b].  No quadrature: the driver keeps the train."""
    if n % 2 == 0:
        n += 1
    mu = np.array([X0 + (rate - 0.5 * (sigma * sigma)) * T for _ in range(d)])
    cov = np.empty((d, d))
    for i in range(d):
        for j in range(d):
            cov[i, j] = (sigma * sigma) * T if i == j else ((sigma * corr) * sigma) * T
    aux = np.concatenate([mu, cov.ravel(order="F"), [a, b]])
    return dict(n=[n] * d, par=np.zeros(0), quad=None, tru=None, acc=500 * EPS, rescale=False, fun_id=TTX_FUN_COSCOEFF, aux=aux)


def devfun_setup(d, n):
    """test_crs_box.inc on [0, 1]: Gauss-Legendre nodes and weights, par = [nodes(1:n), weights(1:n), 0] (2n+1 entries, the
    drivers' convention), quadrature with the weights, acc = 500 eps.  The integrand is the rational example function."""
    if n % 2 == 0:
        n += 1
    x, w = lgwt(n)
    par = np.zeros(2 * n + 1)
    par[:n] = 0.5 * (x + 1.0)
    par[n:2 * n] = 0.5 * w
    return dict(n=[n] * d, par=par, quad=[par[n:2 * n].copy()] * d, tru=None, acc=500 * EPS, rescale=False, fun_id=TTX_FUN_DEVICE, aux=None)


_RATIONAL_C = """#include <stdint.h>
double ttx_rational(const int32_t *m, const int32_t *ind, const int32_t *n, const double *par)
{ double s1 = 0.0, s2 = 0.0; (void)n; for (int i = 0; i < *m; i++) { const double x = par[ind[i] - 1]; s1 = s1 + x; s2 = s2 + x * x; } return s1 / (1.0 + s2); }
"""
_host_keep = []


def _rational_host_addr():
    """The C twin of rational.hip as a host callback (for the device-vs-host comparison of the devfun workload): compiled with gcc
    into the user's cache directory."""
    import ctypes
    import subprocess
    import tempfile
    bdir = os.path.join(os.environ.get("XDG_CACHE_HOME") or tempfile.gettempdir(), "ttcross_amd_devfun")
    os.makedirs(bdir, exist_ok=True)
    src, so = os.path.join(bdir, "rational.c"), os.path.join(bdir, "librational.so")
    if not os.path.exists(so):
        with open(src, "w") as f:
            f.write(_RATIONAL_C)
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", so + f".{os.getpid()}"], check=True)
        os.replace(so + f".{os.getpid()}", so)
    lib = ctypes.CDLL(so)
    _host_keep.append(lib)
    return ctypes.cast(lib.ttx_rational, ctypes.c_void_p).value


def run_devfun(argv, device=0, verbose=True):
    m, n, r, piv = int(argv[0]), int(argv[1]), int(argv[2]), int(argv[3])
    rest = list(argv[4:])
    ng = int(rest.pop(0)) if rest and rest[0].isdigit() else 1
    how = rest.pop(0) if rest and rest[0] in ("device", "host", "wave") else "device"
    s = devfun_setup(m, n)
    if how == "host":
        tt = TTCross(s["n"], TTX_FUN_HOST, [], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], nproc=ng, device=device, verbose=verbose)
        tt.set_integrand_host(_rational_host_addr(), s["par"])
    else:
        src, name = (rest[0], rest[1]) if len(rest) >= 2 else \
            (os.path.join(DEVFUN_DIR, "rational_wave.hip" if how == "wave" else "rational.hip"), "rational_wave" if how == "wave" else "rational")
        tt = TTCross(s["n"], TTX_FUN_DEVICE, [], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], nproc=ng, device=device, verbose=verbose)
        tt.set_integrand_device(compile_device_fun(src), name, s["par"])
    tt.run()
    val = tt.quad(s["quad"])
    if verbose:
        print("...with%12d evaluations completed in %12.4E sec." % (tt.neval, tt.seconds))
        print("computed value: %.16e" % val)
        print("integrand: %s, host calls %d" % (how, tt.host_calls))
    return tt, val, s


def run_driver(argv, device=0, verbose=True):
    drv = argv[0]
    if drv == "devfun":
        return run_devfun(argv[1:], device=device, verbose=verbose)
    if drv == "coscoeff":
        m, n, r, piv = int(argv[1]), int(argv[2]), int(argv[3]), int(argv[4])
        ng = int(argv[5]) if len(argv) > 5 else 1
        s = coscoeff_setup(m, n)
        tt = TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], aux=s["aux"], nproc=ng, device=device,
                     verbose=verbose)
        tt.run()
        if verbose:
            print("...with%12d evaluations completed in %12.4E sec." % (tt.neval, tt.seconds))
        return tt, None, s
    if drv == "ising":
        kind, m, n, r, piv = argv[1], int(argv[2]), int(argv[3]), int(argv[4]), int(argv[5])
        ng = int(argv[6]) if len(argv) > 6 else 1
        s = ising_setup(kind, m, n)
    else:
        m, n, r, piv = int(argv[1]), int(argv[2]), int(argv[3]), int(argv[4])
        ng = int(argv[5]) if len(argv) > 5 else 1
        s = box_setup(drv, m, n)
    tt = TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"],
                 aux=s["aux"], nproc=ng, device=device, verbose=verbose)
    tt.run()
    val = tt.quad(s["quad"])
    if verbose:
        print("...with%12d evaluations completed in %12.4E sec." % (tt.neval, tt.seconds))
        print("computed value: %.16e%s" % (val, "  / 5**(m-1)" if s["rescale"] else ""))
        if s["tru"]:
            print("analytic value: %.16e" % s["tru"])
            print("correct digits:%7.2f" % (-math.log10(abs(1.0 - val / s["tru"]))))
    return tt, val, s


def chf_weights(par, n, d, nfreq=32, upper=300.0):
    """The complex rank-1 quadrature weights of test_crs_chf.f90:153-168: for frequency k the weight of node p in every
    mode is w(p) * exp(i * omega_k * exp(x(p)) / d), omega_k = k*pi/(upper - 0).  Returns an (nfreq, d*n) array."""
    x, w = par[:n], par[n:2 * n]
    return np.array([np.tile(w * np.exp(1j * (k * math.pi / upper) * np.exp(x) / d), d) for k in range(nfreq)])


def cos_approximate(xs, phis, lower_bound, upper_bound, n_terms=None):
    """lib/cos_approx.f90: COS-method density at the points xs from characteristic-function values phis[k] = phi(k pi/(b-a)):
    f(x) ~ sum' 2/(b-a) Re(phi_k exp(-i w_k a)) cos(w_k (x - a)), first term halved (test_crs_pdf.f90:190)."""
    phis = np.asarray(phis, dtype=np.complex128)
    n = len(phis) if n_terms is None else n_terms
    if n > len(phis):
        raise ValueError("n_terms exceeds the size of phis")
    w = np.arange(n) * (math.pi / (upper_bound - lower_bound))
    c = 2.0 / (upper_bound - lower_bound) * np.real(phis[:n] * np.exp(-1j * w * lower_bound))
    c[0] /= 2.0
    return np.cos(np.outer(np.asarray(xs, dtype=np.float64) - lower_bound, w)) @ c


def run_pdf(argv, device=0, verbose=True, n_pts=200, upper=300.0):
    """test_crs_pdf.f90: the chf pipeline followed by the COS-method density of the basket average on linspace(0, upper)."""
    tt, vals, s = run_chf(argv, device=device, verbose=False)
    xs = np.linspace(0.0, upper, n_pts)
    pdf = cos_approximate(xs, vals, 0.0, upper, 32)
    if verbose:
        for x, f in zip(xs, pdf):
            print("%.16e %.16e" % (x, f))
    return tt, xs, pdf


def run_chf(argv, device=0, verbose=True):
    """test_crs_chf.f90:104-168: TT-cross of the multivariate-normal density WITHOUT a quadrature argument, then the
    characteristic function of the basket average at 32 frequencies as complex rank-1 quadratures of the resident
    train (ztt_quad, lib/dmrgg.f90:1418), all 32 in ONE batched device call."""
    d, n, r, piv = int(argv[0]), int(argv[1]), int(argv[2]), int(argv[3])
    ng = int(argv[4]) if len(argv) > 4 else 1
    s = box_setup("mvn", d, n)
    n = s["n"][0]
    tt = TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], aux=s["aux"], nproc=ng, device=device, verbose=verbose)
    tt.run()
    vals = tt.zquad(chf_weights(s["par"], n, d))
    if verbose:
        print("...with%12d evaluations completed in %12.4E sec." % (tt.neval, tt.seconds))
        for k, v in enumerate(vals):
            print("computed value: %3d %.16e %.16e" % (k, v.real, v.imag))
    return tt, vals, s


TIJK_WORKLOADS = {"c64": ("c", 64, 51, 32, 2), "d64": ("d", 64, 51, 32, 2), "c8": ("c", 8, 33, 12, 2)}


def tijk_train(workload, device=0):
    """The train of a tijk measurement: the result of an Ising sweep (c64, d64, c8: 8 bond groups as the benchmark runs them
    where the train is long enough), a random train of the D_256 shape (rand256: d = 255, n = 101, r = 64, entries scaled so
    that elements stay of order one), a random rank-16 train of the D_64 shape (r16d64) or a file written by dtt_write."""
    if workload in TIJK_WORKLOADS:
        kind, m, n, r, piv = TIJK_WORKLOADS[workload]
        s = ising_setup(kind, m, n)
        return TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"],
                       nproc=8 if m >= 32 else 1, device=device).run()
    if workload == "r16d64":                               # standard normal cores of rank 16 in the D_64 shape, elements of order one
        rng = np.random.default_rng(1)
        d, n, r = 63, 51, 16
        return TTCross.from_cores([rng.standard_normal(((1 if k == 0 else r), n, (1 if k == d - 1 else r))) / np.sqrt(n * r) * 2.0 for k in range(d)],
                                  device=device)
    if workload.startswith("rand"):
        d = int(workload[4:]) - 1
        rng = np.random.default_rng(256)
        r = [1] + [64] * (d - 1) + [1]
        return TTCross.from_cores([rng.uniform(0.0, 1.0, (r[k], 101, r[k + 1])) / (0.5 * r[k + 1]) for k in range(d)], device=device)
    return TTCross.read(workload, device=device)


def run_tijk(argv, device=0, repeats=5, tt=None):
    """tijk WORKLOAD NPTS MODE: npts seeded multi-indices drawn ON the device, one warm-up and `repeats` timed batches through
    the device-pointer entry (outputs stay on the device); prints one JSON line with the median."""
    import json
    import time
    import torch
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload, npts, mode = argv[0], int(float(argv[1])), argv[2]
    tt = tt or tijk_train(workload, device=device)
    dev = torch.device("cuda", device)
    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    n = torch.tensor(np.asarray(tt._n), dtype=torch.int32, device=dev)
    ind = (torch.randint(0, 2 ** 31 - 1, (npts, tt.d), dtype=torch.int32, device=dev, generator=g) % n + 1).contiguous()
    torch.cuda.synchronize(dev)
    out = tt.tijk_batch(ind, mode)
    ms = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = tt.tijk_batch(ind, mode)            # synchronises before it returns
        ms.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(ms))
    res = dict(workload=workload, npts=npts, mode_asked=mode, mode=tt.eval_last_mode, d=tt.d, max_rank=int(tt.ranks().max()),
               ms=med, ms_all=[round(x, 4) for x in ms], points_per_s=npts / (med * 1e-3) if med > 0 else None,
               checksum=float(out.sum().item()), invalid=int((out == -3.0).sum().item()))
    print(json.dumps(res))
    return tt, ind, out, res


def _trainfun_twin(trains, op):
    """The host twin of an integrand of trains (tests/trainfun_ref.c of this tree, compiled with gcc into the user's cache
    directory) loaded with the trains' cores; returns the callback's address, or None where the source or gcc is missing."""
    import ctypes
    import shutil
    import subprocess
    import tempfile
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "trainfun_ref.c")
    if not os.path.exists(src) or not shutil.which("gcc"):
        return None
    bdir = os.path.join(os.environ.get("XDG_CACHE_HOME") or tempfile.gettempdir(), "ttcross_amd_devfun")
    os.makedirs(bdir, exist_ok=True)
    so = os.path.join(bdir, "libtrainfun_ref.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", so + f".{os.getpid()}", "-lm"], check=True)
        os.replace(so + f".{os.getpid()}", so)
    lib = ctypes.CDLL(so)
    _host_keep.append(lib)
    ip, dp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    for t, x in enumerate(trains):
        r = np.ascontiguousarray(x.ranks(), dtype=np.int32)
        n = np.ascontiguousarray(x._n, dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([x.core(k).ravel(order="F") for k in range(1, x.d + 1)]))
        if lib.trainfun_set(t, x.d, n.ctypes.data_as(ip), r.ctypes.data_as(ip), flat.ctypes.data_as(dp)):
            raise TTXError("compose: the host twin refused a train")
    lib.trainfun_count(len(trains))
    return ctypes.cast(getattr(lib, "trainfun_" + op), ctypes.c_void_p).value


def run_compose(argv, device=0, tt=None, npts=1 << 18):
    """compose WORKLOAD OP [MAXRANK]: the cross approximation of product (x x), ratio (x / (x + x)) or sqrtabs (sqrt |x|) of the
    workload's train x (tijk_train) as an integrand of trains (TTX_FUN_TRAINS); prints one JSON line: the run, neval, the slot
    kernel's elements per second (a second, profiled run), the same run through the host callback with the host twin, and
    tijk_batch(.., "exact") points per second on the same operand."""
    import json
    import time
    import torch
    torch.cuda.init()          # as run_tijk: torch's device first
    workload, op = argv[0], argv[1]
    x = tt or tijk_train(workload, device=device)
    r = int(argv[2]) if len(argv) > 2 else int(x.ranks().max())
    y = x.axpby(1.0, 1.0, x) if op == "ratio" else None
    trains = {"product": [x, x], "ratio": [x, y], "sqrtabs": [x]}[op]
    nproc = 8 if x.d >= 31 else 1
    quad = [np.full(int(nk), 1.0 / int(nk)) for nk in x._n]
    kw = dict(accuracy=500 * EPS, pivoting=2, quad=quad, nproc=nproc)
    c = TTCross.of_trains(trains, op, r, device=device, **kw).run()
    c.run()                                             # the timed run: the first one carries the first-launch costs
    res = dict(workload=workload, op=op, m=len(trains), d=x.d, maxrank=r, operand_max_rank=int(max(t.ranks().max() for t in trains)),
               run_ms=c.seconds * 1e3, neval=c.neval, value=c.quad(quad), ranks_max=int(c.ranks().max()))
    c.set_profile(True)
    c.run()
    last = c.trainfun_last()
    res.update(slot_ms=last["ms"], slot_launches=last["launches"], slot_elements=last["elements"],
               slot_elements_per_s=last["elements"] / (last["ms"] * 1e-3) if last["ms"] > 0 else None)
    addr = _trainfun_twin(trains, op)
    if addr is not None:
        hh = TTCross(x._n, TTX_FUN_HOST, [], r, device=device, **kw)
        hh.set_integrand_host(addr, [0.0]).run()
        res.update(host_run_ms=hh.seconds * 1e3, host_calls=hh.host_calls, host_same_value=hh.quad(quad) == res["value"],
                   host_same_tapes=bool(np.array_equal(hh.tapes(), c.tapes())))
        hh.close()
    else:
        res["host_route"] = "not run: the host twin (tests/trainfun_ref.c of the source tree, compiled with gcc) is not available here"
        print("compose: no host twin (tests/trainfun_ref.c or gcc missing): the host-callback comparison is left out", file=sys.stderr)
    rng = np.random.default_rng(1)
    ind = np.stack([rng.integers(1, int(nk) + 1, size=npts) for nk in x._n], axis=1).astype(np.int32)
    ti = torch.from_numpy(ind).to(torch.device("cuda", device))
    x.tijk_batch(ti, "exact")
    ms = []
    for _ in range(5):
        t0 = time.perf_counter()
        x.tijk_batch(ti, "exact")
        ms.append((time.perf_counter() - t0) * 1e3)
    res.update(tijk_exact_points_per_s=npts / (float(np.median(ms)) * 1e-3))
    if res.get("slot_elements_per_s"):
        res["slot_vs_tijk_per_operand"] = res["slot_elements_per_s"] / (res["tijk_exact_points_per_s"] / len(trains))
    print(json.dumps(res))
    c.close()
    if y is not None:
        y.close()
    return res


def keep_flags(spec, d):
    """KEEPSPEC of the contract sub-command: 'ends' (first and last mode), 'mid' (the two middle modes), 'everyN' (modes N, 2N,
    ...), or 1-based mode numbers separated by commas"""
    if spec == "ends":
        kept = {1, d}
    elif spec == "mid":
        kept = {d // 2, d // 2 + 1}
    elif spec.startswith("every"):
        kept = set(range(int(spec[5:]), d + 1, int(spec[5:])))
    else:
        kept = {int(x) for x in spec.split(",")}
    return [int(k + 1 in kept) for k in range(d)]


def contract_host(tt, keep, w):
    """what a user does without ttx_contract: every core to the host, the contraction in numpy, the result back to the device"""
    cores = [tt.core(k) for k in range(1, tt.d + 1)]
    out, p = [], None
    for c, kp, q in zip(cores, keep, w):
        if kp:
            out.append(c if p is None else np.einsum("ab,bjc->ajc", p, c))
            p = None
        else:
            m = np.einsum("ajb,j->ab", c, q)
            p = m if p is None else p @ m
    if p is not None:
        out[-1] = np.einsum("ajb,bc->ajc", out[-1], p)
    return TTCross.from_cores(out, device=tt.device)


def run_contract(argv, device=0, tt=None):
    """contract WORKLOAD KEEPSPEC [REPS]: the trains of the tijk sub-command; contract(keep) and marginals() with plain-sum
    weights of 1 / n, one warm-up and the median of REPS (default 10) calls each; per call the milliseconds, and the
    milliseconds and bytes / s of the mode-sum kernel (8 sum r0 n r1 over the contracted cores); then the host route once.
    Prints one JSON line."""
    import json
    import time
    workload, spec = argv[0], argv[1]
    reps = int(argv[2]) if len(argv) > 2 else 10
    tt = tt or tijk_train(workload, device=device)
    keep = keep_flags(spec, tt.d)
    w = [np.full(int(nk), 1.0 / int(nk)) for nk in tt._n]

    def timed(fn):
        fn()
        ms, ks = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()                                   # synchronises before it returns
            ms.append((time.perf_counter() - t0) * 1e3)
            ks.append(tt.contract_modesum())
        kms = float(np.median([k[0] for k in ks]))
        return dict(ms=float(np.median(ms)), ms_min=float(min(ms)), modesum_ms=kms, modesum_bytes=ks[0][1],
                    modesum_bytes_per_s=ks[0][1] / (kms * 1e-3) if kms > 0 else None)

    res = dict(workload=workload, keep=spec, kept=int(sum(keep)), d=tt.d, max_rank=int(tt.ranks().max()), reps=reps)
    res["contract"] = timed(lambda: tt.contract(keep, w).close())
    res["marginals"] = timed(lambda: tt.marginals(w))
    t0 = time.perf_counter()
    ref = contract_host(tt, keep, w)
    res["host_route_ms"] = (time.perf_counter() - t0) * 1e3
    ct = tt.contract(keep, w)
    wk = [q for q, kp in zip(w, keep) if kp]
    res["quad"] = dict(source=tt.quad(w), contracted=ct.quad(wk), host_route=ref.quad(wk))
    res["ranks"] = ct.ranks().tolist()
    print(json.dumps(res))
    return res


def algebra_host(coefs, trains):
    """what a user does without ttx_lincomb: every core to the host, the block cores in numpy, the result back to the device"""
    src = [[t.core(k) for k in range(1, t.d + 1)] for t in trains]
    d, out = trains[0].d, []
    for k in range(d):
        r0 = 1 if k == 0 else sum(x[k].shape[0] for x in src)
        r1 = 1 if k == d - 1 else sum(x[k].shape[2] for x in src)
        z = np.zeros((r0, src[0][k].shape[1], r1))
        ro = co = 0
        for c, x in zip(coefs, src):
            g = x[k]
            z[ro:ro + g.shape[0], :, co:co + g.shape[2]] = c * g if k == 0 else g
            ro += g.shape[0] if k > 0 else 0
            co += g.shape[2] if k < d - 1 else 0
        out.append(z)
    return TTCross.from_cores(out, device=trains[0].device)


def hadamard_host(x, y):
    """the host route of x.hadamard(y)"""
    out = []
    for k in range(1, x.d + 1):
        a, b = x.core(k), y.core(k)
        z = b[:, None, :, :, None] * a[None, :, :, None, :]             # plain products: a sum-of-products routine would turn -0.0 into +0.0
        out.append(z.reshape(b.shape[0] * a.shape[0], a.shape[1], b.shape[2] * a.shape[2]))
    return TTCross.from_cores(out, device=x.device)


def run_algebra(argv, device=0, tt=None):
    """algebra WORKLOAD [REPS]: the trains of the tijk sub-command; x + x, x - x, x o w with a rank-1 weight train w (1 / n), x o x
    where the squared ranks fit, and dist of the exact against the fast-arithmetic train where the workload is an Ising sweep.
    Per case: one warm-up and the median of REPS (default 10) calls, the assembly kernel's milliseconds and bytes through
    ttx_algebra_last, its rate as a fraction of the bandwidth probe (ttx_k_residual_bench on rows x 64 of the same byte count),
    and the host route once.  Prints one JSON line."""
    import json
    import time
    from .engine import k_residual_bench
    workload = argv[0]
    reps = int(argv[1]) if len(argv) > 1 else 10
    tt = tt or tijk_train(workload, device=device)
    rmax = int(tt.ranks().max())
    w = TTCross.from_cores([np.full((1, int(nk), 1), 1.0 / int(nk)) for nk in tt._n], device=device)

    def timed(fn, host):
        try:
            fn().close()
        except TTXError as e:                       # e.g. a result the engine cannot hold (its storage for d cores of the new rank)
            return dict(error=str(e))
        ms, ks = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()                                # synchronises before it returns
            ms.append((time.perf_counter() - t0) * 1e3)
            ks.append(tt.algebra_last())
            r.close()
        kms, rd, wr = float(np.median([k[0] for k in ks])), ks[0][1], ks[0][2]
        probe_ms, probe_bytes = k_residual_bench(max(1, int((rd + wr) / (8 * 64))), 64, 20, device=device)
        rate, probe = (rd + wr) / (kms * 1e-3), probe_bytes / (probe_ms * 1e-3)
        t0 = time.perf_counter()
        ref = host()
        host_ms = (time.perf_counter() - t0) * 1e3
        r = fn()
        same = all(r.core(k).tobytes() == ref.core(k).tobytes() for k in range(1, r.d + 1))
        out = dict(ms=float(np.median(ms)), kernel_ms=kms, bytes_read=rd, bytes_written=wr, bytes_per_s=rate, probe_bytes_per_s=probe,
                   fraction_of_probe=rate / probe, host_route_ms=host_ms, same_bytes_as_host_route=same, ranks_max=int(r.ranks().max()))
        r.close()
        ref.close()
        return out

    res = dict(workload=workload, d=tt.d, max_rank=rmax, reps=reps)
    if 2 * rmax <= 128:
        res["x_plus_x"] = timed(lambda: TTCross.lincomb([1.0, 1.0], [tt, tt]), lambda: algebra_host([1.0, 1.0], [tt, tt]))
        res["x_minus_x"] = timed(lambda: TTCross.lincomb([1.0, -1.0], [tt, tt]), lambda: algebra_host([1.0, -1.0], [tt, tt]))
    res["x_times_w"] = timed(lambda: tt.hadamard(w), lambda: hadamard_host(tt, w))
    if rmax * rmax <= 128:
        res["x_times_x"] = timed(lambda: tt.hadamard(tt), lambda: hadamard_host(tt, tt))
    if workload in TIJK_WORKLOADS and 2 * rmax <= 128:
        kind, m, n, r, piv = TIJK_WORKLOADS[workload]
        s = ising_setup(kind, m, n)
        fast = TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"],
                       nproc=8 if m >= 32 else 1, device=device, arith="fast").run()
        if fast.arith == "fast" and all(int(a) + int(b) <= 128 for a, b in zip(tt.ranks()[1:-1], fast.ranks()[1:-1])):
            t0 = time.perf_counter()
            dist = tt.dist(fast)
            ms = (time.perf_counter() - t0) * 1e3
            nx, ny, xy = tt.norm(), fast.norm(), tt.dot(fast)
            res["dist_exact_fast"] = dict(dist=dist, ms=ms, norm_exact=nx, norm_fast=ny,
                                          by_dots=float(np.sqrt(max(nx * nx - 2.0 * xy + ny * ny, 0.0))))
        fast.close()
    print(json.dumps(res))
    return res


def cos_matrix(xs, n_terms, a, b):
    """The synthesis matrix of a cosine expansion on [a, b]: entry (j, k) = cos(k pi (xs[j] - a) / (b - a)), k = 0 .. n_terms-1.
    Applied to a mode of a train of COS coefficients (TTCross.mode_apply) it gives the values at the points xs; the coefficients
    carry the halved first term and the factor 2 / (b - a) themselves, as the c of cos_approximate."""
    xs = np.asarray(xs, dtype=np.float64).ravel()
    return np.cos(np.outer(xs - a, np.arange(int(n_terms)) * (math.pi / (b - a))))


def mode_apply_host(tt, mats):
    """what a user does without ttx_mode_apply: every core to the host, the products in numpy (the sums over ascending i with a
    separate multiply and add, the order of TTX_EVAL_EXACT), the result back to the device"""
    out = []
    for k, a in enumerate(mats):
        g = tt.core(k + 1)
        if a is None:
            out.append(g)
            continue
        a = np.asarray(a, dtype=np.float64)
        z = np.zeros((g.shape[0], a.shape[0], g.shape[2]))
        for i in range(g.shape[1]):
            z = z + a[None, :, i, None] * g[:, None, i, :]
        out.append(z)
    return TTCross.from_cores(out, device=tt.device)


def run_modeapply(argv, device=0, tt=None):
    """modeapply WORKLOAD M [MODE] [REPS]: the trains of the tijk sub-command; an M x n matrix of seeded standard normals applied
    to every mode in MODE (exact, mfma or auto; default mfma), one warm-up and the median of REPS (default 10) calls: per call the
    milliseconds with the new engine's creation, the apply kernel's milliseconds, bytes and flops through ttx_mode_apply_last, its
    rates and its share of the bandwidth probe (ttx_k_residual_bench on rows x 64 of the same byte count); then the host route
    once and the comparison with it: bit for bit in exact, against 2 (n + 1) u sum |A| |G| otherwise.  Prints one JSON line."""
    import json
    import time
    from .engine import k_residual_bench
    workload, M = argv[0], int(argv[1])
    mode = argv[2] if len(argv) > 2 else "mfma"
    reps = int(argv[3]) if len(argv) > 3 else 10
    tt = tt or tijk_train(workload, device=device)
    rng = np.random.default_rng(M)
    mats = [rng.standard_normal((M, int(nk))) for nk in tt._n]
    tt.mode_apply(mats, mode).close()
    ms, ks = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = tt.mode_apply(mats, mode)               # synchronises before it returns
        ms.append((time.perf_counter() - t0) * 1e3)
        ks.append(tt.mode_apply_last())
        r.close()
    kms = float(np.median([k["ms"] for k in ks]))
    rd, wr, fl = ks[0]["bytes_read"], ks[0]["bytes_written"], ks[0]["flops"]
    probe_ms, probe_bytes = k_residual_bench(max(1, int((rd + wr) / (8 * 64))), 64, 20, device=device)
    rate, probe = (rd + wr) / (kms * 1e-3), probe_bytes / (probe_ms * 1e-3)
    res = dict(workload=workload, d=tt.d, max_rank=int(tt.ranks().max()), M=M, mode=mode, mode_ran=ks[0]["mode"], reps=reps,
               ms=float(np.median(ms)), ms_min=float(min(ms)), kernel_ms=kms, kernel_ms_min=float(min(k["ms"] for k in ks)),
               bytes_read=rd, bytes_written=wr, flops=fl, bytes_per_s=rate, probe_bytes_per_s=probe, fraction_of_probe=rate / probe,
               flops_per_s=fl / (kms * 1e-3))
    t0 = time.perf_counter()
    ref = mode_apply_host(tt, mats)
    res["host_route_ms"] = (time.perf_counter() - t0) * 1e3
    r = tt.mode_apply(mats, mode)
    if ks[0]["mode"] == "exact":
        res["same_bytes_as_host_route"] = all(r.core(k).tobytes() == ref.core(k).tobytes() for k in range(1, r.d + 1))
    else:
        worst = 0.0
        for k in range(1, r.d + 1):
            g, n = np.abs(tt.core(k)), int(tt._n[k - 1])
            S = np.einsum("ji,aib->ajb", np.abs(mats[k - 1]), g)
            diff = np.abs(r.core(k) - ref.core(k))
            worst = max(worst, float(np.max(diff / (2.0 * (n + 1) * 2.0 ** -53 * np.where(S > 0, S, 1.0)))))
        res["max_diff_over_bound"] = worst
        res["within_bound"] = worst <= 1.0
    r.close()
    ref.close()
    print(json.dumps(res))
    return res


def basis_host(tt, x, basis):
    """what a user does without ttx_basis_batch: every core to the host with core(k), the tables from basis_table, the chain of
    include/ttx.h as one numpy product per mode (BLAS order, so equal to the device to rounding only)"""
    from .engine import basis_table
    x = np.asarray(x, dtype=np.float64)
    if isinstance(basis, (tuple, list)) and basis and isinstance(basis[0], str):
        basis = [basis] * tt.d
    cores = [tt.core(k) for k in range(1, tt.d + 1)]
    v = np.ones((x.shape[0], 1))
    for k in range(tt.d - 1, -1, -1):
        g = cores[k]
        r0, n, r1 = g.shape
        phi = basis_table(basis[k], n, x[:, k])
        t = (v @ g.reshape(r0 * n, r1).T).reshape(x.shape[0], r0, n)
        v = np.einsum("paj,pj->pa", t, phi)
    return v[:, 0]


def basis_train(workload, device=0):
    """The train and the basis of a basis measurement: coscoeffD is a coscoeff_setup run of dimension D (n = 65, r = 20, piv = 1)
    with its own [a, b] and the halved first term; everything else is a train of the tijk sub-command, None for its basis."""
    if workload.startswith("coscoeff"):
        s = coscoeff_setup(int(workload[8:]), 65)
        tt = TTCross(s["n"], s["fun_id"], s["par"], 20, pivoting=1, accuracy=s["acc"], aux=s["aux"], device=device).run()
        return tt, ("cos", float(s["aux"][-2]), float(s["aux"][-1]), True)
    return tijk_train(workload, device=device), None


def run_basis(argv, device=0, repeats=5, tt=None, basis=None, host_npts=1000):
    """basis WORKLOAD NPTS [KIND] [MODE]: the trains of the tijk sub-command plus coscoeffD; KIND linear (default: hat functions on
    n equidistant nodes of [0, 1]) or cos (on [0, 1]; coscoeffD always takes its own cosine basis); MODE exact, mfma or auto
    (default).  NPTS seeded points drawn ON the device inside the basis' interval, one warm-up and `repeats` timed calls through
    the device-pointer entry; prints one JSON line: the median milliseconds, flops, the chain's TF/s and the table share from
    ttx_basis_last, and the host route (basis_host: every core pulled, numpy) on the first `host_npts` of the same points."""
    import json
    import time
    import torch
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload, npts = argv[0], int(float(argv[1]))
    kind = argv[2] if len(argv) > 2 else "linear"
    mode = argv[3] if len(argv) > 3 else "auto"
    if tt is None:
        tt, basis = basis_train(workload, device=device)
    if basis is None:
        basis = [("linear", np.linspace(0.0, 1.0, int(nk))) if kind == "linear" and nk > 1 else ("cos", 0.0, 1.0) for nk in tt._n]
        lo, hi = 0.0, 1.0
    else:
        lo, hi = basis[1], basis[2]
    dev = torch.device("cuda", device)
    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    x = (lo + (hi - lo) * torch.rand((npts, tt.d), dtype=torch.float64, device=dev, generator=g)).contiguous()
    torch.cuda.synchronize(dev)
    out = tt.basis_batch(x, basis, mode)
    ms, last = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = tt.basis_batch(x, basis, mode)        # synchronises before it returns
        ms.append((time.perf_counter() - t0) * 1e3)
        last.append(tt.basis_last())
    med = float(np.median(ms))
    ch, tb = float(np.median([k["ms_chain"] for k in last])), float(np.median([k["ms_table"] for k in last]))
    res = dict(workload=workload, npts=npts, kind=basis[0] if isinstance(basis[0], str) else kind, mode_asked=mode, mode=last[0]["mode"],
               d=tt.d, max_rank=int(tt.ranks().max()), ms=med, ms_all=[round(v, 4) for v in ms], ms_chain=ch, ms_table=tb,
               table_share=tb / (tb + ch) if tb + ch > 0 else None, flops=last[0]["flops"],
               chain_tflops=last[0]["flops"] / (ch * 1e-3) / 1e12 if ch > 0 else None, checksum=float(out.sum().item()),
               nan=int(torch.isnan(out).sum().item()))
    hp = min(npts, host_npts)
    if hp > 0:
        xh = x[:hp].cpu().numpy()
        t0 = time.perf_counter()
        ref = basis_host(tt, xh, basis)
        res["host_route_npts"] = hp
        res["host_route_ms"] = (time.perf_counter() - t0) * 1e3
        got = out[:hp].cpu().numpy()
        res["max_rel_diff_to_host_route"] = float(np.max(np.abs(got - ref)) / max(float(np.max(np.abs(ref))), 1e-300))
    print(json.dumps(res))
    return tt, x, out, res


def basis_grad_host(tt, x, basis):
    """what a user does without ttx_basis_grad_batch, the host route: every core to the host with core(k), the tables from
    basis_table and basis_dtable, the chain of basis_host right to left with the rows D_k kept (the same product summed against
    dphi), then the prefix vectors left to right and grad_k = prefix_k . D_k, one numpy product per mode and pass (BLAS order, so
    equal to the device to rounding only).  Returns (val, grad)."""
    from .engine import basis_dtable, basis_table
    x = np.asarray(x, dtype=np.float64)
    if isinstance(basis, (tuple, list)) and basis and isinstance(basis[0], str):
        basis = [basis] * tt.d
    cores = [tt.core(k) for k in range(1, tt.d + 1)]
    phis = [basis_table(basis[k], g.shape[1], x[:, k]) for k, g in enumerate(cores)]
    v = np.ones((x.shape[0], 1))
    D = [None] * tt.d
    for k in range(tt.d - 1, -1, -1):
        g = cores[k]
        r0, n, r1 = g.shape
        t = (v @ g.reshape(r0 * n, r1).T).reshape(x.shape[0], r0, n)
        D[k] = np.einsum("paj,pj->pa", t, basis_dtable(basis[k], n, x[:, k]))
        v = np.einsum("paj,pj->pa", t, phis[k])
    grad = np.zeros((x.shape[0], tt.d))
    pre = np.ones((x.shape[0], 1))
    for k in range(tt.d):
        g = cores[k]
        r0, n, r1 = g.shape
        grad[:, k] = np.einsum("pa,pa->p", pre, D[k])
        if k + 1 < tt.d:
            pre = np.einsum("pjk,pj->pk", (pre @ g.reshape(r0, n * r1)).reshape(x.shape[0], n, r1), phis[k])
    return v[:, 0], grad


def run_basisgrad(argv, device=0, repeats=5, tt=None, basis=None, host_npts=1000, subst_npts=10000, subst_repeats=None):
    """basisgrad WORKLOAD NPTS [KIND] [MODE]: the workloads, kinds and modes of the basis sub-command.  On the same seeded points
    (drawn on the device) and in the same session: one warm-up and `repeats` timed basis_grad_batch calls through the
    device-pointer entry, the same for one basis_batch call, the substitution route (d basis_tab calls, each with one mode's table
    replaced by its derivative table, tables formed on the host beforehand and not timed) on the first `subst_npts` points, and the
    host route (basis_grad_host) on the first `host_npts`.  Prints one JSON line with the medians and the ratios
    (subst_over_grad_same_npts: the substitution route's time per point over the gradient call's time per point;
    max_rel_diff_to_subst compares the modes listed in subst_modes_checked only, the ones whose tables were built)."""
    import json
    import time
    import torch
    from .engine import basis_dtable, basis_table
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload, npts = argv[0], int(float(argv[1]))
    kind = argv[2] if len(argv) > 2 else "linear"
    mode = argv[3] if len(argv) > 3 else "auto"
    if tt is None:
        tt, basis = basis_train(workload, device=device)
    if basis is None:
        basis = [("linear", np.linspace(0.0, 1.0, int(nk))) if kind == "linear" and nk > 1 else ("cos", 0.0, 1.0) for nk in tt._n]
        lo, hi = 0.0, 1.0
    else:
        lo, hi = basis[1], basis[2]
    entries = [basis] * tt.d if isinstance(basis[0], str) else list(basis)
    dev = torch.device("cuda", device)
    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    x = (lo + (hi - lo) * torch.rand((npts, tt.d), dtype=torch.float64, device=dev, generator=g)).contiguous()
    torch.cuda.synchronize(dev)

    def timed(call, reps=repeats):
        out = call()                                # warm-up
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = call()                            # synchronises before it returns
            ms.append((time.perf_counter() - t0) * 1e3)
        return out, float(np.median(ms)), [round(v, 4) for v in ms]

    (val, grad), ms_grad, all_grad = timed(lambda: tt.basis_grad_batch(x, basis, mode))
    last = tt.basis_grad_last()
    vb, ms_val, all_val = timed(lambda: tt.basis_batch(x, basis, last["mode"]))
    res = dict(workload=workload, npts=npts, kind=entries[0][0], mode_asked=mode, mode=last["mode"], chunk=last["chunk"], d=tt.d,
               max_rank=int(tt.ranks().max()), ms_grad=ms_grad, ms_grad_all=all_grad, ms_table=last["ms_table"], ms_back=last["ms_back"],
               ms_fwd=last["ms_fwd"], flops=last["flops"], ms_basis_batch=ms_val, ms_basis_batch_all=all_val, ratio_to_basis_batch=ms_grad / ms_val,
               val_is_basis_batch=bool(torch.equal(val, vb)), nan=int(torch.isnan(grad).sum().item()), checksum=float(grad.sum().item()))
    sp = min(npts, subst_npts)
    if sp > 0:
        xs = x[:sp].cpu().numpy()
        phis = [basis_table(e, int(nk), xs[:, k]) for k, (e, nk) in enumerate(zip(entries, tt._n))]
        dphis = [basis_dtable(e, int(nk), xs[:, k]) for k, (e, nk) in enumerate(zip(entries, tt._n))]
        tabs = [torch.from_numpy(np.ascontiguousarray(np.hstack([dphis[k] if k == m else phis[k] for k in range(tt.d)]))).to(dev) for m in range(min(tt.d, 2))]
        torch.cuda.synchronize(dev)
        # every call of the route costs the same: two distinct substituted tables are cycled through the d calls
        _, ms_sub, _ = timed(lambda: [tt.basis_tab(tabs[m % len(tabs)], last["mode"]) for m in range(tt.d)][-1], subst_repeats or repeats)
        gs = grad[:sp].cpu().numpy()
        first = np.stack([tt.basis_tab(tabs[m], last["mode"]).cpu().numpy() for m in range(len(tabs))], axis=1)
        res.update(subst_npts=sp, ms_subst_route=ms_sub, subst_modes_checked=list(range(1, len(tabs) + 1)), subst_over_grad_same_npts=(ms_sub / sp) / (ms_grad / npts),
                   max_rel_diff_to_subst=float(np.max(np.abs(gs[:, :len(tabs)] - first)) / max(float(np.max(np.abs(first))), 1e-300)))
    hp = min(npts, host_npts)
    if hp > 0:
        xh = x[:hp].cpu().numpy()
        t0 = time.perf_counter()
        _, ref = basis_grad_host(tt, xh, basis)
        res["host_route_npts"] = hp
        res["host_route_ms"] = (time.perf_counter() - t0) * 1e3
        res["max_rel_diff_to_host_route"] = float(np.max(np.abs(grad[:hp].cpu().numpy() - ref)) / max(float(np.max(np.abs(ref))), 1e-300))
    print(json.dumps(res))
    return tt, x, (val, grad), res


def basis_core_grad_host(tt, x, basis, c):
    """what a user does without ttx_basis_core_grad_batch, the host route: every core to the host with core(k), the tables from
    basis_table, the suffix states right to left and the prefix states left to right as in basis_grad_host, then one einsum per
    core over the points (BLAS order, so equal to the device to rounding only).  Returns (val, [G_1 .. G_d])."""
    from .engine import basis_table
    x, c = np.asarray(x, dtype=np.float64), np.asarray(c, dtype=np.float64)
    if isinstance(basis, (tuple, list)) and basis and isinstance(basis[0], str):
        basis = [basis] * tt.d
    cores = [tt.core(k) for k in range(1, tt.d + 1)]
    phis = [basis_table(basis[k], g.shape[1], x[:, k]) for k, g in enumerate(cores)]
    X = [None] * (tt.d + 1)
    X[tt.d] = np.ones((x.shape[0], 1))
    for k in range(tt.d - 1, -1, -1):
        g = cores[k]
        r0, n, r1 = g.shape
        t = (X[k + 1] @ g.reshape(r0 * n, r1).T).reshape(x.shape[0], r0, n)
        X[k] = np.einsum("paj,pj->pa", t, phis[k])
    G = []
    pre = np.ones((x.shape[0], 1))
    for k in range(tt.d):
        g = cores[k]
        r0, n, r1 = g.shape
        G.append(np.einsum("pa,pj,pk->ajk", c[:, None] * pre, phis[k], X[k + 1], optimize=True))
        if k + 1 < tt.d:
            pre = np.einsum("pjk,pj->pk", (pre @ g.reshape(r0, n * r1)).reshape(x.shape[0], n, r1), phis[k])
    return X[0][:, 0], G


def run_coregrad(argv, device=0, repeats=5, tt=None, basis=None, host_npts=1000):
    """coregrad WORKLOAD NPTS [KIND] [MODE]: the workloads, kinds and modes of the basis sub-command.  On the same seeded points and
    weights (drawn on the device) and in the same session: one warm-up and `repeats` timed basis_core_grad calls through the
    device-pointer entry, the same for basis_grad_batch (the same flop count, so ratio_to_basis_grad is the figure of merit), and
    the host route (basis_core_grad_host) on the first `host_npts`.  Prints one JSON line with the medians, the phases of
    ttx_basis_core_grad_last (table, back, fwd, acc) and the ratios."""
    import json
    import time
    import torch
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload, npts = argv[0], int(float(argv[1]))
    kind = argv[2] if len(argv) > 2 else "linear"
    mode = argv[3] if len(argv) > 3 else "auto"
    if tt is None:
        tt, basis = basis_train(workload, device=device)
    if basis is None:
        basis = [("linear", np.linspace(0.0, 1.0, int(nk))) if kind == "linear" and nk > 1 else ("cos", 0.0, 1.0) for nk in tt._n]
        lo, hi = 0.0, 1.0
    else:
        lo, hi = basis[1], basis[2]
    entries = [basis] * tt.d if isinstance(basis[0], str) else list(basis)
    dev = torch.device("cuda", device)
    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    x = (lo + (hi - lo) * torch.rand((npts, tt.d), dtype=torch.float64, device=dev, generator=g)).contiguous()
    c = torch.randn(npts, dtype=torch.float64, device=dev, generator=g).contiguous()
    torch.cuda.synchronize(dev)

    def timed(call):
        out = call()                                # warm-up
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = call()                            # synchronises before it returns
            ms.append((time.perf_counter() - t0) * 1e3)
        return out, float(np.median(ms)), [round(v, 4) for v in ms]

    (val, G), ms_cg, all_cg = timed(lambda: tt.basis_core_grad(x, basis, c, mode))
    last = tt.basis_core_grad_last()
    (vg, _), ms_bg, all_bg = timed(lambda: tt.basis_grad_batch(x, basis, last["mode"]))
    res = dict(workload=workload, npts=npts, kind=entries[0][0], mode_asked=mode, mode=last["mode"], chunk=last["chunk"], d=tt.d,
               max_rank=int(tt.ranks().max()), ms_core_grad=ms_cg, ms_core_grad_all=all_cg, ms_table=last["ms_table"], ms_back=last["ms_back"],
               ms_fwd=last["ms_fwd"], ms_acc=last["ms_acc"], flops=last["flops"], tflops=last["flops"] / (ms_cg * 1e-3) / 1e12,
               ms_basis_grad=ms_bg, ms_basis_grad_all=all_bg, ratio_to_basis_grad=ms_cg / ms_bg, val_is_basis_grads=bool(torch.equal(val, vg)),
               nan=int(torch.isnan(G).sum().item()), checksum=float(G.sum().item()))
    hp = min(npts, host_npts)
    if hp > 0:
        xh, ch = x[:hp].cpu().numpy(), c[:hp].cpu().numpy()
        t0 = time.perf_counter()
        _, ref = basis_core_grad_host(tt, xh, basis, ch)
        res["host_route_npts"] = hp
        res["host_route_ms"] = (time.perf_counter() - t0) * 1e3
        _, got = tt.basis_core_grad(xh, basis, ch, last["mode"])
        res["max_rel_diff_to_host_route"] = max(float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300)) for a, b in zip(got, ref))
    print(json.dumps(res))
    return tt, x, (val, G), res


def run_enrich(argv, device=0, repeats=5, tt=None):
    """enrich WORKLOAD NPTS [ADD] [MODE]: the workloads and modes of the basis sub-command, hat functions on every mode.  On seeded
    points and weights drawn on the device and in the same session: one warm-up and `repeats` timed TTCross.enrich calls through the
    device-pointer entry (each makes and destroys a new engine) and the same for basis_core_grad in the mode that ran -- the yardstick:
    one product over all points per core.  Prints one JSON line with the medians, the phases of ttx_basis_enrich_last (table, back,
    sketch, qr, asm), the share of the QR, the measured ratio and the ratio the flop counts predict."""
    import json
    import time
    import torch
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload, npts = argv[0], int(float(argv[1]))
    add = int(argv[2]) if len(argv) > 2 else 4
    mode = argv[3] if len(argv) > 3 else "auto"
    if tt is None:
        tt, _ = basis_train(workload, device=device)
    basis = [("linear", np.linspace(0.0, 1.0, int(nk))) if nk > 1 else ("cos", 0.0, 1.0) for nk in tt._n]
    dev = torch.device("cuda", device)
    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    x = torch.rand((npts, tt.d), dtype=torch.float64, device=dev, generator=g).contiguous()
    c = torch.randn(npts, dtype=torch.float64, device=dev, generator=g).contiguous()
    torch.cuda.synchronize(dev)
    info = {}

    def once():
        new, inf = tt.enrich(x, basis, c, add, 1, mode)
        info.update(inf)
        info["ranks"] = [int(v) for v in new.ranks()]
        new.close()

    def timed(call):
        call()                                      # warm-up
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            call()                                  # synchronises before it returns
            ms.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ms)), [round(v, 4) for v in ms]

    ms_en, all_en = timed(once)
    last = tt.enrich_last()
    ms_cg, all_cg = timed(lambda: tt.basis_core_grad(x, basis, c, last["mode"]))
    cg = tt.basis_core_grad_last()
    phases = {k: last[k] for k in ("ms_table", "ms_back", "ms_sketch", "ms_qr", "ms_asm")}
    res = dict(workload=workload, npts=npts, add=add, mode_asked=mode, mode=last["mode"], chunk=last["chunk"], d=tt.d, max_rank=int(tt.ranks().max()),
               added=int(sum(info["added"])), max_new_rank=max(info["ranks"]), ms_enrich=ms_en, ms_enrich_all=all_en, **phases,
               qr_share=last["ms_qr"] / max(sum(phases.values()), 1e-300), flops=last["flops"], ms_core_grad=ms_cg, ms_core_grad_all=all_cg,
               core_grad_chunk=cg["chunk"], ratio_to_core_grad=ms_en / ms_cg, ratio_by_flops=last["flops"] / max(cg["flops"], 1e-300))
    print(json.dumps(res))
    return res


def run_fit(argv, device=0, repeats=3, tt=None, basis=None, max_iter=4, cg_max=10):
    """fit WORKLOAD NPTS [MODE] [MAX_ITER] [CG_MAX]: the workloads and modes of the basis sub-command.  Takes the workload's train, evaluates it at NPTS
    seeded points (the targets), perturbs every entry of every core by up to 1 % (seeded) and fits it back with TTCross.fit on device
    tensors (max_iter iterations of at most cg_max CG passes).  Prints one JSON line: the history, the split of fit_last, the
    milliseconds per Gauss-Newton iteration, and -- in the same session, on the same points -- the medians of basis_batch,
    basis_grad_batch, basis_core_grad and basis_jvp (by flops the JVP is 3 value chains; the backward pass of basis_grad_batch is 2,
    with the same two accumulator sets)."""
    import json
    import time
    import torch
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload, npts = argv[0], int(float(argv[1]))
    mode = argv[2] if len(argv) > 2 else "auto"
    max_iter = int(argv[3]) if len(argv) > 3 else max_iter
    cg_max = int(argv[4]) if len(argv) > 4 else cg_max
    if tt is None:
        tt, basis = basis_train(workload, device=device)
    if basis is None:
        basis = [("linear", np.linspace(0.0, 1.0, int(nk))) if nk > 1 else ("cos", 0.0, 1.0) for nk in tt._n]
        lo, hi = 0.0, 1.0
    else:
        lo, hi = basis[1], basis[2]
    dev = torch.device("cuda", device)
    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    x = (lo + (hi - lo) * torch.rand((npts, tt.d), dtype=torch.float64, device=dev, generator=g)).contiguous()
    total = int(tt.core_offsets()[-1])
    truth = tt.cores_get(torch.empty(total, dtype=torch.float64, device=dev))
    v = torch.randn(total, dtype=torch.float64, device=dev, generator=g).contiguous()
    c = torch.randn(npts, dtype=torch.float64, device=dev, generator=g).contiguous()
    torch.cuda.synchronize(dev)

    def timed(call):
        out = call()                                # warm-up
        ms = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            out = call()                            # synchronises before it returns
            ms.append((time.perf_counter() - t0) * 1e3)
        return out, float(np.median(ms))

    # the values of some workloads' trains are tiny at real points (their squares underflow): the first core is scaled so that the
    # largest value at the points is 1, here and in `truth`; the train is put back as it was found at the end
    found = truth.clone()
    scale = 1.0 / float(tt.basis_batch(x, basis, mode).abs().max().item())
    truth[:int(tt.core_offsets()[1])] *= scale
    torch.cuda.synchronize(dev)
    tt.cores_set(truth)
    (_, dval), ms_jvp = timed(lambda: tt.basis_jvp(x, basis, v, mode))
    ran = tt.basis_jvp_last()["mode"]
    y, ms_val = timed(lambda: tt.basis_batch(x, basis, ran))
    _, ms_bg = timed(lambda: tt.basis_grad_batch(x, basis, ran))
    bg = tt.basis_grad_last()
    _, ms_cg = timed(lambda: tt.basis_core_grad(x, basis, c, ran))
    start = (truth * (1.0 + 0.01 * (2.0 * torch.rand(total, dtype=torch.float64, device=dev, generator=g) - 1.0))).contiguous()
    torch.cuda.synchronize(dev)
    tt.cores_set(start)
    t0 = time.perf_counter()
    h = tt.fit(x, basis, y, None, mode=ran, max_iter=max_iter, cg_max=cg_max, lambda0=1e-2, cg_tol=1e-3)
    ms_fit = (time.perf_counter() - t0) * 1e3
    last = tt.fit_last()
    tt.cores_set(found)                             # the workload's train is left as it was found
    res = dict(workload=workload, npts=npts, mode_asked=mode, mode=last["mode"], d=tt.d, max_rank=int(tt.ranks().max()), core_elements=total, scale=scale,
               loss=[float(t) for t in h["loss"]], lambda_=[float(t) for t in h["lambda_"]], cg_iters=[int(t) for t in h["cg_iters"]],
               accepted=[int(t) for t in h["accepted"]], iters=h["iters"], stop=h["stop"], ms_fit=ms_fit, ms_per_iteration=ms_fit / max(h["iters"], 1),
               ms_fit_jvp=last["ms_jvp"], ms_fit_core_grad=last["ms_core_grad"], ms_fit_value=last["ms_value"], ms_fit_vector=last["ms_vector"],
               n_jvp=last["n_jvp"], n_core_grad=last["n_core_grad"], ms_basis_jvp=ms_jvp, ms_basis_batch=ms_val, ms_basis_grad=ms_bg,
               ms_basis_grad_back=bg["ms_back"], ms_basis_core_grad=ms_cg, jvp_to_value=ms_jvp / ms_val, jvp_to_grad_back=ms_jvp / max(bg["ms_back"], 1e-300),
               nan=int(torch.isnan(dval).sum().item()))
    print(json.dumps(res))
    return tt, h, res


def sq_lognorm_grad_host(tt, md, mo=None, gvol=0.0, coef=1.0):
    """what a user does without ttx_sq_lognorm_grad: every core to the host with core(k), then the two Gram chains and the assembly
    as numpy einsums (each step scaled by its largest entry, so that long trains stay in range).  Returns (logz, [G_k])."""
    cores = [tt.core(k) for k in range(1, tt.d + 1)]
    d = len(cores)
    M = []
    for k in range(d):
        m = np.diag(np.asarray(md[k], dtype=np.float64))
        if mo is not None and mo[k] is not None and m.shape[0] > 1:
            o = np.asarray(mo[k], dtype=np.float64)[:m.shape[0] - 1]
            m = m + np.diag(o, 1) + np.diag(o, -1)
        M.append(m)
    V = [np.einsum("aib,ij->ajb", c, m) for c, m in zip(cores, M)]
    PL, PR, lL, lR = [np.ones((1, 1))], [None] * d + [np.ones((1, 1))], [0.0], [0.0] * (d + 1)
    for k in range(d):
        p = np.einsum("ac,aib,cid->bd", PL[k], cores[k], V[k], optimize=True)
        s = np.abs(p).max()
        PL.append(p / s)
        lL.append(lL[k] + np.log(s))
    for k in range(d - 1, 0, -1):
        p = np.einsum("bd,aib,cid->ac", PR[k + 1], cores[k], V[k], optimize=True)
        s = np.abs(p).max()
        PR[k] = p / s
        lR[k] = lR[k + 1] + np.log(s)
    logZ = lL[d] + np.log(PL[d][0, 0])
    logden = np.logaddexp(logZ, np.log(gvol)) if gvol > 0.0 else logZ
    G = [2.0 * coef * np.exp(lL[k] + lR[k + 1] - logden) * np.einsum("ac,cid,bd->aib", PL[k], V[k], PR[k + 1], optimize=True) for k in range(d)]
    return float(logden), G


def run_mle(argv, device=0, repeats=3, tt=None, max_iter=3, history=2):
    """mle WORKLOAD NPTS [MODE] [MAX_ITER]: the trains of the tijk sub-command, taken as the square root of a density on equidistant
    nodes of [0, 1].  First one JSON line of timings on the train as found: sq_lognorm_grad (call, the two chains and the assembly from
    sq_lognorm_grad_last, the assembly's traffic in bytes per second and as a share of the bandwidth probe at the same byte count), sq_nll at NPTS points drawn with sample_sq_real (the call, the
    normaliser's share of it), and in the same session the Gram chain of topk, the head pass of sample_sq_real and the host route
    (sq_lognorm_grad_host).  Then the fit: a weighted sample is drawn from the train with sample_sq_real (weights 1 +- 10 %, seeded),
    every core entry is perturbed by up to 1 % and fit_density refits it; one JSON line per trial with the nll, the normaliser's share
    of the call and the times, and a last line with the held-out nll before and after.  The train is put back as it was found."""
    import json
    import time
    import torch
    from .engine import mass_tridiag
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload, npts = argv[0], int(float(argv[1]))
    mode = argv[2] if len(argv) > 2 else "auto"
    max_iter = int(argv[3]) if len(argv) > 3 else max_iter
    tt = tt or tijk_train(workload, device=device)
    dev = torch.device("cuda", device)
    nodes = [np.linspace(0.0, 1.0, int(nk)) for nk in tt._n]
    lin = [("linear", t) for t in nodes]
    md, mo = mass_tridiag(nodes)
    gamma = 0.0
    total = int(tt.core_offsets()[-1])
    out = torch.empty(total, dtype=torch.float64, device=dev)

    def timed(call, last=None):
        res = call()                                # warm-up
        ms, lasts = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = call()                            # synchronises before it returns
            ms.append((time.perf_counter() - t0) * 1e3)
            lasts.append(last() if last else None)
        return res, float(np.median(ms)), lasts

    res, ms_call, lasts = timed(lambda: tt.sq_lognorm_grad(md, mo, 0.0, 1.0, out=out, mode=mode), tt.sq_lognorm_grad_last)
    med = {k: float(np.median([x[k] for x in lasts])) for k in ("ms_right", "ms_left", "ms_asm")}
    r = tt.ranks().astype(np.int64)
    asm_bytes = 8.0 * (2.0 * total + float(np.sum(r[1:] ** 2)))                 # W read, g written, every PR_k read once
    u = _seeded_uniforms(2 * npts, tt.d, dev)
    smp, ms_smp, slast = timed(lambda: tt.sample_sq_real(u, nodes, gamma=gamma, mode=mode), tt.sample_sq_real_last)
    fin = ~torch.isnan(smp["x"][:, 0])
    pts = smp["x"][fin]
    x, xh = pts[:npts].contiguous(), pts[npts:2 * npts].contiguous()
    g = torch.Generator(device=dev)
    g.manual_seed(20240611)
    w = (1.0 + 0.1 * (2.0 * torch.rand(x.shape[0], dtype=torch.float64, device=dev, generator=g) - 1.0)).contiguous()
    nres, ms_nll, nlast = timed(lambda: tt.sq_nll(x, lin, gamma, md, mo, 0.0, w, mode, out), tt.sq_lognorm_grad_last)
    ms_norm = float(np.median([sum(v[k] for k in ("ms_right", "ms_left", "ms_asm")) for v in nlast]))
    from .engine import k_residual_bench
    probe_ms, probe_bytes = k_residual_bench(max(1, int(asm_bytes / (8 * 64))), 64, 20, device=device)
    line = dict(workload=workload, npts=int(x.shape[0]), d=tt.d, max_rank=int(r.max()), core_elements=total, mode_asked=mode, mode=lasts[-1]["mode"],
                probe_bytes_per_s=probe_bytes / (probe_ms * 1e-3), asm_fraction_of_probe=(asm_bytes / (med["ms_asm"] * 1e-3)) / (probe_bytes / (probe_ms * 1e-3)) if med["ms_asm"] > 0 else None,
                flops=lasts[-1]["flops"], ms_lognorm_grad=ms_call, **med, asm_bytes_per_s=asm_bytes / (med["ms_asm"] * 1e-3) if med["ms_asm"] > 0 else None,
                logz=res["logz"], z_exp=res["z_exp"], ms_nll=ms_nll, nll=nres["nll"], ms_normaliser_in_nll=ms_norm, normaliser_share_of_nll=ms_norm / ms_nll,
                ms_sample_sq_real_head=float(np.median([v["ms_head"] for v in slast])), ms_sample_sq_real=ms_smp)
    try:
        _, ms_topk, tlast = timed(lambda: tt.topk(16, mode=mode), tt.topk_last)
        line["ms_topk_gram"] = float(np.median([v["ms_gram"] for v in tlast]))
    except Exception as e:                          # a train the search refuses still gives the other figures
        line["topk_error"] = str(e)[:200]
    t0 = time.perf_counter()
    hlz, hG = sq_lognorm_grad_host(tt, md, mo)
    line["host_route_ms"] = (time.perf_counter() - t0) * 1e3
    got = tt.sq_lognorm_grad(md, mo, 0.0, 1.0, mode=lasts[-1]["mode"])
    line["max_rel_diff_to_host_route"] = max(float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300)) for a, b in zip(got["g"], hG))
    line["logz_diff_to_host_route"] = abs(got["logz"] - hlz)
    print(json.dumps(line))
    if max_iter > 0:
        found = tt.cores_get(torch.empty(total, dtype=torch.float64, device=dev))
        held = lambda: tt.sq_nll(xh, lin, gamma, md, mo, 0.0, None, mode, out)["nll"]          # noqa: E731
        start = (found * (1.0 + 0.01 * (2.0 * torch.rand(total, dtype=torch.float64, device=dev, generator=g) - 1.0))).contiguous()
        torch.cuda.synchronize(dev)
        held_true = held()
        tt.cores_set(start)
        held_start = held()
        trials = []
        inner = tt.sq_nll

        def traced(*a, **k):
            t0 = time.perf_counter()
            rr = inner(*a, **k)
            ms = (time.perf_counter() - t0) * 1e3
            ll = tt.sq_lognorm_grad_last()
            trials.append(dict(nll=rr["nll"], ms_call=ms, ms_normaliser=ll["ms_right"] + ll["ms_left"] + ll["ms_asm"]))
            return rr
        tt.sq_nll = traced
        try:
            t0 = time.perf_counter()
            h = tt.fit_density(x, lin, gamma, md, mo, 0.0, w, mode, max_iter=max_iter, history=history)
            ms_fit = (time.perf_counter() - t0) * 1e3
        finally:
            del tt.sq_nll
        for j, t in enumerate(trials):
            acc = None if j == 0 else bool(h["hist"][j - 1][1])
            print(json.dumps(dict(trial=j, accepted=acc, nll=t["nll"], ms_call=t["ms_call"], ms_normaliser=t["ms_normaliser"], normaliser_share=t["ms_normaliser"] / t["ms_call"])))
        print(json.dumps(dict(workload=workload, iters=h["iters"], nll=h["nll"], ms_fit=ms_fit, held_out_nll_truth=held_true, held_out_nll_start=held_start, held_out_nll_end=held())))
        tt.cores_set(found)
    return tt, line


def sample_host(tt, u, w=None):
    """what a user does without ttx_sample: every core to the host with core(k), then the conditional marginals walked in
    numpy from the last mode to the first.  Returns (ind, logq, val) of the definition in include/ttx.h, in numpy's own
    summation order."""
    cores = [tt.core(k) for k in range(1, tt.d + 1)]
    w = [np.ones(c.shape[1]) for c in cores] if w is None else [np.asarray(q, dtype=np.float64) for q in w]
    u = np.asarray(u, dtype=np.float64)
    npts, d = u.shape
    lv, heads = np.ones(1), []
    for c, q in zip(cores, w):
        heads.append(np.einsum("a,aib->ib", lv, c) * q[:, None])
        lv = lv @ np.einsum("aib,i->ab", c, q)
    x = np.ones((npts, 1))
    ind, logq, rows = np.zeros((npts, d), dtype=np.int32), np.zeros(npts), np.arange(npts)
    for k in range(d - 1, -1, -1):
        p = np.abs(x @ heads[k].T)
        c = np.cumsum(p, axis=1)
        hit = (p > 0) & (u[:, k:k + 1] * c[:, -1:] < c)
        i = np.where(hit.any(1), hit.argmax(1), p.shape[1] - 1 - (p[:, ::-1] > 0).argmax(1))
        logq += np.log(p[rows, i] / c[:, -1])
        ind[:, k] = i + 1
        x = np.einsum("asb,sb->sa", cores[k][:, i, :], x)
    return ind, logq, x[:, 0]


def _seeded_uniforms(npts, d, dev):
    """the (npts, d) uniforms of the sampling sub-commands, made ON the device from their fixed seed"""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(20240607)
    u = torch.rand((npts, d), dtype=torch.float64, device=dev, generator=g)
    torch.cuda.synchronize(dev)
    return u


def _timed_calls(call, last, repeats):
    """One warm-up of call(), then `repeats` timed calls, each followed by last() (a sampler's *_last): the last result, the median
    of the calls' ms, the medians of last()'s float figures, and the last record."""
    import time
    call()
    ms, figs = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = call()                          # synchronises before it returns
        ms.append((time.perf_counter() - t0) * 1e3)
        figs.append(last())
    return res, float(np.median(ms)), {k: float(np.median([f[k] for f in figs])) for k in figs[0] if isinstance(figs[0][k], float)}, figs[-1]


def run_sample(argv, device=0, repeats=5, tt=None, host_npts=1000):
    """sample WORKLOAD NPTS[,NPTS...]: the trains of the tijk sub-command, weights 1 / n, seeded uniforms made ON the device; per
    sample count one warm-up and the median of `repeats` calls through the device-pointer entry: the call, the two kernels
    (HIP events, ttx_sample_last), k_sm_head's bytes / s next to the bandwidth probe at the same byte count, samples per second
    of k_sm_draw, and tijk_batch(ind, "exact") on the drawn indices; then the host route sample_host once at host_npts
    samples.  Prints one JSON line per sample count."""
    import json
    import time
    import torch
    from . import engine as E
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload = argv[0]
    tt = tt or tijk_train(workload, device=device)
    dev = torch.device("cuda", device)
    w = [np.full(int(nk), 1.0 / int(nk)) for nk in tt._n]
    out = []
    for npts in [int(float(x)) for x in argv[1].split(",")]:
        u = _seeded_uniforms(npts, tt.d, dev)
        res, call_ms, med, last = _timed_calls(lambda: tt.sample(u, w), tt.sample_last, repeats)
        head, draw, by = med["ms_head"], med["ms_draw"], last["bytes_head"]
        probe_ms, probe_by = E.k_residual_bench(max(int(by // 512), 1), 64, 20, device=device)
        tt.tijk_batch(res["ind"], "exact")
        tj = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            val = tt.tijk_batch(res["ind"], "exact")
            tj.append((time.perf_counter() - t0) * 1e3)
        tijk = float(np.median(tj))
        r = dict(workload=workload, npts=npts, d=tt.d, max_rank=int(tt.ranks().max()), call_ms=call_ms, head_ms=head,
                 head_bytes=by, head_bytes_per_s=by / (head * 1e-3) if head > 0 else None,
                 probe_bytes_per_s=probe_by / (probe_ms * 1e-3) if probe_ms > 0 else None, draw_ms=draw,
                 draw_samples_per_s=npts / (draw * 1e-3) if draw > 0 else None, tijk_exact_ms=tijk,
                 tijk_points_per_s=npts / (tijk * 1e-3) if tijk > 0 else None, draw_over_tijk=draw / tijk if tijk > 0 else None,
                 failed=last["failed"], val_is_tijk=bool(torch.equal(val, res["val"])), mean_logq=float(res["logq"].mean().item()))
        if r["head_bytes_per_s"] and r["probe_bytes_per_s"]:
            r["head_fraction_of_probe"] = r["head_bytes_per_s"] / r["probe_bytes_per_s"]
        print(json.dumps(r), flush=True)
        out.append(r)
    uh = np.random.default_rng(7).random((host_npts, tt.d))
    t0 = time.perf_counter()
    hi, hq, hv = sample_host(tt, uh, w)
    host_ms = (time.perf_counter() - t0) * 1e3
    di = tt.sample(uh, w)["ind"]
    r = dict(workload=workload, host_route_npts=host_npts, host_route_ms=host_ms, host_samples_per_s=host_npts / (host_ms * 1e-3),
             host_rows_equal_device=int(np.all(hi == di, axis=1).sum()))
    print(json.dumps(r), flush=True)
    out.append(r)
    return out


def signed_density_train(device=0, d=6, n=33):
    """A density with the sign changes a cross approximation leaves in its tails: two separable Gaussian bumps on [0, 1]^d minus a
    small constant, as a rank-3 train.  Negative on most of the grid by count, positive where the mass is."""
    t = np.linspace(0.0, 1.0, n)
    parts = [[np.exp(-0.5 * ((t - 0.35) / 0.08) ** 2)] * d, [0.6 * np.exp(-0.5 * ((t - 0.7) / 0.06) ** 2)] + [np.exp(-0.5 * ((t - 0.7) / 0.06) ** 2)] * (d - 1),
             [-2e-3 * np.ones(n)] + [np.ones(n)] * (d - 1)]
    cores = []
    for k in range(d):
        r0, r1 = (1 if k == 0 else 3), (1 if k == d - 1 else 3)
        c = np.zeros((r0, n, r1))
        for j in range(3):
            c[0 if k == 0 else j, :, 0 if k == d - 1 else j] = parts[j][k]
        cores.append(c)
    return TTCross.from_cores(cores, device=device)


def sample_sq_host(tt, u, w=None, gamma=0.0):
    """what a user does without ttx_sample_sq: every core to the host with core(k), the factors of the weighted prefix Gram matrices by
    numpy's QR, then the conditionals of the square walked in numpy from the last mode to the first.  Returns (ind, logq, val)."""
    cores = [tt.core(k) for k in range(1, tt.d + 1)]
    w = [np.ones(c.shape[1]) for c in cores] if w is None else [np.asarray(q, dtype=np.float64) for q in w]
    u = np.asarray(u, dtype=np.float64)
    npts, d = u.shape
    F, g, H, gs = np.ones((1, 1)), float(gamma), [], []
    for c, q in zip(cores, w):
        H.append(np.tensordot(F, c, axes=([1], [0])))
        gs.append(g)
        A = (np.sqrt(q)[None, :, None] * H[-1]).reshape(-1, c.shape[2])
        F = np.linalg.qr(A, mode="r") if A.shape[0] > A.shape[1] else A
        m = np.abs(F).max()
        ex = int(np.frexp(m)[1]) if m > 0 and np.isfinite(m) else 0
        F, g = np.ldexp(F, -ex), g * q.sum() * 4.0 ** -ex
    x = np.ones((npts, 1))
    ind, logq, rows = np.zeros((npts, d), dtype=np.int32), np.zeros(npts), np.arange(npts)
    for k in range(d - 1, -1, -1):
        m = np.tensordot(H[k], x, axes=([2], [1]))                 # (a, i, sample)
        p = w[k][None, :] * ((m * m).sum(0).T + gs[k])
        c = np.cumsum(p, axis=1)
        hit = (p > 0) & (u[:, k:k + 1] * c[:, -1:] < c)
        i = np.where(hit.any(1), hit.argmax(1), p.shape[1] - 1 - (p[:, ::-1] > 0).argmax(1))
        logq += np.log(p[rows, i] / c[:, -1])
        ind[:, k] = i + 1
        x = np.einsum("asb,sb->sa", cores[k][:, i, :], x)
    return ind, logq, x[:, 0]


def run_samplesq(argv, device=0, repeats=5, tt=None, host_npts=1000):
    """samplesq WORKLOAD NPTS [MODE] [REPEATS]: the trains of the sample sub-command (or "signed": signed_density_train), weights 1 / n, seeded
    uniforms made ON the device; one warm-up and the median of `repeats` calls of sample_sq through the device-pointer entry: the
    call, the head pass, the rows kernels and the picks (HIP events, ttx_sample_sq_last), samples per second and the fp64 rate of
    the rows; sample() on the same uniforms and train next to it; then the host route sample_sq_host once at host_npts samples.
    On the signed workload the target is |T| / Z: the largest importance weight |T| / q over its mean under sample() on T and under
    sample_sq() on the cross approximation of sqrt |T| (of_trains, sqrtabs), with and without a defensive term.  One JSON line each."""
    import json
    import time
    import torch
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload, npts = argv[0], int(float(argv[1]))
    mode = argv[2] if len(argv) > 2 else "auto"
    repeats = int(argv[3]) if len(argv) > 3 else repeats
    tt = tt or (signed_density_train(device) if workload == "signed" else tijk_train(workload, device=device))
    dev = torch.device("cuda", device)
    w = [np.full(int(nk), 1.0 / int(nk)) for nk in tt._n]
    u = _seeded_uniforms(npts, tt.d, dev)

    res, call_ms, med, last = _timed_calls(lambda: tt.sample_sq(u, w, mode=mode), tt.sample_sq_last, repeats)
    val = tt.tijk_batch(res["ind"], "exact")
    _, s_ms, s_med, s_last = _timed_calls(lambda: tt.sample(u, w), tt.sample_last, repeats)
    rows_ms = med["ms_rows"]
    out = [dict(workload=workload, npts=npts, d=tt.d, max_rank=int(tt.ranks().max()), mode_asked=mode, mode=last["mode"], call_ms=call_ms,
                head_ms=med["ms_head"], rows_ms=rows_ms, pick_ms=med["ms_pick"], samples_per_s=npts / (call_ms * 1e-3), rows_flops=last["flops"],
                rows_flops_per_s=last["flops"] / (rows_ms * 1e-3) if rows_ms > 0 else None, failed=last["failed"],
                val_is_tijk=bool(torch.equal(val, res["val"])), mean_logq=float(res["logq"].mean().item()),
                sample_call_ms=s_ms, sample_head_ms=s_med["ms_head"], sample_draw_ms=s_med["ms_draw"], time_ratio_to_sample=call_ms / s_ms if s_ms > 0 else None)]
    print(json.dumps(out[0]), flush=True)
    uh = np.random.default_rng(7).random((host_npts, tt.d))
    t0 = time.perf_counter()
    hi, hq, hv = sample_sq_host(tt, uh, w)
    host_ms = (time.perf_counter() - t0) * 1e3
    di = tt.sample_sq(uh, w, mode="exact")["ind"]
    out.append(dict(workload=workload, host_route_npts=host_npts, host_route_ms=host_ms, host_samples_per_s=host_npts / (host_ms * 1e-3),
                    host_rows_equal_device=int(np.all(hi == di, axis=1).sum())))
    print(json.dumps(out[-1]), flush=True)
    if workload == "signed":
        def spread(ind, logq):
            iw = torch.abs(tt.tijk_batch(ind, "exact")) / torch.exp(logq)
            return float((iw.max() / iw.mean()).item()), float((iw.sum() ** 2 / (iw * iw).sum() / iw.numel()).item())
        plain = tt.sample(u, w)
        root = TTCross.of_trains([tt], "sqrtabs", 12, accuracy=500 * EPS, pivoting=2, quad=w, device=device).run()
        r = dict(workload=workload, npts=npts, root_max_rank=int(root.ranks().max()))
        r["sample_max_over_mean"], r["sample_ess_fraction"] = spread(plain["ind"], plain["logq"])
        for gam in (0.0, 1e-6):
            sq = root.sample_sq(u, w, gamma=gam, mode=mode)
            key = "sample_sq" if gam == 0.0 else "sample_sq_gamma_%g" % gam
            r[key + "_max_over_mean"], r[key + "_ess_fraction"] = spread(sq["ind"], sq["logq"])
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def sample_real_host(tt, u, nodes):
    """what a user does without ttx_sample_real: every core to the host with core(k), then the interpolated conditionals walked in
    numpy from the last mode to the first and inverted cell by cell.  Returns (x, logq, val) of the definition in include/ttx.h,
    in numpy's own summation order (all modes drawn, at least two nodes each)."""
    cores = [tt.core(k) for k in range(1, tt.d + 1)]
    nodes = [np.asarray(t, dtype=np.float64) for t in nodes]
    u = np.asarray(u, dtype=np.float64)
    npts, d = u.shape
    lv, heads = np.ones(1), []
    for c, t in zip(cores, nodes):
        om = np.concatenate([[t[1] - t[0]], t[2:] - t[:-2], [t[-1] - t[-2]]]) * 0.5
        heads.append(np.einsum("a,aib->ib", lv, c))
        lv = lv @ np.einsum("aib,i->ab", c, om)
    st = np.ones((npts, 1))
    x, logq, rows = np.zeros((npts, d)), np.zeros(npts), np.arange(npts)
    for k in range(d - 1, -1, -1):
        t = nodes[k]
        h = np.diff(t)
        p = np.abs(st @ heads[k].T)
        A = 0.5 * (p[:, :-1] + p[:, 1:]) * h
        C = np.cumsum(A, axis=1)
        T = u[:, k] * C[:, -1]
        hit = (A > 0) & (T[:, None] < C)
        j = np.where(hit.any(1), hit.argmax(1), A.shape[1] - 1 - (A[:, ::-1] > 0).argmax(1))
        p0, p1 = p[rows, j], p[rows, j + 1]
        sp = np.clip(T - np.where(j > 0, C[rows, np.maximum(j - 1, 0)], 0.0), 0.0, A[rows, j]) / h[j]
        den = p0 + np.sqrt(np.maximum(p0 * p0 + 2.0 * (p1 - p0) * sp, 0.0))
        lam = np.where(hit.any(1), np.clip(2.0 * sp / np.where(den > 0, den, 1.0), 0.0, 1.0), 1.0)
        xk = np.clip(t[j] + lam * h[j], t[j], t[j + 1])
        i = np.clip(np.searchsorted(t, xk, side="right") - 1, 0, t.size - 2)
        f1 = (xk - t[i]) / (t[i + 1] - t[i])
        f0 = 1.0 - f1
        logq += np.log((f0 * p[rows, i] + f1 * p[rows, i + 1]) / C[:, -1])
        x[:, k] = xk
        st = f0[:, None] * np.einsum("asb,sb->sa", cores[k][:, i, :], st) + f1[:, None] * np.einsum("asb,sb->sa", cores[k][:, i + 1, :], st)
    return x, logq, st[:, 0]


def run_samplereal(argv, device=0, repeats=5, tt=None, host_npts=1000):
    """samplereal WORKLOAD NPTS[,NPTS...]: the trains of the sample sub-command on equidistant nodes of [0, 1], seeded uniforms made
    ON the device; per sample count one warm-up and the median of `repeats` calls through the device-pointer entry: the call and
    its two kernels (HIP events, ttx_sample_real_last); sample() on the same u with its two kernels, k_sr_draw over k_sm_draw
    next to the derived work ratio sum (n r1 + 2 r0 r1) / sum (n r1 + r0 r1); basis_batch(x, linear, "exact") on the drawn points
    (one call after a small warm-up, on as many of them as 2e13 flops of its dense chain allow), the cost of forming val separately; then the host route sample_real_host once at host_npts samples.  Prints one JSON line
    per sample count."""
    import json
    import time
    import torch
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload = argv[0]
    tt = tt or tijk_train(workload, device=device)
    dev = torch.device("cuda", device)
    nodes = [np.linspace(0.0, 1.0, int(nk)) for nk in tt._n]
    lin = [("linear", t) for t in nodes]
    w = [np.full(int(nk), 1.0 / int(nk)) for nk in tt._n]
    r = [int(q) for q in tt.ranks()]
    flops_pt = 2.0 * sum(r[k] * int(nk) * r[k + 1] for k, nk in enumerate(tt._n))
    work = sum(int(nk) * r[k + 1] + 2 * r[k] * r[k + 1] for k, nk in enumerate(tt._n)) / sum(int(nk) * r[k + 1] + r[k] * r[k + 1] for k, nk in enumerate(tt._n))
    out = []
    for npts in [int(float(x)) for x in argv[1].split(",")]:
        u = _seeded_uniforms(npts, tt.d, dev)
        res, call_ms, med, last = _timed_calls(lambda: tt.sample_real(u, nodes), tt.sample_real_last, repeats)
        _, _, sm, _ = _timed_calls(lambda: tt.sample(u, w), tt.sample_last, repeats)
        fin = ~torch.isnan(res["x"][:, 0])
        nb = min(int(fin.sum().item()), max(1000, int(2e13 / flops_pt)))     # the dense exact chain costs flops_pt per point: at most 2e13 flops are timed
        xs, vs = res["x"][fin][:nb].contiguous(), res["val"][fin][:nb]
        tt.basis_batch(xs[:64].contiguous(), lin, "exact")
        t0 = time.perf_counter()
        val = tt.basis_batch(xs, lin, "exact")
        basis = (time.perf_counter() - t0) * 1e3
        head, draw, sm_head, sm_draw = med["ms_head"], med["ms_draw"], sm["ms_head"], sm["ms_draw"]
        rec = dict(workload=workload, npts=npts, d=tt.d, max_rank=max(r), call_ms=call_ms, head_ms=head, draw_ms=draw,
                   draw_samples_per_s=npts / (draw * 1e-3) if draw > 0 else None, sample_head_ms=sm_head, sample_draw_ms=sm_draw,
                   draw_over_sample_draw=draw / sm_draw if sm_draw > 0 else None, work_ratio=work,
                   time_over_work=draw / sm_draw / work if sm_draw > 0 else None, basis_exact_npts=nb, basis_exact_ms=basis,
                   draw_us_per_sample=draw * 1e3 / npts, basis_exact_us_per_point=basis * 1e3 / nb if nb else None, failed=last["failed"],
                   val_is_basis=bool(torch.all(val == vs).item()), mean_logq=float(res["logq"][fin].mean().item()))
        print(json.dumps(rec), flush=True)
        out.append(rec)
    uh = np.random.default_rng(7).random((host_npts, tt.d))
    t0 = time.perf_counter()
    hx, hq, hv = sample_real_host(tt, uh, nodes)
    host_ms = (time.perf_counter() - t0) * 1e3
    dx = tt.sample_real(uh, nodes)
    with np.errstate(all="ignore"):
        rec = dict(workload=workload, host_route_npts=host_npts, host_route_ms=host_ms, host_samples_per_s=host_npts / (host_ms * 1e-3),
                   host_max_abs_dx=float(np.nanmax(np.abs(hx - dx["x"]))), host_max_abs_dlogq=float(np.nanmax(np.abs(hq - dx["logq"]))))
    print(json.dumps(rec), flush=True)
    out.append(rec)
    return out


def run_samplesqreal(argv, device=0, repeats=5, tt=None):
    """samplesqreal WORKLOAD NPTS [MODE] [REPEATS]: the trains of the sample sub-command (or "signed": signed_density_train) on equidistant
    nodes of [0, 1], seeded uniforms made ON the device; one warm-up and the median of `repeats` calls of sample_sq_real through the
    device-pointer entry: the call, the head pass, the rows kernels and the picks with the chain steps (HIP events,
    ttx_sample_sq_real_last), samples per second and the fp64 rate of the rows; sample_sq (weights 1 / n) and sample_real on the same
    uniforms and train next to it, with the time ratios.  On the signed workload the target is |g| / Z on the box: the largest
    importance weight |g(x)| / q(x) over its mean and the effective sample size under sample_real() on the train and under
    sample_sq_real() on the cross approximation of sqrt |T| (of_trains, sqrtabs), with and without a defensive term.  One JSON line each."""
    import json
    import torch
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload, npts = argv[0], int(float(argv[1]))
    mode = argv[2] if len(argv) > 2 else "auto"
    repeats = int(argv[3]) if len(argv) > 3 else repeats
    tt = tt or (signed_density_train(device) if workload == "signed" else tijk_train(workload, device=device))
    dev = torch.device("cuda", device)
    nodes = [np.linspace(0.0, 1.0, int(nk)) for nk in tt._n]
    lin = [("linear", t) for t in nodes]
    w = [np.full(int(nk), 1.0 / int(nk)) for nk in tt._n]
    u = _seeded_uniforms(npts, tt.d, dev)

    res, call_ms, med, last = _timed_calls(lambda: tt.sample_sq_real(u, nodes, mode=mode), tt.sample_sq_real_last, repeats)
    fin = ~torch.isnan(res["x"][:, 0])
    nb = min(int(fin.sum().item()), 100000)
    val = tt.basis_batch(res["x"][fin][:nb].contiguous(), lin, "exact")
    _, q_ms, q_med, q_last = _timed_calls(lambda: tt.sample_sq(u, w, mode=mode), tt.sample_sq_last, repeats)
    _, r_ms, r_med, r_last = _timed_calls(lambda: tt.sample_real(u, nodes), tt.sample_real_last, repeats)
    rows_ms, q_rows_ms = med["ms_rows"], q_med["ms_rows"]
    out = [dict(workload=workload, npts=npts, d=tt.d, max_rank=int(tt.ranks().max()), mode_asked=mode, mode=last["mode"], call_ms=call_ms,
                head_ms=med["ms_head"], rows_ms=rows_ms, pick_ms=med["ms_pick"], samples_per_s=npts / (call_ms * 1e-3), rows_flops=last["flops"],
                rows_flops_per_s=last["flops"] / (rows_ms * 1e-3) if rows_ms > 0 else None, failed=last["failed"],
                val_is_basis=bool(torch.all(val == res["val"][fin][:nb]).item()), mean_logq=float(res["logq"][fin].mean().item()),
                sample_sq_call_ms=q_ms, sample_sq_rows_ms=q_rows_ms, sample_sq_mode=q_last["mode"],
                sample_sq_rows_flops_per_s=q_last["flops"] / (q_rows_ms * 1e-3) if q_rows_ms > 0 else None,
                rows_rate_over_sample_sq=(q_rows_ms / rows_ms) if rows_ms > 0 else None, time_ratio_to_sample_sq=call_ms / q_ms if q_ms > 0 else None,
                sample_real_call_ms=r_ms, sample_real_draw_ms=r_med["ms_draw"], time_ratio_to_sample_real=call_ms / r_ms if r_ms > 0 else None)]
    print(json.dumps(out[0]), flush=True)
    if workload == "signed":
        def spread(x, logq):
            ok = torch.isfinite(logq)
            iw = torch.abs(tt.basis_batch(x[ok].contiguous(), lin, "exact")) / torch.exp(logq[ok])
            return float((iw.max() / iw.mean()).item()), float((iw.sum() ** 2 / (iw * iw).sum() / iw.numel()).item())
        plain = tt.sample_real(u, nodes)
        root = TTCross.of_trains([tt], "sqrtabs", 12, accuracy=500 * EPS, pivoting=2, quad=w, device=device).run()
        r = dict(workload=workload, npts=npts, root_max_rank=int(root.ranks().max()))
        r["sample_real_max_over_mean"], r["sample_real_ess_fraction"] = spread(plain["x"], plain["logq"])
        for gam in (0.0, 1e-6):
            sq = root.sample_sq_real(u, nodes, gamma=gam, mode=mode)
            key = "sample_sq_real" if gam == 0.0 else "sample_sq_real_gamma_%g" % gam
            r[key + "_max_over_mean"], r[key + "_ess_fraction"] = spread(sq["x"], sq["logq"])
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def run_rosenblatt(argv, device=0, repeats=5, tt=None):
    """rosenblatt WORKLOAD NPTS [MODE] [REPEATS]: the way back of samplesqreal on the same trains, nodes and seeded device-made uniforms.
    The points x are drawn with sample_sq_real (one warm-up and the median of `repeats` calls: the yardstick of the same session), then
    rosenblatt_sq_real maps them back through the device-pointer entry, timed alike: the call, the head pass, the rows kernels and
    k_sqr_cdf with the chain steps (HIP events, ttx_rosenblatt_sq_real_last), points per second, the fp64 rate of the rows next to the
    sampler's, ms_cdf over the sampler's ms_pick, the largest |u' - min(u, 1)| over the points that did not fail and whether logq and
    val repeated bit for bit.  One JSON line."""
    import json
    import torch
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload, npts = argv[0], int(float(argv[1]))
    mode = argv[2] if len(argv) > 2 else "auto"
    repeats = int(argv[3]) if len(argv) > 3 else repeats
    tt = tt or (signed_density_train(device) if workload == "signed" else tijk_train(workload, device=device))
    dev = torch.device("cuda", device)
    nodes = [np.linspace(0.0, 1.0, int(nk)) for nk in tt._n]
    u = _seeded_uniforms(npts, tt.d, dev)
    s, s_ms, s_med, s_last = _timed_calls(lambda: tt.sample_sq_real(u, nodes, mode=mode), tt.sample_sq_real_last, repeats)
    x = s["x"].contiguous()
    f, call_ms, med, last = _timed_calls(lambda: tt.rosenblatt_sq_real(x, nodes, mode=mode), tt.rosenblatt_sq_real_last, repeats)
    ok = ~torch.isnan(f["u"][:, 0])
    drawn = torch.tensor([int(nk) > 1 for nk in tt._n], device=dev)
    err = torch.abs(f["u"] - torch.clamp(u, max=1.0))[ok][:, drawn]
    same = lambda a, b: bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))
    rows_ms, s_rows_ms = med["ms_rows"], s_med["ms_rows"]
    rec = dict(workload=workload, npts=npts, d=tt.d, max_rank=int(tt.ranks().max()), mode_asked=mode, mode=last["mode"], call_ms=call_ms,
               ms_head=med["ms_head"], ms_rows=rows_ms, ms_cdf=med["ms_cdf"], points_per_s=npts / (call_ms * 1e-3), rows_flops=last["flops"],
               rows_flops_per_s=last["flops"] / (rows_ms * 1e-3) if rows_ms > 0 else None, failed=last["failed"],
               max_round_trip_error=float(err.max().item()) if err.numel() else None, logq_repeats=same(f["logq"], s["logq"]), val_repeats=same(f["val"], s["val"]),
               sample_sq_real_call_ms=s_ms, sample_sq_real_ms_head=s_med["ms_head"], sample_sq_real_ms_rows=s_rows_ms, sample_sq_real_ms_pick=s_med["ms_pick"],
               sample_sq_real_rows_flops_per_s=s_last["flops"] / (s_rows_ms * 1e-3) if s_rows_ms > 0 else None, sample_sq_real_failed=s_last["failed"],
               cdf_over_pick=med["ms_cdf"] / s_med["ms_pick"] if s_med["ms_pick"] > 0 else None, time_ratio_to_sample_sq_real=call_ms / s_ms if s_ms > 0 else None)
    print(json.dumps(rec), flush=True)
    return [rec]


def topk_train(workload, device=0):
    """The train of a topk run: a train of the tijk sub-command, or d64diff: the difference lincomb([1, -1], [exact, fast]) of the
    D_64 result trains in the two arithmetics, whose largest element is the max-norm error of the fast arithmetic; NAME+ort: the
    train NAME after ort().  The raw result trains are badly conditioned (elements of 1e10 at slice norms of 1e44), so their Gram
    scores are dominated by rounding; orthogonalise before a search that is to prove anything."""
    if workload.endswith("+ort"):                      # orthogonalised first: P becomes a multiple of the identity, the scores are as accurate as the chain
        return topk_train(workload[:-4], device=device).ort()
    if workload != "d64diff":
        return tijk_train(workload, device=device)
    kind, m, n, r, piv = TIJK_WORKLOADS["d64"]
    s = ising_setup(kind, m, n)
    both = [TTCross(s["n"], s["fun_id"], s["par"], r, pivoting=piv, accuracy=s["acc"], quad=s["quad"], tru=s["tru"], nproc=8, device=device,
                    arith=a).run() for a in ("exact", "fast")]
    return TTCross.lincomb([1.0, -1.0], both)


def topk_host(tt, k):
    """what a user does without ttx_topk: every core to the host with core(k), then the numpy search of tests/topk_ref.py (of this
    tree; None where the file is missing)"""
    tests = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
    if not os.path.exists(os.path.join(tests, "topk_ref.py")):
        return None
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import topk_ref
    return topk_ref.search([tt.core(j) for j in range(1, tt.d + 1)], k)


def run_topk(argv, device=0, repeats=5, tt=None, host_kmax=4096):
    """topk WORKLOAD K[,K...] [MODE] [HOST_KMAX]: the train of the workload (topk_train), per K one warm-up and `repeats` calls of
    the search: the best rows, bound and certificate, the median of the call and of the three times of ttx_topk_last, the achieved
    flop rate of the scoring launches; then, for K <= HOST_KMAX, the host route topk_host once and whether its rows are the
    device's.  Prints one JSON line per K."""
    import json
    import time
    workload, mode = argv[0], argv[2] if len(argv) > 2 else "auto"
    if len(argv) > 3:
        host_kmax = int(argv[3])
    tt = tt or topk_train(workload, device=device)
    out = []
    for k in [int(float(x)) for x in argv[1].split(",")]:
        res = tt.topk(k, mode=mode)
        ms, last = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = tt.topk(k, mode=mode)                # synchronises before it returns
            ms.append((time.perf_counter() - t0) * 1e3)
            last.append(tt.topk_last())
        gram, score, sel = (float(np.median([x[key] for x in last])) for key in ("ms_gram", "ms_score", "ms_select"))
        r = dict(workload=workload, k=k, mode_asked=mode, mode=last[-1]["mode"], d=tt.d, max_rank=int(tt.ranks().max()), nfound=int(res["ind"].shape[0]),
                 call_ms=float(np.median(ms)), gram_ms=gram, score_ms=score, select_ms=sel, flops=last[-1]["flops"],
                 score_flops_per_s=last[-1]["flops"] / (score * 1e-3) if score > 0 else None,
                 best=[dict(ind=res["ind"][j].tolist(), val=float(res["val"][j])) for j in range(min(3, res["ind"].shape[0]))],
                 bound=res["bound"], certified=res["certified"])
        if k <= host_kmax:
            t0 = time.perf_counter()
            ref = topk_host(tt, k)
            if ref is not None:
                r.update(host_route_ms=(time.perf_counter() - t0) * 1e3, host_rows_equal_device=bool(np.array_equal(ref["ind"], res["ind"])),
                         host_bound=ref["bound"])
        print(json.dumps(r), flush=True)
        out.append(r)
    return out


def roundsum_terms(tt, m):
    """m terms from one train: the train itself, then its cyclic shifts by t along mode 1 + (t mod d) (mode_apply with a permutation
    matrix in "exact" mode: the cores are copies), with the coefficients 2^-t"""
    terms, coefs = [tt], [1.0]
    for t in range(1, m):
        k = t % tt.d
        n = int(tt._n[k])
        P = np.roll(np.eye(n), (t // tt.d + 1) % n, axis=0)
        terms.append(tt.mode_apply({k + 1: P}, "exact"))
        coefs.append(2.0 ** -t)
    return coefs, terms


def roundsum_tree(coefs, terms, rank):
    """what the library could do before lincomb_round: a pairwise tree of lincomb, each result rounded to `rank` by svd(0, rank);
    None where a pair's ranks add up to more than 128"""
    level = [TTCross.lincomb([c], [x]) for c, x in zip(coefs, terms)]
    while len(level) > 1:
        if any(int((level[j].ranks() + level[j + 1].ranks())[1:-1].max()) > 128 for j in range(0, len(level) - 1, 2)):
            for x in level:
                x.close()
            return None
        nxt = []
        for j in range(0, len(level) - 1, 2):
            s = TTCross.lincomb([1.0, 1.0], [level[j], level[j + 1]])
            s.svd(0.0, rank)
            nxt.append(s)
            level[j].close()
            level[j + 1].close()
        if len(level) % 2:
            nxt.append(level[-1])
        level = nxt
    return level[0]


def run_roundsum(argv, device=0, repeats=5, tt=None, tree=True):
    """roundsum WORKLOAD M [RANK] [MODE]: M terms from the workload's train (roundsum_terms; a train of the tijk sub-command),
    lincomb_round at sketch rank RANK (default 64) without truncation: one warm-up and `repeats` calls -- the ranks, the median of
    the call and of the four times of ttx_roundsum_last, the achieved fp64 rate of the products; dist to the exact lincomb where
    its ranks fit 128, relative to its norm; the pairwise lincomb + svd tree at the same rank where it fits (tree=False: left out; it takes seconds to minutes).  One JSON line."""
    import json
    import time
    workload, m = argv[0], int(argv[1])
    rank = int(argv[2]) if len(argv) > 2 else 64
    mode = argv[3] if len(argv) > 3 else "auto"
    tt = tt or tijk_train(workload, device=device)
    coefs, terms = roundsum_terms(tt, m)
    TTCross.lincomb_round(coefs, terms, rank=rank, mode=mode).close()
    ms, last = [], []
    for rep in range(repeats):
        t0 = time.perf_counter()
        res = TTCross.lincomb_round(coefs, terms, rank=rank, mode=mode)        # synchronises before it returns
        ms.append((time.perf_counter() - t0) * 1e3)
        last.append(tt.roundsum_last())
        if rep < repeats - 1:
            res.close()
    med = {key: float(np.median([x[key] for x in last])) for key in ("ms_sketch", "ms_gemm", "ms_qr", "ms_advance")}
    prod = med["ms_sketch"] + med["ms_gemm"] + med["ms_advance"]
    r = dict(workload=workload, m=m, rank=rank, mode_asked=mode, mode=last[-1]["mode"], d=tt.d, term_max_rank=int(tt.ranks().max()),
             rank_sum=int(sum(int(x.ranks().max()) for x in terms)), ranks_max=int(res.ranks().max()), call_ms=float(np.median(ms)),
             call_ms_min=float(min(ms)), call_ms_max=float(max(ms)), flops=last[-1]["flops"],
             product_flops_per_s=last[-1]["flops"] / (prod * 1e-3) if prod > 0 else None, **med)
    if r["rank_sum"] + r["ranks_max"] <= 128:                                   # dist is a lincomb of the two itself
        full = TTCross.lincomb(coefs, terms)
        r["dist_over_norm"] = res.dist(full) / full.norm()
        full.close()
    t0 = time.perf_counter()
    tree = roundsum_tree(coefs, terms, rank) if tree else None
    if tree is not None:
        r["tree_ms"] = (time.perf_counter() - t0) * 1e3
        if int((res.ranks() + tree.ranks()).max()) <= 128:
            r["tree_dist_over_norm"] = res.dist(tree) / tree.norm()
        tree.close()
    res.close()
    for x in terms[1:]:
        x.close()
    print(json.dumps(r), flush=True)
    return r


def run_dirt(argv, device=0, npts=1 << 14, gamma=1e-4, keep=False):
    """dirt D N R NLAYERS: a layered (deep inverse Rosenblatt) transport towards the target of examples/devfun/pullback_tempered.hip,
    built over the ladder beta_j = 4^(j - NLAYERS), without a point leaving the device.  Layer 1 is the cross approximation of
    sqrt(pi^beta_1) on the physical grid (TTX_FUN_DEVICE, tempered_root); layer j + 1 is TTCross.pullback of sqrt(exp(beta_(j+1) logpi(x)
    - logq)) through the layers so far, on a reference grid of N nodes in [0, 1].  After each layer: the effective sample size of
    transport_sample at npts uniforms against the FINAL target, as a fraction of npts.  Prints a line per layer and one JSON line.  A
    worked example, not a test.  keep: the layers stay open and are returned with the result."""
    import json
    import torch
    torch.cuda.init()          # as run_tijk: torch's device first
    d, n, r, nl = (int(a) for a in argv[:4])
    mu, sigma, c, rho, lo, hi = 0.4, 0.8, 2.0, 0.1, -2.5, 3.5
    co = compile_device_fun(os.path.join(DEVFUN_DIR, "pullback_tempered.hip"))
    box, unit = lo + (hi - lo) * np.arange(n) / (n - 1.0), np.arange(n) / (n - 1.0)
    box[-1], unit[-1] = hi, 1.0
    kw = dict(accuracy=500 * EPS, pivoting=2, device=device)
    dev = torch.device("cuda", device)
    u = torch.from_numpy(np.random.default_rng(1).random((npts, d))).to(dev)

    def ess(layers):
        x, logq, _ = transport_sample(layers, u)
        z = (x - mu) / sigma
        logw = -0.5 * (z * z).sum(dim=1) - c * (x[:, 0] * x[:, 1] - rho) ** 2 - logq
        logw = logw[torch.isfinite(logw)]
        w = torch.exp(logw - logw.max())
        return float(w.sum() ** 2 / (w * w).sum() / npts)

    betas = [4.0 ** (j + 1 - nl) for j in range(nl)]
    first = TTCross([n] * d, TTX_FUN_DEVICE, [], r, **kw).set_integrand_device(co, "tempered_root", [betas[0], mu, sigma, c, rho, lo, hi]).run()
    layers, rows = [(first, [box] * d, gamma)], []
    rows.append(dict(layer=1, beta=betas[0], run_ms=first.seconds * 1e3, neval=first.neval, ranks_max=int(first.ranks().max()), ess=ess(layers)))
    print(f"layer 1 beta {betas[0]:.4f}: {rows[-1]['run_ms']:.2f} ms, neval {first.neval}, ESS/N {rows[-1]['ess']:.4f}", flush=True)
    for j in range(1, nl):
        tt = TTCross.pullback(layers, [unit] * d, (co, "pullback_tempered"), r, par=[betas[j], mu, sigma, c, rho], **kw).run()
        tt.run()                                        # the timed run: the first one carries the first-launch costs
        run_ms = tt.seconds * 1e3
        tt.set_profile(True)
        tt.run()
        last = tt.pullback_last()
        layers.append((tt, [unit] * d, gamma))
        rows.append(dict(layer=j + 1, beta=betas[j], run_ms=run_ms, neval=tt.neval, ranks_max=int(tt.ranks().max()), slot_ms=last["ms"], slot_launches=last["launches"],
                         slot_elements=last["elements"], slot_failed=last["failed"], slot_ms_per_launch=last["ms"] / max(last["launches"], 1), ess=ess(layers)))
        print(f"layer {j + 1} beta {betas[j]:.4f}: {run_ms:.2f} ms, neval {tt.neval}, slot kernels {last['ms']:.2f} ms in {last['launches']} launches "
              f"({last['elements']} elements, {last['failed']} failed), ESS/N {rows[-1]['ess']:.4f}", flush=True)
    res = dict(d=d, n=n, maxrank=r, layers=nl, npts=npts, gamma=gamma, rows=rows)
    print(json.dumps(res), flush=True)
    if keep:                                            # the caller goes on with the layers (and closes them)
        return dict(res, transport=layers, betas=betas, target=(mu, sigma, c, rho))
    for y, _, _ in reversed(layers):
        y.close()
    return res


def run_moments(argv, device=0, repeats=3, tt=None, nsample=100000):
    """moments WORKLOAD [NSEL] [MODE]: the trains of the tijk sub-command, taken as the square root of a density on equidistant nodes
    of [0, 1].  NSEL modes spread evenly over the train are selected (0 or absent: all).  One JSON line: the sq_moments call with the
    hat functions' moment matrices (the median call and the chains, band, carry and close parts from sq_moments_last, the carried
    steps and the flops per second of the carry part), the same call with TTX_SQM_BATCH = 1 (a launch per carried matrix), the host
    route (every core to the host, the time of numpy einsum chain steps on the widest core times the steps of the call: an estimate, the
    full route is not run), and the mean and covariance of density_moments against those of NSAMPLE points of sample_sq_real in
    standard errors."""
    import json
    import os
    import time
    import torch
    from .engine import mass_tridiag, moment_tridiag
    torch.cuda.init()          # a torch that brings its own HIP runtime must initialise its device before the engine's library does
    workload = argv[0]
    nsel = int(argv[1]) if len(argv) > 1 else 0
    mode = argv[2] if len(argv) > 2 else "auto"
    tt = tt or tijk_train(workload, device=device)
    d = tt.d
    nodes = [np.linspace(0.0, 1.0, int(nk)) for nk in tt._n]
    sel = list(range(d)) if nsel <= 0 or nsel >= d else sorted(set(int(round(v)) for v in np.linspace(0, d - 1, nsel)))
    md, mo = mass_tridiag(nodes)
    ad, ao, a2d, a2o = [None] * d, [None] * d, [None] * d, [None] * d
    for k in sel:
        ad[k], ao[k] = moment_tridiag(nodes[k], 1)
        a2d[k], a2o[k] = moment_tridiag(nodes[k], 2)

    def timed():
        tt.sq_moments(md, mo, ad, ao, a2d, a2o, mode=mode)                      # warm-up
        ms, lasts = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            res = tt.sq_moments(md, mo, ad, ao, a2d, a2o, mode=mode)
            ms.append((time.perf_counter() - t0) * 1e3)
            lasts.append(tt.sq_moments_last())
        med = {k: float(np.median([x[k] for x in lasts])) for k in ("ms_chains", "ms_band", "ms_carry", "ms_close")}
        return res, float(np.median(ms)), med, lasts[-1]

    res, ms_call, med, last = timed()
    r = tt.ranks().astype(np.int64)
    n = np.asarray(tt._n, dtype=np.int64)
    smax = max(sel)
    carry_flops = float(sum(2.0 * r[j] * n[j] * r[j + 1] * (r[j] + r[j + 1]) for k in sel if k < smax for j in range(k, smax)))
    line = dict(workload=workload, d=d, max_rank=int(r.max()), selected=len(sel), mode_asked=mode, mode=last["mode"], steps=last["steps"], flops=last["flops"],
                ms_call=ms_call, **med, carry_flops=carry_flops, carry_tflops=carry_flops / (med["ms_carry"] * 1e-3) / 1e12 if med["ms_carry"] > 0 else None, z_exp=res["z_exp"])
    old = os.environ.get("TTX_SQM_BATCH")
    os.environ["TTX_SQM_BATCH"] = "1"
    try:
        res1, ms1, med1, _ = timed()
    finally:
        if old is None:
            del os.environ["TTX_SQM_BATCH"]
        else:
            os.environ["TTX_SQM_BATCH"] = old
    line.update(ms_call_batch1=ms1, ms_carry_batch1=med1["ms_carry"], batch1_equal=bool(np.array_equal(res["c2"], res1["c2"]) and np.array_equal(res["m1"], res1["m1"])))
    t0 = time.perf_counter()
    cores = [tt.core(k + 1) for k in range(d)]
    ms_get = (time.perf_counter() - t0) * 1e3
    kw = int(np.argmax(r[:-1] * n * r[1:]))
    c, M = cores[kw], np.diag(md[kw]) + np.diag(mo[kw], 1) + np.diag(mo[kw], -1)
    P = np.ones((c.shape[0], c.shape[0]))
    t0 = time.perf_counter()
    for _ in range(3):
        np.einsum("ac,aib,ij,cjd->bd", P, c, M, c, optimize=True)
    ms_step = (time.perf_counter() - t0) * 1e3 / 3.0
    line.update(host_cores_get_ms=ms_get, host_step_ms_widest_core=ms_step, host_route_ms_estimated=ms_get + ms_step * (2 * d + last["steps"]))
    dm = tt.density_moments(nodes, select=sel, mode=mode)
    u = _seeded_uniforms(nsample, d, torch.device("cuda", device))
    x = tt.sample_sq_real(u, nodes, mode=mode, want=("x",))["x"].cpu().numpy()
    x = x[~np.isnan(x[:, 0])][:, sel]
    sm = x.mean(axis=0)
    y = x - sm
    sc = (y.T @ y) / x.shape[0]
    se_m = np.sqrt(np.maximum(np.diag(dm["cov"]), 0.0) / x.shape[0])
    se_c = np.sqrt(np.maximum(np.einsum("pk,pl->kl", y * y, y * y) / x.shape[0] - sc * sc, 0.0) / x.shape[0])
    with np.errstate(invalid="ignore", divide="ignore"):
        line.update(samples=int(x.shape[0]), alpha=dm["alpha"], logz=dm["logz"], mean_worst_se=float(np.nanmax(np.abs(sm - dm["mean"]) / se_m)),
                    cov_worst_se=float(np.nanmax(np.abs(sc - dm["cov"]) / se_c)), cov_finite=bool(np.isfinite(dm["cov"]).all()))
    print(json.dumps(line))
    return line


if __name__ == "__main__":
    if sys.argv[1] == "moments":
        run_moments(sys.argv[2:])
    elif sys.argv[1] == "dirt":
        run_dirt(sys.argv[2:])
    elif sys.argv[1] == "roundsum":
        run_roundsum(sys.argv[2:])
    elif sys.argv[1] == "tijk":
        run_tijk(sys.argv[2:])
    elif sys.argv[1] == "compose":
        run_compose(sys.argv[2:])
    elif sys.argv[1] == "sample":
        run_sample(sys.argv[2:])
    elif sys.argv[1] == "samplereal":
        run_samplereal(sys.argv[2:])
    elif sys.argv[1] == "samplesq":
        run_samplesq(sys.argv[2:])
    elif sys.argv[1] == "samplesqreal":
        run_samplesqreal(sys.argv[2:])
    elif sys.argv[1] == "rosenblatt":
        run_rosenblatt(sys.argv[2:])
    elif sys.argv[1] == "topk":
        run_topk(sys.argv[2:])
    elif sys.argv[1] == "contract":
        run_contract(sys.argv[2:])
    elif sys.argv[1] == "algebra":
        run_algebra(sys.argv[2:])
    elif sys.argv[1] == "modeapply":
        run_modeapply(sys.argv[2:])
    elif sys.argv[1] == "basis":
        run_basis(sys.argv[2:])
    elif sys.argv[1] == "basisgrad":
        run_basisgrad(sys.argv[2:])
    elif sys.argv[1] == "coregrad":
        run_coregrad(sys.argv[2:])
    elif sys.argv[1] == "fit":
        run_fit(sys.argv[2:])
    elif sys.argv[1] == "enrich":
        run_enrich(sys.argv[2:])
    elif sys.argv[1] == "mle":
        run_mle(sys.argv[2:])
    elif sys.argv[1] == "chf":
        run_chf(sys.argv[2:])
    elif sys.argv[1] == "pdf":
        run_pdf(sys.argv[2:])
    else:
        run_driver(sys.argv[1:])
