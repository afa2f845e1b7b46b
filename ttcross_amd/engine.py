"""ctypes binding of libttx.so (include/ttx.h) and a host-side mirror of the reference's dmrgg_lib API.

Reference interface mirrored (lib/dmrgg.f90:11-26):
    subroutine dtt_dmrgg(arg, fun, par, accuracy, maxrank, mybonds, pivoting, neval, quad, tru)
    double precision function dtt_quad(arg, quad, mybonds)
`fun` is replaced by the id of a built-in device integrand (TTX_FUN_*), everything else keeps its name,
meaning and error behaviour (the reference prints and stops; here TTXError carries the same message).
"""
import ctypes
import os
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_int32, c_int64, c_uint8, c_uint64, c_void_p

import numpy as np

TTX_FUN_ISING, TTX_FUN_STDNORM, TTX_FUN_MVN, TTX_FUN_HOST = 1, 2, 3, 4
TTX_FUN_COSCOEFF = 5       # calc_coefficient of test_crs_coscoeff.f90: aux = [mu, Sigma column-major, a, b], par unused
TTX_FUN_DEVICE = 6         # any user `fun` on the device: a code object written against include/ttx_device_fun.h (set_integrand_device)
TTX_FUN_TRAINS = 7         # fun(i) = g(x_1(i), .., x_m(i)) of resident trains (TTCross.of_trains, set_integrand_trains)
TTX_FUN_PULLBACK = 8       # fun(i) = h(x, logq, val) at the grid point of i pulled back through resident transports (TTCross.pullback)
TTX_PULLBACK_MAX = 8
TTX_TRAINS_MAX = 8
TTX_TOP_PRODUCT, TTX_TOP_RATIO, TTX_TOP_SQRTABS, TTX_TOP_DEVICE = 1, 2, 3, 4
TRAIN_OPS = {"product": TTX_TOP_PRODUCT, "ratio": TTX_TOP_RATIO, "sqrtabs": TTX_TOP_SQRTABS}
TTX_EVAL_EXACT, TTX_EVAL_MFMA, TTX_EVAL_AUTO = 0, 1, 2
EVAL_MODES = {"exact": TTX_EVAL_EXACT, "mfma": TTX_EVAL_MFMA, "auto": TTX_EVAL_AUTO}
TOPK_WHICH = {"abs": 0, "max": 1, "min": 2}
TTX_BASIS_COS, TTX_BASIS_LINEAR, TTX_BASIS_HALVE_FIRST = 1, 2, 1
BASIS_KINDS = {"cos": TTX_BASIS_COS, "linear": TTX_BASIS_LINEAR}
K_NAMES = ("lottery", "halfstep", "accept", "exchange", "quad", "other")

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path():
    """libttx.so of this tree; TTX_LIB names another build of the same sources (e.g. the -DTTX_STAMPS phase-timing build)."""
    return os.environ.get("TTX_LIB") or os.path.join(_HERE, "lib", "libttx.so")


class _Layer(ctypes.Structure):
    """ttx_layer of include/ttx.h: one layer of a pulled-back integrand"""
    _fields_ = [("x", c_void_p), ("nodes", POINTER(POINTER(c_double))), ("gamma", c_double)]


class TTXError(RuntimeError):
    pass


class _Config(ctypes.Structure):
    _fields_ = [("d", c_int32), ("n", POINTER(c_int32)), ("fun_id", c_int32), ("par", POINTER(c_double)),
                ("npar", c_int32), ("aux", POINTER(c_double)), ("naux", c_int32), ("quadw", POINTER(c_double)),
                ("accuracy", c_double), ("maxrank", c_int32), ("pivoting", c_int32), ("tru", c_double),
                ("has_tru", c_int32), ("nproc", c_int32), ("mybonds", POINTER(c_int32)), ("device", c_int32),
                ("world_rank", c_int32), ("world_size", c_int32), ("verbose", c_int32), ("arith", c_int32)]


_SENDRECV = ctypes.CFUNCTYPE(ctypes.c_int, c_void_p, ctypes.c_int, c_void_p, c_int64, ctypes.c_int, c_void_p, c_int64)
_ALLREDUCE = ctypes.CFUNCTYPE(ctypes.c_int, c_void_p, POINTER(c_double), c_int64, ctypes.c_int)


class _Transport(ctypes.Structure):
    _fields_ = [("ctx", c_void_p), ("sendrecv", _SENDRECV), ("allreduce", _ALLREDUCE)]


class _Basis(ctypes.Structure):      # ttx_basis
    _fields_ = [("kind", c_int32), ("flags", c_int32), ("a", c_double), ("b", c_double), ("nodes", POINTER(c_double))]


class _FitOpts(ctypes.Structure):    # ttx_fit_opts
    _fields_ = [("max_iter", c_int32), ("cg_max", c_int32), ("max_reject", c_int32), ("mode", c_int32), ("lambda0", c_double),
                ("lambda_down", c_double), ("lambda_up", c_double), ("cg_tol", c_double), ("loss_tol", c_double)]


class _FitResult(ctypes.Structure):  # ttx_fit_result
    _fields_ = [("iters", c_int32), ("stop", c_int32)]


FIT_STOPS = {1: "max_iter", 2: "loss_tol", 3: "zero_gradient", 4: "max_reject", 5: "non_finite"}
FIT_DEFAULTS = dict(max_iter=20, cg_max=40, max_reject=8, mode="auto", lambda0=1.0, lambda_down=0.3, lambda_up=4.0, cg_tol=1e-2, loss_tol=0.0)


class SweepRec(ctypes.Structure):
    _fields_ = [("it", c_int32), ("dir", c_int32), ("erank", c_double), ("neval", c_int64), ("val", c_double),
                ("amax", c_double), ("pivotmax", c_double), ("pivotmin", c_double), ("seconds", c_double)]


_lib = None


def load_library():
    """Load libttx.so; fails loudly if the HIP extension has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise TTXError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(the engine has no CPU path)")
    L = ctypes.CDLL(p)
    L.ttx_last_error.restype = c_char_p
    L.ttx_version.restype = ctypes.c_int
    L.ttx_create.argtypes = [POINTER(c_void_p), POINTER(_Config)]
    L.ttx_destroy.argtypes = [c_void_p]
    L.ttx_destroy.restype = None
    L.ttx_comm_unique_id.argtypes = [POINTER(c_uint8)]
    L.ttx_comm_init.argtypes = [c_void_p, POINTER(c_uint8)]
    L.ttx_set_transport.argtypes = [c_void_p, POINTER(_Transport)]
    L.ttx_run.argtypes = [c_void_p]
    L.ttx_num_sweeps.argtypes = [c_void_p]
    L.ttx_get_sweeps.argtypes = [c_void_p, POINTER(SweepRec), ctypes.c_int]
    L.ttx_get_tapes.argtypes = [c_void_p, POINTER(c_int32), c_int64]
    L.ttx_neval.argtypes = [c_void_p]
    L.ttx_neval.restype = c_int64
    L.ttx_seconds.argtypes = [c_void_p]
    L.ttx_seconds.restype = c_double
    L.ttx_get_ranks.argtypes = [c_void_p, POINTER(c_int32)]
    L.ttx_core_size.argtypes = [c_void_p, ctypes.c_int]
    L.ttx_core_size.restype = c_int64
    L.ttx_get_core.argtypes = [c_void_p, ctypes.c_int, POINTER(c_double)]
    L.ttx_quad.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double)]
    L.ttx_set_profile.argtypes = [c_void_p, ctypes.c_int]
    L.ttx_ort.argtypes = [c_void_p]
    L.ttx_svd.argtypes = [c_void_p, c_double, c_int32]
    L.ttx_norm.argtypes = [c_void_p, c_double, POINTER(c_double)]
    L.ttx_lognrm.argtypes = [c_void_p, c_double, POINTER(c_double)]
    L.ttx_dot.argtypes = [c_void_p, c_void_p, POINTER(c_double)]
    L.ttx_ijk.argtypes = [c_void_p, POINTER(c_int32), POINTER(c_double)]
    L.ttx_ijk_batch.argtypes = [c_void_p, c_int64, POINTER(c_int32), POINTER(c_double), c_int32]
    L.ttx_ijk_batch_dev.argtypes = [c_void_p, c_int64, c_void_p, c_void_p, c_int32]
    L.ttx_value_batch.argtypes = [c_void_p, c_int64, c_int32, POINTER(c_double), POINTER(c_double), c_int32]
    L.ttx_eval_last_mode.argtypes = [c_void_p]
    L.ttx_contract.argtypes = [c_void_p, POINTER(c_int32), POINTER(c_double), POINTER(c_void_p)]
    L.ttx_marginals.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double)]
    L.ttx_contract_modesum.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double)]
    L.ttx_lincomb.argtypes = [c_int32, POINTER(c_double), POINTER(c_void_p), POINTER(c_void_p)]
    L.ttx_hadamard.argtypes = [c_void_p, c_void_p, POINTER(c_void_p)]
    L.ttx_algebra_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double)]
    L.ttx_lincomb_round.argtypes = [c_int32, POINTER(c_double), POINTER(c_void_p), c_int32, c_double, c_int32, ctypes.c_uint64, c_int32, POINTER(c_void_p)]
    L.ttx_roundsum_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_int32), POINTER(c_int32)]
    L.ttx_mode_apply.argtypes = [c_void_p, POINTER(c_int32), POINTER(c_double), c_int32, POINTER(c_void_p)]
    L.ttx_mode_apply_dev.argtypes = [c_void_p, POINTER(c_int32), c_void_p, c_int32, POINTER(c_void_p)]
    L.ttx_mode_apply_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int32)]
    L.ttx_basis_batch.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(_Basis), POINTER(c_double), c_int32]
    L.ttx_basis_batch_dev.argtypes = [c_void_p, c_int64, c_void_p, POINTER(_Basis), c_void_p, c_int32]
    L.ttx_basis_tab.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(c_double), c_int32]
    L.ttx_basis_tab_dev.argtypes = [c_void_p, c_int64, c_void_p, c_void_p, c_int32]
    L.ttx_basis_host.argtypes = [POINTER(_Basis), c_int32, c_int64, POINTER(c_double), c_int64, POINTER(c_double)]
    L.ttx_basis_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int32)]
    L.ttx_basis_grad_batch.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(_Basis), POINTER(c_double), POINTER(c_double), c_int32]
    L.ttx_basis_grad_batch_dev.argtypes = [c_void_p, c_int64, c_void_p, POINTER(_Basis), c_void_p, c_void_p, c_int32]
    L.ttx_basis_grad_tab.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), c_int32]
    L.ttx_basis_grad_tab_dev.argtypes = [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32]
    L.ttx_basis_host_d.argtypes = [POINTER(_Basis), c_int32, c_int64, POINTER(c_double), c_int64, POINTER(c_double)]
    L.ttx_basis_grad_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int32), POINTER(c_int64)]
    L.ttx_basis_core_grad_batch.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(_Basis), POINTER(c_double), POINTER(c_double), POINTER(c_double), c_int32, c_int32]
    L.ttx_basis_core_grad_batch_dev.argtypes = [c_void_p, c_int64, c_void_p, POINTER(_Basis), c_void_p, c_void_p, c_void_p, c_int32, c_int32]
    L.ttx_basis_core_grad_tab.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), c_int32, c_int32]
    L.ttx_basis_core_grad_tab_dev.argtypes = [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32]
    L.ttx_basis_core_grad_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int32),
                                           POINTER(c_int64)]
    L.ttx_cores_axpy.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double)]
    L.ttx_cores_axpy_dev.argtypes = [c_void_p, POINTER(c_double), c_void_p]
    _en_host = [POINTER(c_int32), ctypes.c_uint64, c_int32, POINTER(c_void_p), POINTER(c_int32), POINTER(c_double), POINTER(c_double), POINTER(c_double)]
    _en_dev = _en_host[:-1] + [c_void_p]
    L.ttx_basis_enrich_batch.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(_Basis), POINTER(c_double)] + _en_host
    L.ttx_basis_enrich_batch_dev.argtypes = [c_void_p, c_int64, c_void_p, POINTER(_Basis), c_void_p] + _en_dev
    L.ttx_basis_enrich_tab.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(c_double)] + _en_host
    L.ttx_basis_enrich_tab_dev.argtypes = [c_void_p, c_int64, c_void_p, c_void_p] + _en_dev
    L.ttx_basis_enrich_last.argtypes = [c_void_p] + [POINTER(c_double)] * 6 + [POINTER(c_int32), POINTER(c_int64)]
    L.ttx_basis_jvp_batch.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(_Basis), POINTER(c_double), POINTER(c_double), POINTER(c_double), c_int32]
    L.ttx_basis_jvp_batch_dev.argtypes = [c_void_p, c_int64, c_void_p, POINTER(_Basis), c_void_p, c_void_p, c_void_p, c_int32]
    L.ttx_basis_jvp_tab.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), c_int32]
    L.ttx_basis_jvp_tab_dev.argtypes = [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int32]
    L.ttx_basis_jvp_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int32)]
    L.ttx_cores_dot.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double)]
    L.ttx_cores_dot_dev.argtypes = [c_void_p, c_void_p, c_void_p, POINTER(c_double)]
    L.ttx_cores_axpby_dev.argtypes = [c_void_p, c_double, c_void_p, c_double, c_void_p]
    L.ttx_cores_get_dev.argtypes = [c_void_p, c_void_p]
    L.ttx_cores_get.argtypes = [c_void_p, POINTER(c_double)]
    L.ttx_cores_set.argtypes = [c_void_p, POINTER(c_double)]
    L.ttx_cores_set_dev.argtypes = [c_void_p, c_void_p]
    _hist = [POINTER(_FitOpts), POINTER(c_double), POINTER(c_double), POINTER(c_int32), POINTER(c_int32), POINTER(_FitResult)]
    L.ttx_basis_fit_batch.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(_Basis), POINTER(c_double), POINTER(c_double)] + _hist
    L.ttx_basis_fit_batch_dev.argtypes = [c_void_p, c_int64, c_void_p, POINTER(_Basis), c_void_p, c_void_p] + _hist
    L.ttx_basis_fit_tab.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(c_double), POINTER(c_double)] + _hist
    L.ttx_basis_fit_tab_dev.argtypes = [c_void_p, c_int64, c_void_p, c_void_p, c_void_p] + _hist
    L.ttx_basis_fit_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int64), POINTER(c_int64), POINTER(c_int32)]
    _rows = POINTER(POINTER(c_double))
    _zout = [POINTER(c_double), POINTER(c_int64), POINTER(c_double)]
    L.ttx_sq_lognorm_grad.argtypes = [c_void_p, _rows, _rows, c_double, c_double, POINTER(c_double), c_int32, c_int32] + _zout
    L.ttx_sq_lognorm_grad_dev.argtypes = [c_void_p, _rows, _rows, c_double, c_double, c_void_p, c_int32, c_int32] + _zout
    L.ttx_sq_lognorm_grad_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int32)]
    L.ttx_sq_nll_batch.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(_Basis), POINTER(c_double), c_double, _rows, _rows, c_double, c_int32,
                                   POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double)]
    L.ttx_sq_nll_batch_dev.argtypes = [c_void_p, c_int64, c_void_p, POINTER(_Basis), c_void_p, c_double, _rows, _rows, c_double, c_int32,
                                       POINTER(c_double), POINTER(c_double), c_void_p, c_void_p]
    L.ttx_sq_moments.argtypes = [c_void_p] + [_rows] * 6 + [c_int32, POINTER(c_double), POINTER(c_int64)] + [POINTER(c_double)] * 4
    L.ttx_sq_moments_last.argtypes = [c_void_p] + [POINTER(c_double)] * 5 + [POINTER(c_int64), POINTER(c_int32)]
    L.ttx_sample.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(c_double), POINTER(c_int32), POINTER(c_int32), POINTER(c_double), POINTER(c_double)]
    L.ttx_sample_dev.argtypes = [c_void_p, c_int64, c_void_p, POINTER(c_double), POINTER(c_int32), c_void_p, c_void_p, c_void_p]
    L.ttx_sample_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int64)]
    L.ttx_sample_real.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(POINTER(c_double)), POINTER(c_double), POINTER(c_double), POINTER(c_int32), POINTER(c_double),
                                  POINTER(c_double)]
    L.ttx_sample_real_dev.argtypes = [c_void_p, c_int64, c_void_p, POINTER(POINTER(c_double)), POINTER(c_double), c_void_p, c_void_p, c_void_p, c_void_p]
    L.ttx_sample_real_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int64)]
    L.ttx_sample_sq.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(c_double), POINTER(c_int32), c_double, c_int32, POINTER(c_int32), POINTER(c_double),
                                POINTER(c_double)]
    L.ttx_sample_sq_dev.argtypes = [c_void_p, c_int64, c_void_p, POINTER(c_double), POINTER(c_int32), c_double, c_int32, c_void_p, c_void_p, c_void_p]
    L.ttx_sample_sq_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int64), POINTER(c_int32)]
    L.ttx_sample_sq_real.argtypes = [c_void_p, c_int64, POINTER(c_double), POINTER(POINTER(c_double)), POINTER(c_double), c_double, c_int32, POINTER(c_double),
                                     POINTER(c_int32), POINTER(c_double), POINTER(c_double)]
    L.ttx_sample_sq_real_dev.argtypes = [c_void_p, c_int64, c_void_p, POINTER(POINTER(c_double)), POINTER(c_double), c_double, c_int32, c_void_p, c_void_p, c_void_p, c_void_p]
    L.ttx_sample_sq_real_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int64), POINTER(c_int32)]
    L.ttx_rosenblatt_sq_real.argtypes = L.ttx_sample_sq_real.argtypes
    L.ttx_rosenblatt_sq_real_dev.argtypes = L.ttx_sample_sq_real_dev.argtypes
    L.ttx_rosenblatt_sq_real_last.argtypes = L.ttx_sample_sq_real_last.argtypes
    L.ttx_topk.argtypes = [c_void_p, c_int32, c_int32, POINTER(c_int32), c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_double), POINTER(c_double)]
    L.ttx_topk_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int32)]
    L.ttx_zquad.argtypes = [c_void_p, c_int32, POINTER(c_double), POINTER(c_double)]
    L.ttx_accchk.argtypes = [c_void_p, c_int32, POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_double), POINTER(c_int32)]
    L.ttx_from_tt.argtypes = [POINTER(c_void_p), c_int32, POINTER(c_int32), POINTER(c_int32), POINTER(c_double), c_int32]
    L.ttx_write.argtypes = [c_void_p, ctypes.c_char_p]
    L.ttx_read.argtypes = [POINTER(c_void_p), ctypes.c_char_p, c_int32]
    L.ttx_get_modes.argtypes = [c_void_p, POINTER(c_int32), POINTER(c_int32)]
    L.ttx_kernel_stats.argtypes = [c_void_p, POINTER(c_int64), POINTER(c_double), POINTER(c_double)]
    L.ttx_k_residual_argmax.argtypes = [c_int32, c_int32, c_int32, POINTER(c_double), POINTER(c_double),
                                        POINTER(c_double), POINTER(c_double), POINTER(c_int32), POINTER(c_double)]
    L.ttx_k_residual_bench.argtypes = [c_int32, c_int64, c_int32, c_int32, POINTER(c_double), POINTER(c_double)]
    L.ttx_k_eval.argtypes = [c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_double), c_int32,
                             POINTER(c_double), c_int32, c_int64, POINTER(c_int32), POINTER(c_double)]
    L.ttx_k_lottery.argtypes = [c_int32, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32),
                                c_uint64, POINTER(c_int32)]
    L.ttx_set_integrand_host.argtypes = [c_void_p, c_void_p, POINTER(c_double)]
    L.ttx_host_calls.argtypes = [c_void_p]
    L.ttx_host_calls.restype = c_int64
    L.ttx_set_integrand_device.argtypes = [c_void_p, c_char_p, c_int64, c_char_p, POINTER(c_double), c_int32]
    L.ttx_set_integrand_device_file.argtypes = [c_void_p, c_char_p, c_char_p, POINTER(c_double), c_int32]
    L.ttx_eval_device.argtypes = [c_void_p, c_int64, POINTER(c_int32), POINTER(c_double)]
    L.ttx_set_integrand_trains.argtypes = [c_void_p, c_int32, POINTER(c_void_p), c_int32]
    L.ttx_set_integrand_trains_device.argtypes = [c_void_p, c_int32, POINTER(c_void_p), c_char_p, c_int64, c_char_p, POINTER(c_double), c_int32]
    L.ttx_set_integrand_trains_device_file.argtypes = [c_void_p, c_int32, POINTER(c_void_p), c_char_p, c_char_p, POINTER(c_double), c_int32]
    L.ttx_trainfun_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int64), POINTER(c_int64)]
    L.ttx_set_integrand_pullback.argtypes = [c_void_p, c_int32, POINTER(_Layer), POINTER(POINTER(c_double)), c_char_p, c_int64, c_char_p, POINTER(c_double), c_int32]
    L.ttx_set_integrand_pullback_file.argtypes = [c_void_p, c_int32, POINTER(_Layer), POINTER(POINTER(c_double)), c_char_p, c_char_p, POINTER(c_double), c_int32]
    L.ttx_pullback_points.argtypes = [c_void_p, c_int64, POINTER(c_int32), POINTER(c_double), POINTER(c_double), POINTER(c_double)]
    L.ttx_pullback_last.argtypes = [c_void_p, POINTER(c_double), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]
    L.ttx_k_exp.argtypes = [c_int32, c_int64, POINTER(c_double), POINTER(c_double)]
    L.ttx_exp_host.argtypes = [c_int64, POINTER(c_double), POINTER(c_double)]
    _lib = L
    return L


INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")      # ttx.h, ttx_device_fun.h
DEVFUN_DIR = os.path.join(os.path.dirname(_HERE), "examples", "devfun")    # example device integrands (source)


def compile_device_fun(source_path, out_path=None, extra_flags=()):
    """Compile a device integrand (a .hip file written against include/ttx_device_fun.h) to a gfx950 code object with
    `hipcc --genco --offload-arch=gfx950 -O3 -ffp-contract=off -I <repo>/include`; returns the path of the code object
    (default: the source path with the suffix .hsaco).  Rebuilds only when the code object is older than the source or
    the header; when no hipcc is found an existing code object is used as it is.  Raises TTXError with the compiler's
    stderr on failure."""
    source_path = os.fspath(source_path)
    out_path = os.fspath(out_path) if out_path else os.path.splitext(source_path)[0] + ".hsaco"
    deps = [source_path, os.path.join(INCLUDE_DIR, "ttx_device_fun.h")]
    if not os.path.exists(source_path):
        raise TTXError(f"compile_device_fun: {source_path} not found")
    fresh = os.path.exists(out_path) and all(os.path.getmtime(out_path) >= os.path.getmtime(f) for f in deps)
    if fresh:
        return out_path
    hipcc = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
    if hipcc is None:
        if os.path.exists(out_path):
            return out_path
        raise TTXError(f"compile_device_fun: no hipcc on this machine and no code object {out_path}")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    cmd = [hipcc, "--genco", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-I", INCLUDE_DIR, *extra_flags, source_path, "-o", out_path]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0 or not os.path.exists(out_path):
        raise TTXError("compile_device_fun: " + " ".join(cmd) + " failed:\n" + p.stderr[-4000:])
    return out_path


def _check(rc):
    if rc != 0:
        raise TTXError(load_library().ttx_last_error().decode())


def _dp(a):
    return a.ctypes.data_as(POINTER(c_double)) if a is not None else None


def _ip(a):
    return a.ctypes.data_as(POINTER(c_int32)) if a is not None else None


def _eval_mode(mode):
    if mode in EVAL_MODES:
        return EVAL_MODES[mode]
    if mode in EVAL_MODES.values():
        return int(mode)
    raise ValueError(f"mode must be one of {sorted(EVAL_MODES)} (got {mode!r})")


def _basis_struct(entry, n):
    """one basis entry, ("cos", a, b[, halve_first]) or ("linear", nodes) for a mode of n indices -> (ttx_basis, what it points to)"""
    if not isinstance(entry, (tuple, list)) or not entry or entry[0] not in BASIS_KINDS:
        raise ValueError(f'basis: ("cos", a, b[, halve_first]) or ("linear", nodes) expected (got {entry!r})')
    if entry[0] == "cos":
        if len(entry) not in (3, 4):
            raise ValueError(f'basis: ("cos", a, b[, halve_first]) expected (got {entry!r})')
        flags = TTX_BASIS_HALVE_FIRST if len(entry) == 4 and entry[3] else 0
        return _Basis(TTX_BASIS_COS, flags, float(entry[1]), float(entry[2]), None), None
    if len(entry) != 2:
        raise ValueError(f'basis: ("linear", nodes) expected (got {entry!r})')
    nodes = np.ascontiguousarray(entry[1], dtype=np.float64)
    if nodes.ndim != 1 or nodes.size != int(n):
        raise ValueError(f"basis: {int(n)} nodes expected for a mode of {int(n)} indices (got shape {nodes.shape})")
    return _Basis(TTX_BASIS_LINEAR, 0, 0.0, 0.0, _dp(nodes)), nodes


def basis_table(entry, n, x):
    """The table of one mode on the host (include/ttx.h: ttx_basis_host): phi[p, j] = phi_j(x[p]), j = 0..n-1, for a basis entry
    ("cos", a, b[, halve_first]) or ("linear", nodes).  The device forms the same numbers bit for bit.  No engine, no GPU."""
    b, _keep = _basis_struct(entry, n)
    xa = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    phi = np.zeros((xa.size, int(n)))
    _check(load_library().ttx_basis_host(ctypes.byref(b), int(n), xa.size, _dp(xa), 1, _dp(phi)))
    return phi


def basis_dtable(entry, n, x):
    """The derivative table of one mode on the host (include/ttx.h: ttx_basis_host_d): dphi[p, j] = dphi_j/dx (x[p]) for a basis
    entry as basis_table takes it; for "linear" the right-hand derivative at an interior node, 0 on and outside the end nodes.
    The device forms the same numbers bit for bit.  No engine, no GPU."""
    b, _keep = _basis_struct(entry, n)
    xa = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    dphi = np.zeros((xa.size, int(n)))
    _check(load_library().ttx_basis_host_d(ctypes.byref(b), int(n), xa.size, _dp(xa), 1, _dp(dphi)))
    return dphi


def trapezoid_weights(nodes):
    """The trapezoid weights of strictly ascending nodes, the weights sample_real gives a drawn mode (include/ttx.h:
    ttx_sample_real): om[0] = 0.5 (t[1] - t[0]), om[i] = 0.5 (t[i+1] - t[i-1]), om[n-1] = 0.5 (t[n-1] - t[n-2]); a single node carries
    1.0.  One array of nodes gives one array, a list of arrays a list: quad(trapezoid_weights(nodes)) is the Z of sample_real."""
    if isinstance(nodes, (list, tuple)) and len(nodes) and np.ndim(nodes[0]) == 1:
        return [trapezoid_weights(t) for t in nodes]
    t = np.ascontiguousarray(nodes, dtype=np.float64)
    if t.ndim != 1 or t.size < 1:
        raise ValueError("trapezoid_weights: a one-dimensional array of nodes expected")
    if t.size == 1:
        return np.ones(1)
    om = np.empty(t.size)
    om[0], om[-1] = 0.5 * (t[1] - t[0]), 0.5 * (t[-1] - t[-2])
    om[1:-1] = 0.5 * (t[2:] - t[:-2])
    return om


def mass_cholesky(nodes):
    """The upper bidiagonal Cholesky factor (dg, sp) of the hat functions' mass matrix on strictly ascending nodes, the factor
    sample_sq_real gives a drawn mode (include/ttx.h: ttx_sample_sq_real): M = U^T U with U[i, i] = dg[i], U[i, i+1] = sp[i],
    M[i, i] = (h[i-1] + h[i]) / 3 with one term at each end, M[i, i+1] = h[i] / 6.  Plain float64, one operation at a time: the
    engine's host code forms the same bits.  A single node gives ([1.], [0.]).  One array of nodes gives one pair, a list of arrays
    a list of pairs."""
    if isinstance(nodes, (list, tuple)) and len(nodes) and np.ndim(nodes[0]) == 1:
        return [mass_cholesky(t) for t in nodes]
    t = np.ascontiguousarray(nodes, dtype=np.float64)
    if t.ndim != 1 or t.size < 1:
        raise ValueError("mass_cholesky: a one-dimensional array of nodes expected")
    n = t.size
    if n == 1:
        return np.ones(1), np.zeros(1)
    h = t[1:] - t[:-1]
    diag = np.empty(n)
    diag[0], diag[-1] = h[0] / 3.0, h[-1] / 3.0
    diag[1:-1] = (h[:-1] + h[1:]) / 3.0
    off = h / 6.0
    dg, sp = np.zeros(n), np.zeros(n)
    dg[0] = np.sqrt(diag[0])
    for i in range(n - 1):
        sp[i] = off[i] / dg[i]
        dg[i + 1] = np.sqrt(diag[i + 1] - sp[i] * sp[i])
    return dg, sp


def mass_tridiag(nodes, cond=None):
    """(md, mo) of the symmetric tridiagonal matrices sq_lognorm_grad and sq_nll take (include/ttx.h: ttx_sq_lognorm_grad) for the
    hat functions on strictly ascending nodes: the mass matrix M[i, i] = (h[i-1] + h[i]) / 3 with one term at each end,
    M[i, i+1] = h[i] / 6 -- U^T U of mass_cholesky(nodes) to rounding.  A single node gives ([1.], []).  One array of nodes gives
    one pair; a list of arrays gives (list of md, list of mo).  cond (with a list): per mode None or NaN for a drawn mode, else the
    coordinate the mode is held at, whose matrix is phi phi^T of its two adjacent hat values (zero elsewhere)."""
    if isinstance(nodes, (list, tuple)) and len(nodes) and np.ndim(nodes[0]) == 1:
        cond = [None] * len(nodes) if cond is None else list(cond)
        if len(cond) != len(nodes):
            raise ValueError("mass_tridiag: one cond entry per mode expected")
        pairs = [mass_tridiag(t, c) for t, c in zip(nodes, cond)]
        return [p[0] for p in pairs], [p[1] for p in pairs]
    t = np.ascontiguousarray(nodes, dtype=np.float64)
    if t.ndim != 1 or t.size < 1:
        raise ValueError("mass_tridiag: a one-dimensional array of nodes expected")
    n = t.size
    if cond is not None and not np.isnan(cond):
        x = float(cond)
        md, mo = np.zeros(n), np.zeros(max(n - 1, 0))
        if n == 1:
            md[0] = 1.0
            return md, mo
        if not t[0] <= x <= t[-1]:
            raise ValueError("mass_tridiag: a held coordinate lies outside the nodes")
        c = min(max(int(np.searchsorted(t, x, side="right")) - 1, 0), n - 2)
        p1 = (x - t[c]) / (t[c + 1] - t[c])
        p0 = 1.0 - p1
        md[c], md[c + 1], mo[c] = p0 * p0, p1 * p1, p0 * p1
        return md, mo
    if n == 1:
        return np.ones(1), np.zeros(0)
    h = t[1:] - t[:-1]
    md = np.empty(n)
    md[0], md[-1] = h[0] / 3.0, h[-1] / 3.0
    md[1:-1] = (h[:-1] + h[1:]) / 3.0
    return md, h / 6.0


def moment_tridiag(nodes, power, cond=None):
    """(d, o) of the symmetric tridiagonal matrix of int x^power phi_i(x) phi_j(x) dx for the hat functions on strictly ascending
    nodes, power 0, 1 or 2: the observables sq_moments takes for the mean (power 1) and the second moments (power 2).  Power 0 is
    mass_tridiag(nodes, cond), bit for bit.  Closed forms, one operation at a time; on the cell [a, b] of width h:
        power 1:  int x phi_a^2 = h (3 a + b) / 12,          int x phi_b^2 = h (a + 3 b) / 12,          int x phi_a phi_b = h (a + b) / 12
        power 2:  int x^2 phi_a^2 = h (6 a^2 + 3 a b + b^2) / 30,  int x^2 phi_b^2 = h (a^2 + 3 a b + 6 b^2) / 30,  int x^2 phi_a phi_b = h (3 a^2 + 4 a b + 3 b^2) / 60
    and a diagonal entry is the left cell's term plus the right cell's.  A single node t gives ([t^power], []).  Lists and cond as
    for mass_tridiag; a mode held at x0 gives x0^power times its mass_tridiag matrix."""
    if power not in (0, 1, 2):
        raise ValueError("moment_tridiag: power is 0, 1 or 2")
    if isinstance(nodes, (list, tuple)) and len(nodes) and np.ndim(nodes[0]) == 1:
        cond = [None] * len(nodes) if cond is None else list(cond)
        if len(cond) != len(nodes):
            raise ValueError("moment_tridiag: one cond entry per mode expected")
        pairs = [moment_tridiag(t, power, c) for t, c in zip(nodes, cond)]
        return [p[0] for p in pairs], [p[1] for p in pairs]
    if power == 0:
        return mass_tridiag(nodes, cond)
    t = np.ascontiguousarray(nodes, dtype=np.float64)
    if t.ndim != 1 or t.size < 1:
        raise ValueError("moment_tridiag: a one-dimensional array of nodes expected")
    held = cond is not None and not np.isnan(cond)
    if held or t.size == 1:
        md, mo = mass_tridiag(t, cond)
        x0 = float(cond) if held else float(t[0])
        f = x0 if power == 1 else x0 * x0
        return f * md, f * mo
    a, b = t[:-1], t[1:]
    h = b - a
    if power == 1:
        lo, hi, of = h * (3.0 * a + b) / 12.0, h * (a + 3.0 * b) / 12.0, h * (a + b) / 12.0
    else:
        aa, ab, bb = a * a, a * b, b * b
        lo, hi, of = h * (6.0 * aa + 3.0 * ab + bb) / 30.0, h * (aa + 3.0 * ab + 6.0 * bb) / 30.0, h * (3.0 * aa + 4.0 * ab + 3.0 * bb) / 60.0
    dg = np.empty(t.size)
    dg[0], dg[-1] = lo[0], hi[-1]
    dg[1:-1] = hi[:-1] + lo[1:]
    return dg, of


def roundsum_omega(seed, k, shape):
    """Core k (1-based) of the sketch train of lincomb_round, shape (l(k-1), n_k, l(k)), restated in numpy uint64 arithmetic
    (include/ttx.h: ttx_lincomb_round, step 2): bit for bit what the device generates.  Entry x = a + l(k-1) (i + n_k b):
    z = seed + 0x9E3779B97F4A7C15 ((k << 40) + x + 1), the splitmix64 finaliser, then sign = bit 63, magnitude = the next 52 bits
    times 2^-52: uniform on (-1, 1), every step exact."""
    shape = tuple(int(s) for s in shape)
    cnt = int(np.prod(shape))
    with np.errstate(over="ignore"):
        x = np.arange(cnt, dtype=np.uint64)
        z = np.uint64(int(seed) & (2 ** 64 - 1)) + np.uint64(0x9E3779B97F4A7C15) * (np.uint64(int(k) << 40) + x + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    mag = ((z >> np.uint64(11)) & np.uint64(2 ** 52 - 1)).astype(np.float64) * 2.0 ** -52
    v = np.where((z >> np.uint64(63)) != 0, -mag, mag)
    return v.reshape(shape, order="F")


def value_indices(n, x):
    """The index digits dtt_value (lib/tt.f90:702-728) forms for coordinate vectors x (npts, dd) of a train with mode sizes
    n(1:d), restated on the host in plain float64: mm = d // dd digits per coordinate, written from the LAST mode of the
    coordinate's group backwards; i = int(n xx), i = n clamped to n - 1, xx = xx n - i; xx > 1 is first reduced by
    xx - int(xx).  Returns (ind, neg): ind (npts, d) int32, 1-based, 0 where a mode got no digit (d not divisible by dd;
    dtt_ijk answers -3.0 there); neg (npts,) bool, true where a coordinate is negative (dtt_value answers 0.0)."""
    n = np.asarray(n, dtype=np.int64).ravel()
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    if not np.all(x < 2147483648.0):
        raise ValueError("value_indices: coordinates must be below 2^31")
    d, (npts, dd) = n.size, x.shape
    mm = d // dd
    ind = np.zeros((npts, d), dtype=np.int32)
    neg = np.zeros(npts, dtype=bool)
    for c in range(dd):
        xx = x[:, c].copy()
        neg |= xx < 0.0              # dtt_value returns at the first negative coordinate: the digits no longer matter
        big = xx > 1.0
        xx[big] = xx[big] - np.trunc(xx[big])
        for j in range(1, mm + 1):
            pos = c * mm + mm - j
            nn = float(n[pos])
            with np.errstate(invalid="ignore"):
                i = np.trunc(nn * xx)
            i[i == nn] = nn - 1.0
            ind[:, pos] = np.where(neg, 0, i).astype(np.int32) + 1
            xx = xx * nn - i
    ind[neg] = 0
    return ind, neg


def split_groups(nproc, world_rank, world_size):
    """Bond groups [g0, g0+G) held by one process: contiguous deal, as ttx_create does (include/ttx.h, nproc/world_size)."""
    g0 = nproc * world_rank // world_size
    return g0, nproc * (world_rank + 1) // world_size - g0


def neighbour_ranks(nproc, world_rank, world_size):
    """(left, right) process ranks the boundary groups exchange with; -1 where the chain ends."""
    g0, G = split_groups(nproc, world_rank, world_size)
    return (world_rank - 1 if g0 > 0 else -1), (world_rank + 1 if g0 + G < nproc else -1)


def transport_sample(layers, u, mode="exact"):
    """The composed inverse Rosenblatt map of a layered transport: layers = [(train, nodes, gamma), ..], layer 1 first; u (npts, d) in
    [0, 1], a host array or a float64 torch tensor on the layers' device, which then never leaves it (sample_sq_real's _dev entry).
    The layers are applied in the order m .. 1.  Returns x, logq (lq_m, then + lq_t for t = m-1 .. 1) and val of layer 1."""
    logq = val = None
    for x, nodes, gamma in reversed(list(layers)):
        o = x.sample_sq_real(u, nodes, gamma=gamma, mode=mode, want=("x", "logq", "val"))
        u, val = o["x"], o["val"]
        logq = o["logq"] if logq is None else logq + o["logq"]
    return u, logq, val


def transport_rosenblatt(layers, x, mode="exact"):
    """The way back of transport_sample: the layers' forward Rosenblatt maps in the order 1 .. m (rosenblatt_sq_real, its _dev entry
    for a tensor on the device).  Returns u, the summed logq and val of layer 1 at x."""
    logq = val = None
    for y, nodes, gamma in layers:
        o = y.rosenblatt_sq_real(x, nodes, gamma=gamma, mode=mode, want=("u", "logq", "val"))
        x = o["u"]
        val = o["val"] if val is None else val
        logq = o["logq"] if logq is None else logq + o["logq"]
    return x, logq, val


def make_dist_transport(dist, group=None):
    """ctypes thunks (sendrecv, allreduce) of include/ttx.h's ttx_transport over torch.distributed CPU tensors."""
    import torch

    def _t(ptr, nbytes):
        return torch.frombuffer((ctypes.c_char * nbytes).from_address(ptr), dtype=torch.uint8)

    def sendrecv(ctx, to, sbuf, ns, frm, rbuf, nr):
        try:
            ops = []
            if to >= 0:
                ops.append(dist.P2POp(dist.isend, _t(sbuf, ns), to, group))
            if frm >= 0:
                ops.append(dist.P2POp(dist.irecv, _t(rbuf, nr), frm, group))
            if ops:
                for w in dist.batch_isend_irecv(ops):
                    w.wait()
            return 0
        except Exception as e:  # noqa: BLE001
            print("transport sendrecv failed:", e, flush=True)
            return 1

    def allreduce(ctx, buf, count, op):
        try:
            t = torch.frombuffer((ctypes.c_double * count).from_address(ctypes.addressof(buf.contents)), dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX if op else dist.ReduceOp.SUM, group=group)
            return 0
        except Exception as e:  # noqa: BLE001
            print("transport allreduce failed:", e, flush=True)
            return 1

    return _SENDRECV(sendrecv), _ALLREDUCE(allreduce)


class TTCross:
    """One dtt_dmrgg problem resident on one MI355X (the `type(dtt) :: arg` of the reference plus the
    sweep state).  n: mode sizes arg%n(1:d); quad: list/array of per-mode weight vectors (rank-1 TT)."""

    def __init__(self, n, fun_id, par, maxrank, pivoting=3, accuracy=None, quad=None, tru=None, aux=None,
                 nproc=1, mybonds=None, device=0, verbose=False, arith=None, world_rank=0, world_size=1):
        L = load_library()
        self._n = np.ascontiguousarray(n, dtype=np.int32)
        self.d = int(self._n.size)
        self._par = np.ascontiguousarray(par, dtype=np.float64)
        self._aux = None if aux is None else np.ascontiguousarray(aux, dtype=np.float64)
        self._quad = None if quad is None else np.ascontiguousarray(np.concatenate([np.asarray(q, dtype=np.float64).ravel() for q in quad]))
        self._mybonds = None if mybonds is None else np.ascontiguousarray(mybonds, dtype=np.int32)
        c = _Config()
        c.d = self.d
        c.n = _ip(self._n)
        c.fun_id = fun_id
        c.par = _dp(self._par)
        c.npar = self._par.size
        c.aux = _dp(self._aux)
        c.naux = 0 if self._aux is None else self._aux.size
        c.quadw = _dp(self._quad)
        c.accuracy = -1.0 if accuracy is None else float(accuracy)
        c.maxrank = int(maxrank)
        c.pivoting = int(pivoting)
        c.tru = 0.0 if tru is None else float(tru)
        c.has_tru = 0 if tru is None else 1
        c.nproc = int(nproc)
        c.mybonds = _ip(self._mybonds)
        c.device = int(device)
        c.world_rank, c.world_size = int(world_rank), int(world_size)
        self.world_rank, self.world_size = int(world_rank), int(world_size)
        c.verbose = 1 if verbose else 0
        c.arith = 1 if arith in (1, "fast") else 0      # None / "exact": exact unless TTX_ARITH=fast is set
        self.device = int(device)
        self._h = c_void_p()
        _check(L.ttx_create(ctypes.byref(self._h), ctypes.byref(c)))

    # ---- trains that do not come from a sweep (lib/ttio.f90) -----------------------------------
    @classmethod
    def _adopt(cls, handle, device=0):
        L = load_library()
        self = cls.__new__(cls)
        self._h = handle
        self.device = int(device)
        d = c_int32()
        _check(L.ttx_get_modes(handle, ctypes.byref(d), None))
        self.d = d.value
        self._n = np.zeros(self.d, dtype=np.int32)
        _check(L.ttx_get_modes(handle, ctypes.byref(d), _ip(self._n)))
        self.world_rank, self.world_size = 0, 1
        return self

    @classmethod
    def from_cores(cls, cores, device=0):
        """Upload a train given as (r(k-1), n(k), r(k)) arrays; it becomes the resident train of a new engine."""
        cores = [np.asarray(c, dtype=np.float64) for c in cores]
        n = np.array([c.shape[1] for c in cores], dtype=np.int32)
        r = np.array([cores[0].shape[0]] + [c.shape[2] for c in cores], dtype=np.int32)
        flat = np.ascontiguousarray(np.concatenate([c.ravel(order="F") for c in cores]))
        h = c_void_p()
        _check(load_library().ttx_from_tt(ctypes.byref(h), len(cores), _ip(n), _ip(r), _dp(flat), int(device)))
        return cls._adopt(h, device)

    @classmethod
    def read(cls, path, device=0):
        """dtt_read (lib/ttio.f90:196-297): load the reference's stream file onto the device."""
        h = c_void_p()
        _check(load_library().ttx_read(ctypes.byref(h), os.fsencode(path), int(device)))
        return cls._adopt(h, device)

    def write_hdf5(self, path):
        """save_dtt_to_hdf5 (lib/utils.f90:8-57): group TT with modes, ranks and core_k."""
        L = load_library()
        L.ttx_write_hdf5.argtypes = [c_void_p, ctypes.c_char_p]
        _check(L.ttx_write_hdf5(self._h, os.fsencode(path)))

    @classmethod
    def read_hdf5(cls, path, device=0):
        L = load_library()
        L.ttx_read_hdf5.argtypes = [POINTER(c_void_p), ctypes.c_char_p, c_int32]
        h = c_void_p()
        _check(L.ttx_read_hdf5(ctypes.byref(h), os.fsencode(path), int(device)))
        return cls._adopt(h, device)

    def replicate(self):
        """The train of a multi-process job gathered onto this process as a new single-process engine (collective; include/ttx.h)."""
        L = load_library()
        L.ttx_replicate.argtypes = [c_void_p, POINTER(c_void_p)]
        h = c_void_p()
        _check(L.ttx_replicate(self._h, ctypes.byref(h)))
        return TTCross._adopt(h, self.device)

    def write(self, path):
        """dtt_write (lib/ttio.f90:29-108): the resident train in the reference's stream format."""
        _check(load_library().ttx_write(self._h, os.fsencode(path)))

    def close(self):
        if getattr(self, "_h", None):
            load_library().ttx_destroy(self._h)
            self._h = None

    __del__ = close

    # ---- multi-GPU bootstrap (replaces mpi_init of the drivers) ---------------------------------------
    def comm_init(self, dist):
        """RCCL transport: rank 0 creates the unique id, torch.distributed broadcasts it, every rank joins."""
        import torch
        L = load_library()
        buf = (c_uint8 * 128)()
        if self.world_rank == 0:
            _check(L.ttx_comm_unique_id(buf))
        dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
        t = torch.tensor(list(buf), dtype=torch.uint8, device=dev)
        dist.broadcast(t, src=0)
        ids = t.cpu().tolist()
        for i in range(128):
            buf[i] = ids[i]
        _check(L.ttx_comm_init(self._h, buf))

    def comm_init_shm(self, name):
        """The engine's built-in node-local transport over POSIX shared memory (include/ttx.h: ttx_comm_init_shm): every
        rank of the job passes the same name.  No MPI, no RCCL, no torch.distributed."""
        L = load_library()
        L.ttx_comm_init_shm.argtypes = [c_void_p, ctypes.c_char_p]
        _check(L.ttx_comm_init_shm(self._h, name.encode()))

    def set_dist_transport(self, dist, group=None):
        """Host-callback transport over torch.distributed CPU tensors (gloo): used where RCCL cannot run
        (several ranks on one GPU) -- same engine code path, messages staged through pinned host memory."""
        self._cb = make_dist_transport(dist, group)                   # keep the thunks alive
        tr = _Transport(None, self._cb[0], self._cb[1])
        _check(load_library().ttx_set_transport(self._h, ctypes.byref(tr)))

    def set_integrand_host(self, fun_addr, par=None):
        """The reference's user callback `fun(m, ind, n, par)` (lib/dmrgg.f90:18) for an engine created with
        fun_id = TTX_FUN_HOST: fun_addr is the address of a C / Fortran function with that interface (everything by
        reference), par the array handed to it untouched.  Fibers are then evaluated on the host, the sweep on the GPU."""
        self._hpar = None if par is None else np.ascontiguousarray(par, dtype=np.float64)
        _check(load_library().ttx_set_integrand_host(self._h, c_void_p(fun_addr), _dp(self._hpar)))
        return self

    def set_integrand_device(self, image_or_path, name, par=None):
        """The user's `fun` on the DEVICE for an engine created with fun_id = TTX_FUN_DEVICE (include/ttx.h): a code object --
        bytes, or the path of a file compile_device_fun wrote -- that holds the integrand `name` (TTX_DEVICE_INTEGRAND(name) of
        include/ttx_device_fun.h).  par is COPIED to the device.  Setting an integrand again replaces the first."""
        L = load_library()
        p = np.zeros(0) if par is None else np.ascontiguousarray(par, dtype=np.float64)
        if isinstance(image_or_path, (bytes, bytearray, memoryview)):
            img = bytes(image_or_path)
            _check(L.ttx_set_integrand_device(self._h, img, len(img), name.encode(), _dp(p) if p.size else None, p.size))
        else:
            _check(L.ttx_set_integrand_device_file(self._h, os.fsencode(image_or_path), name.encode(), _dp(p) if p.size else None, p.size))
        return self

    @classmethod
    def of_trains(cls, trains, op, maxrank, accuracy=None, pivoting=3, quad=None, nproc=1, combiner=None, par=None, device=None):
        """An engine whose integrand is a function of resident trains, fun(i) = g(x_1(i), .., x_m(i)) (include/ttx.h:
        TTX_FUN_TRAINS): mode sizes from trains[0], the integrand set (set_integrand_trains); .run() is the cross sweep.
        op: TTX_TOP_PRODUCT / _RATIO / _SQRTABS or their names in TRAIN_OPS; with combiner = (image_or_path, name) the loaded
        combiner of include/ttx_device_fun.h (TTX_DEVICE_COMBINER) is used instead and op is ignored."""
        trains = list(trains)
        if not trains:
            raise ValueError("of_trains: at least one train")
        tt = cls(trains[0]._n, TTX_FUN_TRAINS, [], maxrank, pivoting=pivoting, accuracy=accuracy, quad=quad, nproc=nproc,
                 device=trains[0].device if device is None else device)
        try:
            return tt.set_integrand_trains(trains, combiner if combiner is not None else op, par)
        except Exception:
            tt.close()
            raise

    def set_integrand_trains(self, trains, op, par=None):
        """The operands and the combiner of an engine created with fun_id = TTX_FUN_TRAINS (include/ttx.h).  op: a TTX_TOP_* value,
        its name in TRAIN_OPS, or (image_or_path, name) for a loaded combiner, whose par is COPIED to the device.  The engine records
        the operands' handles and looks at them again at the start of every run / accchk / eval_device; this wrapper keeps the
        operand objects referenced so that they cannot be collected while registered."""
        L = load_library()
        trains = list(trains)
        hs = (c_void_p * max(len(trains), 1))(*[t._h if t is not None else None for t in trains])
        if isinstance(op, (tuple, list)):
            image_or_path, name = op
            p = np.zeros(0) if par is None else np.ascontiguousarray(par, dtype=np.float64)
            pp = _dp(p) if p.size else None
            if isinstance(image_or_path, (bytes, bytearray, memoryview)):
                img = bytes(image_or_path)
                _check(L.ttx_set_integrand_trains_device(self._h, len(trains), hs, img, len(img), name.encode(), pp, p.size))
            else:
                _check(L.ttx_set_integrand_trains_device_file(self._h, len(trains), hs, os.fsencode(image_or_path), name.encode(), pp, p.size))
        else:
            _check(L.ttx_set_integrand_trains(self._h, len(trains), hs, int(TRAIN_OPS.get(op, op))))
        self._operands = trains
        return self

    def trainfun_last(self):
        """Of the last run / eval_device of a TTX_FUN_TRAINS engine: {'ms', 'launches', 'elements'} of the slot kernel (ms needs
        set_profile(True)) (include/ttx.h: ttx_trainfun_last)."""
        ms, nl, ne = c_double(), c_int64(), c_int64()
        _check(load_library().ttx_trainfun_last(self._h, ctypes.byref(ms), ctypes.byref(nl), ctypes.byref(ne)))
        return dict(ms=ms.value, launches=nl.value, elements=ne.value)

    @classmethod
    def pullback(cls, layers, ref, fun, maxrank, accuracy=None, pivoting=3, quad=None, nproc=1, par=None, device=None):
        """An engine whose integrand is a loaded device function of a point pulled back through resident squared-train transports
        (include/ttx.h: TTX_FUN_PULLBACK): the next layer of a layered transport.  layers: a list of (train, nodes, gamma), layer 1
        first (the outermost, built first; its nodes span the physical box, the others run from 0 to 1); ref: the reference grid in
        [0, 1], one array for all modes or a list of d -- its sizes are the engine's mode sizes; fun: (image_or_path, name) of a
        TTX_DEVICE_COMBINER called with v = [x_1 .. x_d, logq, val], or None to record the layers only (pullback_points works, run
        does not).  .run() is the cross sweep."""
        layers = list(layers)
        if not layers:
            raise ValueError("pullback: at least one layer")
        d = layers[0][0].d
        refs = [ref] * d if not isinstance(ref, (list, tuple)) or (len(ref) and np.ndim(ref[0]) == 0) else list(ref)
        refs = [np.ascontiguousarray(r, dtype=np.float64).ravel() for r in refs]
        tt = cls([r.size for r in refs], TTX_FUN_PULLBACK, [], maxrank, pivoting=pivoting, accuracy=accuracy, quad=quad, nproc=nproc,
                 device=layers[0][0].device if device is None else device)
        try:
            return tt.set_integrand_pullback(layers, refs, fun, par)
        except Exception:
            tt.close()
            raise

    def set_integrand_pullback(self, layers, ref, fun=None, par=None):
        """The layers, the reference grid and the combiner of an engine created with fun_id = TTX_FUN_PULLBACK (include/ttx.h).
        layers: a list of (train, nodes, gamma); ref: one array for all modes or a list of d; fun: (image_or_path, name) or None; par
        is COPIED to the device.  The engine records the layers' handles and looks at them again at the start of every run / accchk /
        eval_device / pullback_points; this wrapper keeps the layer objects referenced."""
        L = load_library()
        layers = [tuple(y) for y in layers]
        arr = (_Layer * max(len(layers), 1))()
        keep = []
        for t, (x, nodes, gamma) in enumerate(layers):
            arr[t].x = x._h if x is not None else None
            arr[t].gamma = float(gamma)
            if x is not None and nodes is not None:
                _, rowp = x._node_rows(nodes, f"set_integrand_pullback: layer {t + 1}")
                arr[t].nodes = ctypes.cast(rowp, POINTER(POINTER(c_double)))
                keep.append(rowp)
        refs = [ref] * self.d if not isinstance(ref, (list, tuple)) or (len(ref) and np.ndim(ref[0]) == 0) else list(ref)
        _, refp = self._node_rows(refs, "set_integrand_pullback: ref")
        p = np.zeros(0) if par is None else np.ascontiguousarray(par, dtype=np.float64)
        pp = _dp(p) if p.size else None
        if fun is None:
            _check(L.ttx_set_integrand_pullback(self._h, len(layers), arr, refp, None, 0, None, pp, p.size))
        else:
            image_or_path, name = fun
            if isinstance(image_or_path, (bytes, bytearray, memoryview)):
                img = bytes(image_or_path)
                _check(L.ttx_set_integrand_pullback(self._h, len(layers), arr, refp, img, len(img), name.encode(), pp, p.size))
            else:
                _check(L.ttx_set_integrand_pullback_file(self._h, len(layers), arr, refp, os.fsencode(image_or_path), name.encode(), pp, p.size))
        self._operands = [y[0] for y in layers]
        return self

    def pullback_points(self, ind):
        """x (npts, d), logq and val of a TTX_FUN_PULLBACK engine at the multi-indices ind (npts x d, 1-based): the reference grid's
        points pulled back through the layers, bit for bit the chain of sample_sq_real(.., mode="exact") calls (include/ttx.h:
        ttx_pullback_points).  A failed sample has x NaN, logq NaN and val 0."""
        ind = np.ascontiguousarray(ind, dtype=np.int32).reshape(-1, self.d)
        x, lq, v = np.zeros((ind.shape[0], self.d)), np.zeros(ind.shape[0]), np.zeros(ind.shape[0])
        _check(load_library().ttx_pullback_points(self._h, ind.shape[0], _ip(ind), _dp(x), _dp(lq), _dp(v)))
        return x, lq, v

    def pullback_last(self):
        """Of the last run / eval_device / pullback_points of a TTX_FUN_PULLBACK engine: {'ms', 'launches', 'elements', 'failed'} of
        the transport kernel (ms needs set_profile(True)) (include/ttx.h: ttx_pullback_last)."""
        ms, nl, ne, nf = c_double(), c_int64(), c_int64(), c_int64()
        _check(load_library().ttx_pullback_last(self._h, ctypes.byref(ms), ctypes.byref(nl), ctypes.byref(ne), ctypes.byref(nf)))
        return dict(ms=ms.value, launches=nl.value, elements=ne.value, failed=nf.value)

    def eval_device(self, ind):
        """The loaded device integrand at the multi-indices ind (npts x d, 1-based), through the code object's list kernel; for a
        TTX_FUN_TRAINS engine the operands at those indices and the combiner, for a TTX_FUN_PULLBACK engine the combiner at the
        pulled-back points."""
        ind = np.ascontiguousarray(ind, dtype=np.int32).reshape(-1, self.d)
        out = np.zeros(ind.shape[0])
        _check(load_library().ttx_eval_device(self._h, ind.shape[0], _ip(ind), _dp(out)))
        return out

    @property
    def host_calls(self):
        return int(load_library().ttx_host_calls(self._h))

    @property
    def fun_id(self):
        """TTX_FUN_* the engine was created with (include/ttx.h: ttx_fun_id)."""
        L = load_library()
        L.ttx_fun_id.argtypes = [c_void_p]
        return L.ttx_fun_id(self._h)

    @property
    def arith(self):
        """'exact' or 'fast': the arithmetic the integrand is evaluated with (include/ttx.h: ttx_arith)."""
        L = load_library()
        L.ttx_arith.argtypes = [c_void_p]
        return ("exact", "fast")[L.ttx_arith(self._h)]

    def sweep_path(self):
        """'chain', 'fused' or 'cluster': the sweep implementation chosen at creation (TTX_SWEEP)."""
        L = load_library()
        L.ttx_sweep_path.argtypes = [c_void_p]
        return ("chain", "fused", "cluster")[L.ttx_sweep_path(self._h)]

    def plan(self):
        """The kernels the engine would launch now, stage by stage: {'path': .., 'tables': .., 'lottery': .., 'halfstep': ..} (and
        'fullpiv' with pivoting -1), the values as include/ttx.h writes them (ttx_plan_describe)."""
        L = load_library()
        L.ttx_plan_describe.argtypes = [c_void_p, c_char_p, c_int64]
        buf = ctypes.create_string_buffer(1024)
        _check(L.ttx_plan_describe(self._h, buf, len(buf)))
        return dict(line.split(": ", 1) for line in buf.value.decode().splitlines())

    def cluster_eval(self):
        """Integrand evaluator of the cluster sweep kernel: 'none' (not on that path), 'predicated' (exact, remainders of the
        chains tested per step: TTX_CL_PAD=0 or a node outside [0,1]), 'chunks' (exact, rows padded to whole chunks) or 'closed'
        (TTX_ARITH=fast) (include/ttx.h: ttx_cluster_eval)."""
        L = load_library()
        L.ttx_cluster_eval.argtypes = [c_void_p]
        return ("none", "predicated", "chunks", "closed")[L.ttx_cluster_eval(self._h)]

    @property
    def resid_halfsteps(self):
        L = load_library()
        L.ttx_resid_halfsteps.argtypes = [c_void_p]
        L.ttx_resid_halfsteps.restype = c_int64
        return int(L.ttx_resid_halfsteps(self._h))

    @property
    def cluster_fallbacks(self):
        """Runs replayed on the chain path after a wait inside the cluster sweep kernel timed out (include/ttx.h)."""
        L = load_library()
        L.ttx_cluster_fallbacks.argtypes = [c_void_p]
        return int(L.ttx_cluster_fallbacks(self._h))

    def cluster_entry(self):
        """The entry of a cluster launch (include/ttx.h: ttx_cluster_entry): the forms in force ('powtab', 'word', 'lists') and how
        many launches of the last run took the carried pivot lists and the carried generator word (local group 0)."""
        L = load_library()
        L.ttx_cluster_entry.argtypes = [c_void_p, ctypes.POINTER(c_int64)]
        out = (c_int64 * 3)()
        _check(L.ttx_cluster_entry(self._h, out))
        return {"powtab": bool(out[0] & 1), "word": bool(out[0] & 2), "lists": bool(out[0] & 4), "lists_taken": int(out[1]), "word_taken": int(out[2])}

    def sweep_gap(self):
        """The forms of the stretch between two sweeps in force (include/ttx.h: ttx_sweep_gap): 'tail_event' is 'kernel' or 'marker',
        'tail_event_fallbacks' counts the refusals of the extended launch."""
        L = load_library()
        L.ttx_sweep_gap.argtypes = [c_void_p, ctypes.POINTER(ctypes.c_int32)]
        out = (ctypes.c_int32 * 4)()
        _check(L.ttx_sweep_gap(self._h, out))
        return {"tail_event": "kernel" if out[0] else "marker", "tail_event_fallbacks": int(out[1]), "tail_lean": bool(out[2]),
                "cl_pack2": bool(out[3])}

    @property
    def det_fallbacks(self):
        """Runs repeated without the wave teams / relay of the Ising D/E half-step after a reported fault (include/ttx.h)."""
        L = load_library()
        L.ttx_det_fallbacks.argtypes = [c_void_p]
        return int(L.ttx_det_fallbacks(self._h))

    def set_profile(self, on=True):
        _check(load_library().ttx_set_profile(self._h, 1 if on else 0))

    def run(self):
        _check(load_library().ttx_run(self._h))
        return self

    # ---- results -----------------------------------------------------------------------------
    @property
    def neval(self):
        return int(load_library().ttx_neval(self._h))

    @property
    def seconds(self):
        return float(load_library().ttx_seconds(self._h))

    def sweeps(self):
        L = load_library()
        k = L.ttx_num_sweeps(self._h)
        buf = (SweepRec * k)()
        _check(L.ttx_get_sweeps(self._h, buf, k))
        return [dict(it=b.it, dir=b.dir, erank=b.erank, neval=b.neval, val=b.val, amax=b.amax,
                     pivotmax=b.pivotmax, pivotmin=b.pivotmin, seconds=b.seconds) for b in buf]

    def tapes(self):
        L = load_library()
        k = L.ttx_num_sweeps(self._h) - 1
        out = np.zeros((max(k, 0), self.d + 1, 4), dtype=np.int32)
        if k > 0:
            _check(L.ttx_get_tapes(self._h, _ip(out), out.size))
        return out

    def fast_tables(self, group, side=None, bond=None, cols=None):
        """Tables of the fast evaluators as the run left them (include/ttx.h: ttx_fast_tables).  Without side / bond: (first, last)
        of the local group.  Else dict(r, idx [len][r], near, dv [d+1][r], piv [8][r]) of the left (side 0) / right (side 1) pivots
        of `bond`; cols: an upper bound of the bond's rank (default 4096)."""
        L = load_library()
        L.ttx_fast_tables.argtypes = [c_void_p, c_int32, c_int32, c_int32, c_int32, POINTER(c_int32), POINTER(c_int32)] + [POINTER(c_double)] * 3
        info = np.zeros(3, dtype=np.int32)
        if side is None:
            _check(L.ttx_fast_tables(self._h, group, 0, 0, 0, _ip(info), None, None, None, None))
            return int(info[1]), int(info[2])
        cols = 4096 if cols is None else int(cols)
        d = self.d
        idx = np.zeros(d * cols, dtype=np.int32)
        near, dv, piv = np.zeros((d + 1) * cols), np.zeros((d + 1) * cols), np.zeros(8 * cols)
        _check(L.ttx_fast_tables(self._h, group, side, bond, cols, _ip(info), _ip(idx), _dp(near), _dp(dv), _dp(piv)))
        r = int(info[0])
        ln = bond if side == 0 else d - bond
        return dict(r=r, idx=idx[:d * r].reshape(d, r)[:ln], near=near[:(d + 1) * r].reshape(d + 1, r), dv=dv[:(d + 1) * r].reshape(d + 1, r),
                    piv=piv[:8 * r].reshape(8, r))

    def ranks(self):
        r = np.zeros(self.d + 1, dtype=np.int32)
        _check(load_library().ttx_get_ranks(self._h, _ip(r)))
        return r

    def core(self, k):
        """arg%u(k)%p as a Fortran-ordered (r(k-1), n(k), r(k)) array, k = 1..d."""
        L = load_library()
        r = self.ranks()
        sz = L.ttx_core_size(self._h, k)
        buf = np.zeros(sz, dtype=np.float64)
        _check(L.ttx_get_core(self._h, k, _dp(buf)))
        return buf.reshape((r[k - 1], self._n[k - 1], r[k]), order="F")

    def _weights(self, w, who):
        """per-mode weight vectors as the concatenated block the C entry points take (on trust, as the reference takes its rank-1 train)"""
        if w is None:
            return None
        if len(w) != self.d or any(np.size(q) != int(nk) for q, nk in zip(w, self._n)):
            raise ValueError(f"{who}: {self.d} weight vectors of lengths {list(map(int, self._n))} expected")
        return np.ascontiguousarray(np.concatenate([np.asarray(q, dtype=np.float64).ravel() for q in w]))

    def quad(self, w=None):
        """dtt_quad(arg, quad) (lib/dmrgg.f90:1261); w = list of per-mode weight vectors or None."""
        v = c_double()
        wa = self._weights(w, "quad")
        _check(load_library().ttx_quad(self._h, _dp(wa), ctypes.byref(v)))
        return v.value

    def contract(self, keep, w=None):
        """The train with the modes where keep is 0 / False summed against their weights (include/ttx.h: ttx_contract), as a new
        engine on the same device; keep: d booleans or 0 / 1, at least two kept; w as for quad (the vectors of kept modes are
        ignored), None = plain sums.  A slice is a contraction with a unit vector.  No core crosses the host link."""
        k = np.asarray(keep)
        if k.ndim != 1 or k.size != self.d:
            raise ValueError(f"contract: {self.d} keep flags expected")
        k = np.ascontiguousarray(k.astype(np.int32))
        wa = self._weights(w, "contract")
        h = c_void_p()
        _check(load_library().ttx_contract(self._h, _ip(k), _dp(wa), ctypes.byref(h)))
        return TTCross._adopt(h, self.device)

    def marginals(self, w=None):
        """All d one-mode marginals (include/ttx.h: ttx_marginals): a list of d arrays, entry k of length n(k) = the train summed
        over every other mode against its weights (w as for quad, None = plain sums)."""
        out = np.zeros(int(self._n.sum()))
        _check(load_library().ttx_marginals(self._h, _dp(self._weights(w, "marginals")), _dp(out)))
        return [a.copy() for a in np.split(out, np.cumsum(self._n)[:-1])]

    def contract_modesum(self):
        """(milliseconds, bytes) of the mode-sum kernel of the last contract / marginals (include/ttx.h: ttx_contract_modesum)"""
        ms, by = c_double(), c_double()
        _check(load_library().ttx_contract_modesum(self._h, ctypes.byref(ms), ctypes.byref(by)))
        return ms.value, by.value

    # ---- sums and elementwise products of resident trains (include/ttx.h: ttx_lincomb, ttx_hadamard) -----
    @staticmethod
    def lincomb(coefs, trains):
        """sum_t coefs[t] * trains[t] as a new engine on the same device: ranks add on the interior bonds, the first cores are
        multiplied by their coefficients, everything else is copied (block diagonal cores with explicit zeros).  The same train
        may appear several times.  Rank sums above 128 are refused: round the terms, or fewer of them, first (svd).  No core
        crosses the host link."""
        trains = list(trains)
        c = np.ascontiguousarray(np.asarray(coefs, dtype=np.float64).ravel())
        if not trains or c.size != len(trains):
            raise ValueError(f"lincomb: one coefficient per train expected (got {c.size} and {len(trains)})")
        hs = (c_void_p * len(trains))(*[t._h for t in trains])
        h = c_void_p()
        _check(load_library().ttx_lincomb(len(trains), _dp(c), hs, ctypes.byref(h)))
        return TTCross._adopt(h, trains[0].device)

    def axpby(self, alpha, beta, y):
        """alpha * self + beta * y (lincomb of two trains)"""
        return TTCross.lincomb([alpha, beta], [self, y])

    def hadamard(self, y):
        """The elementwise product self(i) * y(i) as a new engine on the same device: ranks multiply (products above 128 are
        refused), the index of self runs fastest on both bonds; y may be self."""
        h = c_void_p()
        _check(load_library().ttx_hadamard(self._h, y._h, ctypes.byref(h)))
        return TTCross._adopt(h, self.device)

    def dist(self, y):
        """|self - y| in the Frobenius norm as norm(self - y): the QR-based norm of the difference train keeps what
        sqrt(dot(x,x) - 2 dot(x,y) + dot(y,y)) loses to cancellation below sqrt(2^-53) |x|"""
        t = TTCross.lincomb([1.0, -1.0], [self, y])
        try:
            return t.norm()
        finally:
            t.close()

    def wdot(self, y, w=None):
        """sum_i w(i) self(i) y(i) with rank-1 weights w as for quad (None: plain sum): quad of the elementwise product"""
        t = self.hadamard(y)
        try:
            return t.quad(w)
        finally:
            t.close()

    def algebra_last(self):
        """(milliseconds, bytes read, bytes written) of the assembly kernel of the last lincomb / hadamard that had this engine
        as its first operand (include/ttx.h: ttx_algebra_last)"""
        ms, rd, wr = c_double(), c_double(), c_double()
        _check(load_library().ttx_algebra_last(self._h, ctypes.byref(ms), ctypes.byref(rd), ctypes.byref(wr)))
        return ms.value, rd.value, wr.value

    # ---- a rounded sum of resident trains (include/ttx.h: ttx_lincomb_round) -----------------------------
    @staticmethod
    def lincomb_round(coefs, trains, rank=0, tol=-1.0, rmax=0, seed=0, mode="auto"):
        """sum_t coefs[t] * trains[t] rounded on the device by a randomized sketch of rank `rank` (0: 128), as a new engine on
        the same device (include/ttx.h: ttx_lincomb_round): no core of rank sum_t r_t is ever formed, so sums far beyond the
        engine's rank cap of 128 are taken (up to 256 terms, rank sums up to 4096).  tol < 0 returns the left-orthogonal train
        with the sketch ranks, tol >= 0 truncates it as svd(tol, rmax) does.  The same train may appear several times; a call
        with the same seed repeats bit for bit.  mode: "exact", "mfma" or "auto"; trains[0].roundsum_last() tells what ran."""
        trains = list(trains)
        c = np.ascontiguousarray(np.asarray(coefs, dtype=np.float64).ravel())
        if not trains or c.size != len(trains):
            raise ValueError(f"lincomb_round: one coefficient per train expected (got {c.size} and {len(trains)})")
        md = _eval_mode(mode)
        hs = (c_void_p * len(trains))(*[t._h for t in trains])
        h = c_void_p()
        _check(load_library().ttx_lincomb_round(len(trains), _dp(c), hs, int(rank), float(tol), int(rmax), int(seed) & (2 ** 64 - 1), md, ctypes.byref(h)))
        return TTCross._adopt(h, trains[0].device)

    def roundsum_last(self):
        """dict(ms_sketch, ms_gemm, ms_qr, ms_advance, flops, l, mode) of the last lincomb_round that had this engine as its first
        operand (include/ttx.h: ttx_roundsum_last): l are the sketch ranks l(0 .. d), mode is "exact" or "mfma" (None before the
        first call)"""
        ms, fl, md = (c_double * 4)(), c_double(), c_int32()
        l = np.zeros(self.d + 1, dtype=np.int32)
        _check(load_library().ttx_roundsum_last(self._h, ms, ctypes.byref(fl), _ip(l), ctypes.byref(md)))
        names = {v: k for k, v in EVAL_MODES.items()}
        return dict(ms_sketch=ms[0], ms_gemm=ms[1], ms_qr=ms[2], ms_advance=ms[3], flops=fl.value, l=[int(v) for v in l], mode=names.get(md.value))

    # ---- matrices applied to chosen modes (include/ttx.h: ttx_mode_apply) --------------------------------
    def mode_apply(self, mats, mode="auto"):
        """The train with a matrix applied to chosen modes, G'_k(a, j, b) = sum_i A_k[j, i] G_k(a, i, b) (include/ttx.h:
        ttx_mode_apply), as a new engine on the same device: ranks stay, mode k gets m_k indices.  mats: d entries, None = the mode
        is left alone (its core is copied bit for bit), otherwise an (m_k, n_k) array; or a dict {mode (1-based): array}.  mode:
        "exact" (ascending i, separate multiply and add), "mfma" (fp64 matrix cores) or "auto"; mode_apply_last() tells what ran.
        When every matrix is a float64 torch tensor on the engine's device they are passed by pointer (ttx_mode_apply_dev).
        No core crosses the host link."""
        L, md = load_library(), _eval_mode(mode)
        if isinstance(mats, dict):
            bad = [k for k in mats if not (isinstance(k, (int, np.integer)) and 1 <= k <= self.d)]
            if bad:
                raise ValueError(f"mode_apply: modes 1..{self.d} expected as keys (got {bad})")
            mats = [mats.get(k) for k in range(1, self.d + 1)]
        mats = list(mats)
        if len(mats) != self.d:
            raise ValueError(f"mode_apply: {self.d} entries expected (None leaves a mode alone), got {len(mats)}")
        is_torch = [a is not None and type(a).__module__.split(".")[0] == "torch" for a in mats]
        for k, a in enumerate(mats):
            if a is None:
                continue
            shape = tuple(a.shape)
            if len(shape) != 2 or shape[0] < 1 or shape[1] != int(self._n[k]):
                raise ValueError(f"mode_apply: the matrix of mode {k + 1} has shape {shape}, (m, {int(self._n[k])}) with m >= 1 expected")
        m = np.ascontiguousarray([0 if a is None else int(a.shape[0]) for a in mats], dtype=np.int32)
        h = c_void_p()
        if any(is_torch) and all(t or a is None for t, a in zip(is_torch, mats)) and all(a.is_cuda for a in mats if a is not None):
            import torch
            ts = [a for a in mats if a is not None]
            if any(a.device.index != self.device for a in ts):
                raise ValueError(f"mode_apply: the matrices lie on another device than the engine's ({self.device})")
            if any(a.dtype != torch.float64 for a in ts):
                raise ValueError("mode_apply: float64 tensors expected")
            flat = torch.cat([a.t().contiguous().reshape(-1) for a in ts])    # column-major blocks, assembled on the device
            torch.cuda.current_stream(flat.device).synchronize()             # the engine runs on a stream of its own
            _check(L.ttx_mode_apply_dev(self._h, _ip(m), c_void_p(flat.data_ptr()), md, ctypes.byref(h)))
            return TTCross._adopt(h, self.device)
        blocks = [np.asarray(a.cpu().numpy() if t else a, dtype=np.float64).ravel(order="F") for a, t in zip(mats, is_torch) if a is not None]
        flat = np.ascontiguousarray(np.concatenate(blocks)) if blocks else None
        _check(L.ttx_mode_apply(self._h, _ip(m), _dp(flat), md, ctypes.byref(h)))
        return TTCross._adopt(h, self.device)

    def mode_apply_last(self):
        """dict(ms, bytes_read, bytes_written, flops, mode) of the apply launch of the last mode_apply on this engine (include/ttx.h:
        ttx_mode_apply_last); mode is "exact" or "mfma" (None before the first call)"""
        ms, rd, wr, fl, md = c_double(), c_double(), c_double(), c_double(), c_int32()
        _check(load_library().ttx_mode_apply_last(self._h, ctypes.byref(ms), ctypes.byref(rd), ctypes.byref(wr), ctypes.byref(fl), ctypes.byref(md)))
        names = {v: k for k, v in EVAL_MODES.items()}
        return dict(ms=ms.value, bytes_read=rd.value, bytes_written=wr.value, flops=fl.value, mode=names.get(md.value))

    # ---- the train in a function basis at real points (include/ttx.h: ttx_basis_batch) -------------------
    def _dev_pair(self, who, t, cols):
        """a float64 torch tensor (npts, cols) on the engine's device and the tensor of its values; None for anything else"""
        if type(t).__module__.split(".")[0] != "torch" or not t.is_cuda:
            return None
        import torch
        if t.device.index != self.device:
            raise ValueError(f"{who}: the tensor lies on {t.device}, the engine on device {self.device}")
        if t.dtype != torch.float64 or not t.is_contiguous() or t.dim() != 2 or t.shape[1] != cols:
            raise ValueError(f"{who}: a contiguous float64 tensor of shape (npts, {cols}) expected")
        out = torch.empty(t.shape[0], dtype=torch.float64, device=t.device)
        torch.cuda.current_stream(t.device).synchronize()            # the engine runs on a stream of its own
        return out

    def basis_batch(self, x, basis, mode="auto"):
        """f(x_p) = sum_i T(i) prod_m phi_(m, i_m)(x[p, m]) at real points x (npts, d) (include/ttx.h: ttx_basis_batch).  basis: a
        list of d entries ("cos", a, b[, halve_first]) or ("linear", nodes), or one entry for all modes; the tables are formed on
        the device (basis_table gives the same numbers on the host).  mode "exact", "mfma" or "auto"; basis_last() tells what ran.
        A host array gives a numpy array; a contiguous float64 torch tensor on the engine's device goes by pointer
        (ttx_basis_batch_dev) and gives a tensor on that device."""
        L, md = load_library(), _eval_mode(mode)
        if isinstance(basis, (tuple, list)) and basis and isinstance(basis[0], str):
            basis = [basis] * self.d
        basis = list(basis)
        if len(basis) != self.d:
            raise ValueError(f"basis_batch: {self.d} basis entries expected (got {len(basis)})")
        pairs = [_basis_struct(e, self._n[k]) for k, e in enumerate(basis)]
        arr = (_Basis * self.d)(*[p[0] for p in pairs])          # pairs keeps the node arrays alive
        out = self._dev_pair("basis_batch", x, self.d)
        if out is not None:
            _check(L.ttx_basis_batch_dev(self._h, x.shape[0], c_void_p(x.data_ptr()), arr, c_void_p(out.data_ptr()), md))
            return out
        if type(x).__module__.split(".")[0] == "torch":
            x = x.numpy()
        xa = np.ascontiguousarray(x, dtype=np.float64)
        if xa.ndim != 2 or xa.shape[1] != self.d:
            raise ValueError(f"basis_batch: an array of shape (npts, {self.d}) expected")
        res = np.zeros(xa.shape[0])
        _check(L.ttx_basis_batch(self._h, xa.shape[0], _dp(xa), arr, _dp(res), md))
        return res

    def basis_tab(self, phi, mode="auto"):
        """The same with the caller's own tables (include/ttx.h: ttx_basis_tab): phi (npts, sum n), the n(k) numbers of mode 1
        first.  Host arrays and torch tensors on the engine's device (read in place, ttx_basis_tab_dev) as for basis_batch."""
        L, md = load_library(), _eval_mode(mode)
        sumn = int(self._n.sum())
        out = self._dev_pair("basis_tab", phi, sumn)
        if out is not None:
            _check(L.ttx_basis_tab_dev(self._h, phi.shape[0], c_void_p(phi.data_ptr()), c_void_p(out.data_ptr()), md))
            return out
        if type(phi).__module__.split(".")[0] == "torch":
            phi = phi.numpy()
        pa = np.ascontiguousarray(phi, dtype=np.float64)
        if pa.ndim != 2 or pa.shape[1] != sumn:
            raise ValueError(f"basis_tab: an array of shape (npts, {sumn}) expected")
        res = np.zeros(pa.shape[0])
        _check(L.ttx_basis_tab(self._h, pa.shape[0], _dp(pa), _dp(res), md))
        return res

    def basis_last(self):
        """dict(ms_table, ms_chain, flops, mode) of the last basis_batch / basis_tab on this engine (include/ttx.h: ttx_basis_last);
        mode is "exact" or "mfma" (None before the first call)"""
        mt, mc, fl, md = c_double(), c_double(), c_double(), c_int32()
        _check(load_library().ttx_basis_last(self._h, ctypes.byref(mt), ctypes.byref(mc), ctypes.byref(fl), ctypes.byref(md)))
        names = {v: k for k, v in EVAL_MODES.items()}
        return dict(ms_table=mt.value, ms_chain=mc.value, flops=fl.value, mode=names.get(md.value))

    # ---- its gradient (include/ttx.h: ttx_basis_grad_batch) ----------------------------------------------
    def basis_grad_batch(self, x, basis, mode="auto"):
        """(val, grad) of f at real points x (npts, d) (include/ttx.h: ttx_basis_grad_batch): val (npts,) is basis_batch(x, basis)
        bit for bit in the mode that ran, grad (npts, d) holds df/dx_m, mode 1 first.  basis, mode and the two kinds of x (host
        array -> numpy arrays, float64 tensor on the engine's device -> tensors, by pointer) are basis_batch's; basis_grad_last()
        tells what ran.  The score of the sample_sq_real proposal is 2 val grad / (val^2 + gamma)."""
        L, md = load_library(), _eval_mode(mode)
        if isinstance(basis, (tuple, list)) and basis and isinstance(basis[0], str):
            basis = [basis] * self.d
        basis = list(basis)
        if len(basis) != self.d:
            raise ValueError(f"basis_grad_batch: {self.d} basis entries expected (got {len(basis)})")
        pairs = [_basis_struct(e, self._n[k]) for k, e in enumerate(basis)]
        arr = (_Basis * self.d)(*[p[0] for p in pairs])          # pairs keeps the node arrays alive
        val = self._dev_pair("basis_grad_batch", x, self.d)
        if val is not None:
            import torch
            grad = torch.empty((x.shape[0], self.d), dtype=torch.float64, device=x.device)
            _check(L.ttx_basis_grad_batch_dev(self._h, x.shape[0], c_void_p(x.data_ptr()), arr, c_void_p(val.data_ptr()), c_void_p(grad.data_ptr()), md))
            return val, grad
        if type(x).__module__.split(".")[0] == "torch":
            x = x.numpy()
        xa = np.ascontiguousarray(x, dtype=np.float64)
        if xa.ndim != 2 or xa.shape[1] != self.d:
            raise ValueError(f"basis_grad_batch: an array of shape (npts, {self.d}) expected")
        val, grad = np.zeros(xa.shape[0]), np.zeros((xa.shape[0], self.d))
        _check(L.ttx_basis_grad_batch(self._h, xa.shape[0], _dp(xa), arr, _dp(val), _dp(grad), md))
        return val, grad

    def basis_grad_tab(self, phi, dphi, mode="auto"):
        """The same with the caller's own tables (include/ttx.h: ttx_basis_grad_tab): phi and dphi (npts, sum n) each, in
        basis_tab's layout; any differentiable basis works.  Host arrays, or two torch tensors on the engine's device (read in
        place, ttx_basis_grad_tab_dev)."""
        L, md = load_library(), _eval_mode(mode)
        sumn = int(self._n.sum())
        val = self._dev_pair("basis_grad_tab", phi, sumn)
        if val is not None:
            import torch
            if self._dev_pair("basis_grad_tab", dphi, sumn) is None or dphi.shape != phi.shape:
                raise ValueError("basis_grad_tab: phi and dphi must be tensors of one shape on the engine's device")
            grad = torch.empty((phi.shape[0], self.d), dtype=torch.float64, device=phi.device)
            _check(L.ttx_basis_grad_tab_dev(self._h, phi.shape[0], c_void_p(phi.data_ptr()), c_void_p(dphi.data_ptr()), c_void_p(val.data_ptr()),
                                            c_void_p(grad.data_ptr()), md))
            return val, grad
        tabs = []
        for t in (phi, dphi):
            if type(t).__module__.split(".")[0] == "torch":
                t = t.cpu().numpy()
            tabs.append(np.ascontiguousarray(t, dtype=np.float64))
        pa, da = tabs
        if pa.ndim != 2 or pa.shape[1] != sumn or da.shape != pa.shape:
            raise ValueError(f"basis_grad_tab: two arrays of shape (npts, {sumn}) expected")
        val, grad = np.zeros(pa.shape[0]), np.zeros((pa.shape[0], self.d))
        _check(L.ttx_basis_grad_tab(self._h, pa.shape[0], _dp(pa), _dp(da), _dp(val), _dp(grad), md))
        return val, grad

    def basis_grad_last(self):
        """dict(ms_table, ms_back, ms_fwd, flops, mode, chunk) of the last basis_grad_batch / basis_grad_tab on this engine
        (include/ttx.h: ttx_basis_grad_last); mode is "exact" or "mfma" (None before the first call), chunk the points per chunk"""
        mt, mb, mf, fl, md, ck = c_double(), c_double(), c_double(), c_double(), c_int32(), c_int64()
        _check(load_library().ttx_basis_grad_last(self._h, ctypes.byref(mt), ctypes.byref(mb), ctypes.byref(mf), ctypes.byref(fl), ctypes.byref(md),
                                                  ctypes.byref(ck)))
        names = {v: k for k, v in EVAL_MODES.items()}
        return dict(ms_table=mt.value, ms_back=mb.value, ms_fwd=mf.value, flops=fl.value, mode=names.get(md.value), chunk=ck.value)

    # ---- the gradient with respect to the cores (include/ttx.h: ttx_basis_core_grad_batch) ----------------
    def core_offsets(self):
        """where every core's block starts in the packed gradient (and, last, its length): d + 1 numbers, mode 1 first"""
        r, n = self.ranks().astype(np.int64), self._n.astype(np.int64)
        return np.concatenate([[0], np.cumsum(r[:-1] * n * r[1:])])

    def _core_blocks(self, flat):
        """the packed gradient as a list of (r(k-1), n(k), r(k)) arrays (views of flat)"""
        off, r = self.core_offsets(), self.ranks()
        return [flat[off[k]:off[k + 1]].reshape((r[k], self._n[k], r[k + 1]), order="F") for k in range(self.d)]

    def _core_pack(self, who, g):
        """a list of blocks, or one flat array, as the packed host array"""
        off, r = self.core_offsets(), self.ranks()
        if isinstance(g, (list, tuple)):
            if len(g) != self.d or any(np.shape(b) != (r[k], self._n[k], r[k + 1]) for k, b in enumerate(g)):
                raise ValueError(f"{who}: {self.d} blocks of the cores' shapes expected")
            return np.ascontiguousarray(np.concatenate([np.asarray(b, dtype=np.float64).ravel(order="F") for b in g]))
        flat = np.ascontiguousarray(g, dtype=np.float64).reshape(-1)
        if flat.size != off[-1]:
            raise ValueError(f"{who}: {off[-1]} numbers expected (got {flat.size})")
        return flat

    def _core_grad(self, who, host, dev, head, t, cols, c, mode, out, accumulate):
        L, md, acc = load_library(), _eval_mode(mode), int(bool(accumulate))
        total = int(self.core_offsets()[-1])
        val = self._dev_pair(who, t, cols)
        if val is not None:
            import torch
            if type(c).__module__.split(".")[0] != "torch" or c.device != t.device or c.dtype != torch.float64 or not c.is_contiguous() or c.shape != (t.shape[0],):
                raise ValueError(f"{who}: c must be a contiguous float64 tensor of shape (npts,) on the engine's device")
            if out is None:
                if acc:
                    raise ValueError(f"{who}: accumulate needs out")
                out = torch.empty(total, dtype=torch.float64, device=t.device)
            elif type(out).__module__.split(".")[0] != "torch" or out.device != t.device or out.dtype != torch.float64 or not out.is_contiguous() or out.shape != (total,):
                raise ValueError(f"{who}: out must be a contiguous float64 tensor of {total} numbers on the engine's device")
            torch.cuda.current_stream(t.device).synchronize()
            _check(dev(self._h, t.shape[0], c_void_p(t.data_ptr()), *head, c_void_p(c.data_ptr()), c_void_p(val.data_ptr()), c_void_p(out.data_ptr()), acc, md))
            return val, out
        if type(t).__module__.split(".")[0] == "torch":
            t = t.cpu().numpy()
        if type(c).__module__.split(".")[0] == "torch":
            c = c.cpu().numpy()
        ta, ca = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
        if ta.ndim != 2 or ta.shape[1] != cols or ca.shape != (ta.shape[0],):
            raise ValueError(f"{who}: an array of shape (npts, {cols}) and npts weights expected")
        if out is None:
            if acc:
                raise ValueError(f"{who}: accumulate needs out")
            flat = np.zeros(total)
        else:
            flat = self._core_pack(who, out)
        val = np.zeros(ta.shape[0])
        _check(host(self._h, ta.shape[0], _dp(ta), *head, _dp(ca), _dp(val), _dp(flat), acc, md))
        return val, self._core_blocks(flat)

    def basis_core_grad(self, x, basis, c, mode="auto", out=None, accumulate=False):
        """(val, g) at real points x (npts, d) with weights c (npts,) (include/ttx.h: ttx_basis_core_grad_batch): val is
        basis_batch(x, basis) bit for bit in the mode that ran; g holds G_i = sum_p c[p] d f(x_p) / d U_i for every core -- for
        c = dLoss/df the gradient of the loss with respect to the cores.  basis and mode as for basis_batch.  Host arrays in give
        numpy out: g is a list of (r(k-1), n(k), r(k)) arrays.  Contiguous float64 torch tensors on the engine's device go by
        pointer (ttx_basis_core_grad_batch_dev) and give one flat device tensor; core_offsets() gives the block starts.  out: a
        gradient to write into (a list of blocks or a flat array on the host, a flat tensor on the device); accumulate=True adds
        onto it.  A point masked with c = 0 still needs finite coordinates.  basis_core_grad_last() tells what ran."""
        L = load_library()
        if isinstance(basis, (tuple, list)) and basis and isinstance(basis[0], str):
            basis = [basis] * self.d
        basis = list(basis)
        if len(basis) != self.d:
            raise ValueError(f"basis_core_grad: {self.d} basis entries expected (got {len(basis)})")
        pairs = [_basis_struct(e, self._n[k]) for k, e in enumerate(basis)]
        arr = (_Basis * self.d)(*[p[0] for p in pairs])          # pairs keeps the node arrays alive
        return self._core_grad("basis_core_grad", L.ttx_basis_core_grad_batch, L.ttx_basis_core_grad_batch_dev, (arr,), x, self.d, c, mode, out, accumulate)

    def basis_core_grad_tab(self, phi, c, mode="auto", out=None, accumulate=False):
        """The same with the caller's own tables (include/ttx.h: ttx_basis_core_grad_tab): phi (npts, sum n) in basis_tab's layout."""
        L = load_library()
        return self._core_grad("basis_core_grad_tab", L.ttx_basis_core_grad_tab, L.ttx_basis_core_grad_tab_dev, (), phi, int(self._n.sum()), c, mode, out, accumulate)

    def basis_core_grad_last(self):
        """dict(ms_table, ms_back, ms_fwd, ms_acc, flops, mode, chunk) of the last basis_core_grad / basis_core_grad_tab on this engine
        (include/ttx.h: ttx_basis_core_grad_last); mode is "exact" or "mfma" (None before the first call), chunk the points per chunk"""
        mt, mb, mf, ma, fl, md, ck = c_double(), c_double(), c_double(), c_double(), c_double(), c_int32(), c_int64()
        _check(load_library().ttx_basis_core_grad_last(self._h, ctypes.byref(mt), ctypes.byref(mb), ctypes.byref(mf), ctypes.byref(ma), ctypes.byref(fl),
                                                       ctypes.byref(md), ctypes.byref(ck)))
        names = {v: k for k, v in EVAL_MODES.items()}
        return dict(ms_table=mt.value, ms_back=mb.value, ms_fwd=mf.value, ms_acc=ma.value, flops=fl.value, mode=names.get(md.value), chunk=ck.value)

    def cores_axpy(self, alpha, g):
        """U_i <- U_i + alpha_i G_i for every core in one launch (include/ttx.h: ttx_cores_axpy).  alpha: a scalar or d numbers;
        alpha_i = 0 leaves core i alone, whatever G_i holds.  g: what basis_core_grad returned (a list of blocks or a flat host
        array; a flat float64 tensor on the engine's device goes by pointer)."""
        L = load_library()
        al = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha, dtype=np.float64), (self.d,)))
        if type(g).__module__.split(".")[0] == "torch" and g.is_cuda:
            import torch
            total = int(self.core_offsets()[-1])
            if g.device.index != self.device or g.dtype != torch.float64 or not g.is_contiguous() or g.shape != (total,):
                raise ValueError(f"cores_axpy: a contiguous float64 tensor of {total} numbers on the engine's device expected")
            torch.cuda.current_stream(g.device).synchronize()
            _check(L.ttx_cores_axpy_dev(self._h, _dp(al), c_void_p(g.data_ptr())))
            return self
        if type(g).__module__.split(".")[0] == "torch":
            g = g.numpy()
        _check(L.ttx_cores_axpy(self._h, _dp(al), _dp(self._core_pack("cores_axpy", g))))
        return self

    # ---- the derivative along a direction in core space, vector operations, the solver (include/ttx.h: ttx_basis_jvp_batch) ----
    def _flat_dev(self, who, t):
        """a flat float64 tensor of core_offsets()[-1] numbers on the engine's device, or None for anything else"""
        if type(t).__module__.split(".")[0] != "torch" or not t.is_cuda:
            return None
        import torch
        total = int(self.core_offsets()[-1])
        if t.device.index != self.device or t.dtype != torch.float64 or not t.is_contiguous() or t.shape != (total,):
            raise ValueError(f"{who}: a contiguous float64 tensor of {total} numbers on the engine's device expected")
        torch.cuda.current_stream(t.device).synchronize()
        return t

    def _jvp(self, who, host, dev, head, t, cols, v, mode):
        md = _eval_mode(mode)
        val = self._dev_pair(who, t, cols)
        if val is not None:
            import torch
            if self._flat_dev(who, v) is None:
                raise ValueError(f"{who}: with points on the device, V must be a flat float64 tensor on the engine's device")
            dval = torch.empty_like(val)
            _check(dev(self._h, t.shape[0], c_void_p(t.data_ptr()), *head, c_void_p(v.data_ptr()), c_void_p(val.data_ptr()), c_void_p(dval.data_ptr()), md))
            return val, dval
        if type(t).__module__.split(".")[0] == "torch":
            t = t.cpu().numpy()
        if type(v).__module__.split(".")[0] == "torch":
            v = v.cpu().numpy()
        ta = np.ascontiguousarray(t, dtype=np.float64)
        if ta.ndim != 2 or ta.shape[1] != cols:
            raise ValueError(f"{who}: an array of shape (npts, {cols}) expected")
        flat = self._core_pack(who, v)
        val, dval = np.zeros(ta.shape[0]), np.zeros(ta.shape[0])
        _check(host(self._h, ta.shape[0], _dp(ta), *head, _dp(flat), _dp(val), _dp(dval), md))
        return val, dval

    def _basis_arr(self, who, basis):
        if isinstance(basis, (tuple, list)) and basis and isinstance(basis[0], str):
            basis = [basis] * self.d
        basis = list(basis)
        if len(basis) != self.d:
            raise ValueError(f"{who}: {self.d} basis entries expected (got {len(basis)})")
        pairs = [_basis_struct(e, self._n[k]) for k, e in enumerate(basis)]
        return (_Basis * self.d)(*[p[0] for p in pairs]), pairs          # pairs keeps the node arrays alive

    def basis_jvp(self, x, basis, V, mode="auto"):
        """(val, dval) at real points x (npts, d) (include/ttx.h: ttx_basis_jvp_batch): dval_p = sum_i f_(U_i <- V_i)(x_p), the
        derivative of f(x_p) along the direction V in core space -- J V, where basis_core_grad is J^T c.  val is basis_batch(x, basis)
        bit for bit in the mode that ran.  V: a list of blocks of the cores' shapes or a flat array, as cores_axpy takes g; with
        points on the device, a flat float64 tensor on that device (read in place).  basis_jvp_last() tells what ran."""
        L = load_library()
        arr, keep = self._basis_arr("basis_jvp", basis)
        return self._jvp("basis_jvp", L.ttx_basis_jvp_batch, L.ttx_basis_jvp_batch_dev, (arr,), x, self.d, V, mode)

    def basis_jvp_tab(self, phi, V, mode="auto"):
        """The same with the caller's own tables (include/ttx.h: ttx_basis_jvp_tab): phi (npts, sum n) in basis_tab's layout."""
        L = load_library()
        return self._jvp("basis_jvp_tab", L.ttx_basis_jvp_tab, L.ttx_basis_jvp_tab_dev, (), phi, int(self._n.sum()), V, mode)

    def basis_jvp_last(self):
        """dict(ms_table, ms_chain, flops, mode) of the last basis_jvp / basis_jvp_tab on this engine (include/ttx.h: ttx_basis_jvp_last)"""
        mt, mc, fl, md = c_double(), c_double(), c_double(), c_int32()
        _check(load_library().ttx_basis_jvp_last(self._h, ctypes.byref(mt), ctypes.byref(mc), ctypes.byref(fl), ctypes.byref(md)))
        names = {v: k for k, v in EVAL_MODES.items()}
        return dict(ms_table=mt.value, ms_chain=mc.value, flops=fl.value, mode=names.get(md.value))

    def cores_dot(self, a, b):
        """sum_e a_e * b_e of two packed core-space buffers in the fixed order of include/ttx.h (ttx_cores_dot): lists of blocks or
        flat host arrays, or two flat float64 tensors on the engine's device (by pointer).  A Python float."""
        L, out = load_library(), c_double()
        da, db = self._flat_dev("cores_dot", a), self._flat_dev("cores_dot", b)
        if (da is None) != (db is None):
            raise ValueError("cores_dot: both buffers on the host or both on the engine's device")
        if da is not None:
            _check(L.ttx_cores_dot_dev(self._h, c_void_p(a.data_ptr()), c_void_p(b.data_ptr()), ctypes.byref(out)))
            return out.value
        a, b = (t.numpy() if type(t).__module__.split(".")[0] == "torch" else t for t in (a, b))
        _check(L.ttx_cores_dot(self._h, _dp(self._core_pack("cores_dot", a)), _dp(self._core_pack("cores_dot", b)), ctypes.byref(out)))
        return out.value

    def cores_axpby(self, alpha, x, beta, y):
        """y <- (alpha * x) + (beta * y) on packed core-space buffers (include/ttx.h: ttx_cores_axpby_dev).  Two flat float64 tensors
        on the engine's device are updated in place on the device (y is returned); host arrays (lists of blocks or flat) give a new
        flat numpy array by the same three operations."""
        dx, dy = self._flat_dev("cores_axpby", x), self._flat_dev("cores_axpby", y)
        if (dx is None) != (dy is None):
            raise ValueError("cores_axpby: both buffers on the host or both on the engine's device")
        if dx is not None:
            _check(load_library().ttx_cores_axpby_dev(self._h, float(alpha), c_void_p(x.data_ptr()), float(beta), c_void_p(y.data_ptr())))
            return y
        x, y = (t.numpy() if type(t).__module__.split(".")[0] == "torch" else t for t in (x, y))
        return (float(alpha) * self._core_pack("cores_axpby", x)) + (float(beta) * self._core_pack("cores_axpby", y))

    def cores_get(self, out=None):
        """the engine's cores as one packed buffer, bit for bit (include/ttx.h: ttx_cores_get_dev): into the flat float64 device
        tensor out where one is given (and returned), otherwise a flat numpy array (ttx_cores_get)"""
        L = load_library()
        if out is not None:
            if self._flat_dev("cores_get", out) is None:
                raise ValueError("cores_get: out must be a flat float64 tensor on the engine's device")
            _check(L.ttx_cores_get_dev(self._h, c_void_p(out.data_ptr())))
            return out
        flat = np.zeros(int(self.core_offsets()[-1]))
        _check(L.ttx_cores_get(self._h, _dp(flat)))
        return flat

    def cores_set(self, g):
        """the engine's cores from a packed buffer of the present ranks, bit for bit (include/ttx.h: ttx_cores_set_dev): a flat float64
        tensor on the engine's device by pointer; a list of blocks or a flat host array through ttx_cores_set"""
        L = load_library()
        if self._flat_dev("cores_set", g) is not None:
            _check(L.ttx_cores_set_dev(self._h, c_void_p(g.data_ptr())))
            return self
        if type(g).__module__.split(".")[0] == "torch":
            g = g.numpy()
        _check(L.ttx_cores_set(self._h, _dp(self._core_pack("cores_set", g))))
        return self

    def _fit(self, who, host, dev, head, t, cols, y, w, opts):
        o = dict(FIT_DEFAULTS)
        unknown = set(opts) - set(o)
        if unknown:
            raise ValueError(f"{who}: unknown options {sorted(unknown)}")
        o.update(opts)
        fo = _FitOpts(int(o["max_iter"]), int(o["cg_max"]), int(o["max_reject"]), _eval_mode(o["mode"]), float(o["lambda0"]), float(o["lambda_down"]),
                      float(o["lambda_up"]), float(o["cg_tol"]), float(o["loss_tol"]))
        mi = max(fo.max_iter, 0)
        loss, lam, cg, acc, res = np.zeros(mi + 1), np.zeros(max(mi, 1)), np.zeros(max(mi, 1), dtype=np.int32), np.zeros(max(mi, 1), dtype=np.int32), _FitResult()
        tail = (ctypes.byref(fo), _dp(loss), _dp(lam), cg.ctypes.data_as(POINTER(c_int32)), acc.ctypes.data_as(POINTER(c_int32)), ctypes.byref(res))
        if self._dev_pair(who, t, cols) is not None:
            import torch
            for name, a in (("y", y), ("w", w)):
                if a is None and name == "w":
                    continue
                if type(a).__module__.split(".")[0] != "torch" or a.device != t.device or a.dtype != torch.float64 or not a.is_contiguous() or a.shape != (t.shape[0],):
                    raise ValueError(f"{who}: {name} must be a contiguous float64 tensor of shape (npts,) on the engine's device")
            torch.cuda.current_stream(t.device).synchronize()
            _check(dev(self._h, t.shape[0], c_void_p(t.data_ptr()), *head, c_void_p(y.data_ptr()), c_void_p(w.data_ptr()) if w is not None else None, *tail))
        else:
            t, y, w = (a.cpu().numpy() if type(a).__module__.split(".")[0] == "torch" else a for a in (t, y, w))
            ta, ya = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
            wa = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
            if ta.ndim != 2 or ta.shape[1] != cols or ya.shape != (ta.shape[0],) or (wa is not None and wa.shape != ya.shape):
                raise ValueError(f"{who}: an array of shape (npts, {cols}), npts targets and (or no) npts weights expected")
            _check(host(self._h, ta.shape[0], _dp(ta), *head, _dp(ya), _dp(wa) if wa is not None else None, *tail))
        return dict(loss=loss, lambda_=lam[:mi], cg_iters=cg[:mi], accepted=acc[:mi], iters=res.iters, stop=FIT_STOPS.get(res.stop, res.stop))

    def fit(self, x, basis, y, w=None, **opts):
        """Fit the resident train to data in place (include/ttx.h: ttx_basis_fit_batch): minimise 1/2 sum_p w_p (f(x_p) - y_p)^2 over
        all cores by a matrix-free Levenberg-Marquardt iteration on the device.  x (npts, d), basis as for basis_batch, y (npts,),
        w (npts,) or None for all ones; host arrays, or float64 tensors on the engine's device (by pointer).  opts: max_iter, cg_max,
        max_reject, mode, lambda0, lambda_down, lambda_up, cg_tol, loss_tol (FIT_DEFAULTS).  Returns the history: dict(loss
        (max_iter + 1), lambda_, cg_iters, accepted (max_iter each), iters, stop).  fit_last() reads the figures."""
        L = load_library()
        arr, keep = self._basis_arr("fit", basis)
        return self._fit("fit", L.ttx_basis_fit_batch, L.ttx_basis_fit_batch_dev, (arr,), x, self.d, y, w, opts)

    def fit_tab(self, phi, y, w=None, **opts):
        """The same with the caller's own tables (include/ttx.h: ttx_basis_fit_tab): phi (npts, sum n) in basis_tab's layout."""
        L = load_library()
        return self._fit("fit_tab", L.ttx_basis_fit_tab, L.ttx_basis_fit_tab_dev, (), phi, int(self._n.sum()), y, w, opts)

    def fit_last(self):
        """dict(ms_jvp, ms_core_grad, ms_value, ms_vector, n_jvp, n_core_grad, mode) of the last fit / fit_tab on this engine
        (include/ttx.h: ttx_basis_fit_last)"""
        mj, mc, mv, mx, nj, nc, md = c_double(), c_double(), c_double(), c_double(), c_int64(), c_int64(), c_int32()
        _check(load_library().ttx_basis_fit_last(self._h, ctypes.byref(mj), ctypes.byref(mc), ctypes.byref(mv), ctypes.byref(mx), ctypes.byref(nj),
                                                 ctypes.byref(nc), ctypes.byref(md)))
        names = {v: k for k, v in EVAL_MODES.items()}
        return dict(ms_jvp=mj.value, ms_core_grad=mc.value, ms_value=mv.value, ms_vector=mx.value, n_jvp=nj.value, n_core_grad=nc.value, mode=names.get(md.value))

    # ---- the normaliser of the squared density, maximum likelihood (include/ttx.h: ttx_sq_lognorm_grad) ---------
    def _tridiag_rows(self, who, md, mo):
        """(md rows, mo rows or None, what keeps them alive) as the arrays of d row pointers the C calls take"""
        if len(md) != self.d or (mo is not None and len(mo) != self.d):
            raise ValueError(f"{who}: {self.d} rows of md (and of mo, or mo=None) expected")
        keep = []
        dp, op = (POINTER(c_double) * self.d)(), (POINTER(c_double) * self.d)()
        for k in range(self.d):
            a = np.ascontiguousarray(md[k], dtype=np.float64)
            if a.shape != (self._n[k],):
                raise ValueError(f"{who}: md[{k}] must hold {self._n[k]} numbers")
            keep.append(a)
            dp[k] = _dp(a)
            if mo is not None and mo[k] is not None:
                b = np.ascontiguousarray(mo[k], dtype=np.float64)
                if b.shape != (max(self._n[k] - 1, 0),):
                    raise ValueError(f"{who}: mo[{k}] must hold {self._n[k] - 1} numbers")
                b = np.concatenate([b, np.zeros(1)])                    # never an empty array behind a non-null pointer
                keep.append(b)
                dp_b = _dp(b)
                op[k] = dp_b
        return dp, (op if mo is not None else None), keep

    def sq_lognorm_grad(self, md, mo=None, gvol=0.0, coef=1.0, out=None, accumulate=False, mode="auto"):
        """dict(z_mant, z_exp, logz, g) (include/ttx.h: ttx_sq_lognorm_grad): Z = <f, f>_M = z_mant 2^z_exp for the symmetric
        tridiagonal matrices M_k (md[k] the diagonal, mo[k] the off-diagonal or None for a diagonal matrix: mass_tridiag gives the
        hat functions' mass matrices), logz = log(Z + gvol) and g = out + (coef / (Z + gvol)) dZ/dU_k for every core.  out: None, a
        list of blocks or a flat host array (g is a list of blocks), or a flat float64 tensor on the engine's device (written in
        place, by pointer); accumulate=True adds onto it.  sq_lognorm_grad_last() tells what ran."""
        L, m, acc = load_library(), _eval_mode(mode), int(bool(accumulate))
        dp, op, keep = self._tridiag_rows("sq_lognorm_grad", md, mo)
        zm, ze, lz = c_double(), c_int64(), c_double()
        tail = (acc, m, ctypes.byref(zm), ctypes.byref(ze), ctypes.byref(lz))
        if out is not None and self._flat_dev("sq_lognorm_grad", out) is not None:
            _check(L.ttx_sq_lognorm_grad_dev(self._h, dp, op, float(gvol), float(coef), c_void_p(out.data_ptr()), *tail))
            g = out
        else:
            if out is None:
                if acc:
                    raise ValueError("sq_lognorm_grad: accumulate needs out")
                flat = np.zeros(int(self.core_offsets()[-1]))
            else:
                flat = self._core_pack("sq_lognorm_grad", out.numpy() if type(out).__module__.split(".")[0] == "torch" else out)
                flat = flat if flat.flags.writeable else flat.copy()
            _check(L.ttx_sq_lognorm_grad(self._h, dp, op, float(gvol), float(coef), _dp(flat), *tail))
            g = self._core_blocks(flat)
        return dict(z_mant=zm.value, z_exp=ze.value, logz=lz.value, g=g)

    def sq_lognorm_grad_last(self):
        """dict(ms_right, ms_left, ms_asm, flops, mode) of the last sq_lognorm_grad (also the one inside sq_nll) on this engine
        (include/ttx.h: ttx_sq_lognorm_grad_last)"""
        mr, ml, ma, fl, md = c_double(), c_double(), c_double(), c_double(), c_int32()
        _check(load_library().ttx_sq_lognorm_grad_last(self._h, ctypes.byref(mr), ctypes.byref(ml), ctypes.byref(ma), ctypes.byref(fl), ctypes.byref(md)))
        names = {v: k for k, v in EVAL_MODES.items()}
        return dict(ms_right=mr.value, ms_left=ml.value, ms_asm=ma.value, flops=fl.value, mode=names.get(md.value))

    # ---- moments and marginals of the squared density (include/ttx.h: ttx_sq_moments) ---------
    def _opt_rows(self, who, name, dg, of):
        """(diagonal rows, off-diagonal rows, keep) of an optional observable: a None entry of dg leaves the mode out"""
        if dg is None:
            return None, None, []
        if len(dg) != self.d or (of is not None and len(of) != self.d):
            raise ValueError(f"{who}: {self.d} rows of {name} (entries may be None) expected")
        keep = []
        dp, op = (POINTER(c_double) * self.d)(), (POINTER(c_double) * self.d)()
        for k in range(self.d):
            if dg[k] is None:
                continue
            a = np.ascontiguousarray(dg[k], dtype=np.float64)
            if a.shape != (self._n[k],):
                raise ValueError(f"{who}: {name}[{k}] must hold {self._n[k]} numbers")
            keep.append(a)
            dp[k] = _dp(a)
            if of is not None and of[k] is not None:
                b = np.ascontiguousarray(of[k], dtype=np.float64)
                if b.shape != (max(self._n[k] - 1, 0),):
                    raise ValueError(f"{who}: the off-diagonal of {name}[{k}] must hold {self._n[k] - 1} numbers")
                b = np.concatenate([b, np.zeros(1)])
                keep.append(b)
                op[k] = _dp(b)
        return dp, (op if of is not None else None), keep

    def sq_moments(self, md, mo=None, ad=None, ao=None, a2d=None, a2o=None, mode="auto", band=True):
        """dict(z_mant, z_exp, bd, bo, m1, c2) (include/ttx.h: ttx_sq_moments): ratios over Z = <f, f>_M = z_mant 2^z_exp of the squared
        train.  md, mo as for sq_lognorm_grad.  ad, ao: per mode the diagonal and off-diagonal of a symmetric tridiagonal observable A_k
        (moment_tridiag gives those of x and x^2), an entry None where the mode is not selected; m1[k] = <f, A_k f>_M / Z, c2[k][l] =
        <f, (A_k x A_l) f>_M / Z for selected k != l, c2[k][k] = <f, A2_k f>_M / Z with A2 from a2d, a2o (0.0 where not given); unselected
        entries are 0.0 (ad=None: m1 and c2 are None).  bd, bo: per mode the diagonal and off-diagonal of the reduced density matrix
        B_k / Z (band=False: None).  sq_moments_last() tells what ran."""
        L, m = load_library(), _eval_mode(mode)
        dp, op, keep = self._tridiag_rows("sq_moments", md, mo)
        adp, aop, keep_a = self._opt_rows("sq_moments", "ad", ad, ao)
        a2p, a2op, keep_b = self._opt_rows("sq_moments", "a2d", a2d, a2o)
        zm, ze = c_double(), c_int64()
        nsum = int(sum(self._n))
        bd = np.zeros(nsum) if band else None
        bo = np.zeros(nsum) if band else None
        m1 = np.zeros(self.d) if ad is not None else None
        c2 = np.zeros((self.d, self.d)) if ad is not None else None
        _check(L.ttx_sq_moments(self._h, dp, op, adp, aop, a2p, a2op, m, ctypes.byref(zm), ctypes.byref(ze),
                                _dp(bd) if band else None, _dp(bo) if band else None, _dp(m1) if ad is not None else None, _dp(c2) if ad is not None else None))
        cut = np.cumsum([int(v) for v in self._n])[:-1]
        return dict(z_mant=zm.value, z_exp=ze.value, bd=np.split(bd, cut) if band else None, bo=np.split(bo, cut) if band else None, m1=m1, c2=c2)

    def sq_moments_last(self):
        """dict(ms_chains, ms_band, ms_carry, ms_close, flops, steps, mode) of the last sq_moments on this engine (include/ttx.h:
        ttx_sq_moments_last); steps counts the carried chain steps"""
        a, b, c, e, fl, st, md = c_double(), c_double(), c_double(), c_double(), c_double(), c_int64(), c_int32()
        _check(load_library().ttx_sq_moments_last(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(e), ctypes.byref(fl), ctypes.byref(st), ctypes.byref(md)))
        names = {v: k for k, v in EVAL_MODES.items()}
        return dict(ms_chains=a.value, ms_band=b.value, ms_carry=c.value, ms_close=e.value, flops=fl.value, steps=int(st.value), mode=names.get(md.value))

    def _density_frame(self, who, nodes, gamma, cond):
        """(node rows, cond as floats with NaN for a drawn mode, the drawn modes, V) for the density over the hat functions on nodes"""
        rows, _ = self._node_rows(nodes, who)
        c = np.full(self.d, np.nan) if cond is None else np.array([np.nan if v is None else float(v) for v in cond], dtype=np.float64)
        if c.size != self.d:
            raise ValueError(f"{who}: {self.d} cond entries expected")
        if not (gamma >= 0.0 and np.isfinite(gamma)):
            raise ValueError(f"{who}: gamma is negative or not finite")
        drawn = [k for k in range(self.d) if np.isnan(c[k]) and rows[k].size > 1]
        vol = float(np.prod([rows[k][-1] - rows[k][0] for k in drawn]))
        return rows, c, drawn, vol

    @staticmethod
    def _alpha_logz(z_mant, z_exp, gvol):
        """alpha = z_mant / (z_mant + ldexp(gvol, -z_exp)), the weight of f^2 in q, and log(Z + gvol)"""
        den = z_mant + float(np.ldexp(gvol, int(max(-100000, min(100000, -z_exp)))))
        with np.errstate(invalid="ignore", divide="ignore"):
            return float(np.float64(z_mant) / np.float64(den)), float(z_exp * 0.6931471805599453 + np.log(np.float64(den)))

    def density_moments(self, nodes, gamma=0.0, cond=None, select=None, mode="auto"):
        """dict(mean, cov, alpha, logz, modes) of q = (f^2 + gamma) / (Z + gamma V) itself, f the piecewise-multilinear interpolant of
        the train of grid values on nodes (sample_sq_real's density): the exact mean and covariance of the drawn modes named in select
        (0-based; None: every drawn mode; held modes and modes of one node are left out), from one sq_moments call with the hat
        functions' moment matrices.  alpha = Z / (Z + gamma V) weighs the f^2 part, the uniform box's analytic moments take the rest:
        E_q[g] = alpha E_f2[g] + (1 - alpha) E_unif[g]; cov = E[x_k x_l] - E[x_k] E[x_l].  logz = log(Z + gamma V)."""
        rows, c, drawn, vol = self._density_frame("density_moments", nodes, gamma, cond)
        sel = drawn if select is None else [int(k) for k in select]
        if any(k not in drawn for k in sel) or len(set(sel)) != len(sel) or not sel:
            raise ValueError("density_moments: select names drawn modes, each once")
        sel = sorted(sel)
        md, mo = mass_tridiag(rows, list(c))
        ad, ao, a2d, a2o = [None] * self.d, [None] * self.d, [None] * self.d, [None] * self.d
        for k in sel:
            ad[k], ao[k] = moment_tridiag(rows[k], 1)
            a2d[k], a2o[k] = moment_tridiag(rows[k], 2)
        res = self.sq_moments(md, mo, ad, ao, a2d, a2o, mode=mode, band=False)
        alpha, logz = self._alpha_logz(res["z_mant"], res["z_exp"], gamma * vol)
        lo, hi = np.array([rows[k][0] for k in sel]), np.array([rows[k][-1] for k in sel])
        um, u2 = 0.5 * (lo + hi), (lo * lo + lo * hi + hi * hi) / 3.0
        ix = np.ix_(sel, sel)
        usec = np.outer(um, um)
        usec[np.diag_indices(len(sel))] = u2
        mean = alpha * res["m1"][sel] + (1.0 - alpha) * um
        sec = alpha * res["c2"][ix] + (1.0 - alpha) * usec
        return dict(mean=mean, cov=sec - np.outer(mean, mean), alpha=alpha, logz=logz, modes=sel)

    def sq_marginal_pdf(self, k, x, nodes, gamma=0.0, cond=None):
        """The one-mode marginal density of q (density_moments' q) in the drawn mode k (0-based) at the real points x: from the band of
        the reduced density matrix, alpha phi(x)^T (B_k / Z) phi(x) with the two hat functions phi of x's cell, plus the uniform part
        (1 - alpha) / (b_k - a_k).  0.0 outside the nodes' range."""
        rows, c, drawn, vol = self._density_frame("sq_marginal_pdf", nodes, gamma, cond)
        if k not in drawn:
            raise ValueError("sq_marginal_pdf: k names a drawn mode")
        md, mo = mass_tridiag(rows, list(c))
        res = self.sq_moments(md, mo, mode="exact", band=True)
        alpha, _ = self._alpha_logz(res["z_mant"], res["z_exp"], gamma * vol)
        t, bd, bo = rows[k], res["bd"][k], res["bo"][k]
        x = np.asarray(x, dtype=np.float64)
        cell = np.clip(np.searchsorted(t, x, side="right") - 1, 0, t.size - 2)
        p1 = (x - t[cell]) / (t[cell + 1] - t[cell])
        p0 = 1.0 - p1
        pdf = alpha * (bd[cell] * p0 * p0 + 2.0 * bo[cell] * p0 * p1 + bd[cell + 1] * p1 * p1) + (1.0 - alpha) / (t[-1] - t[0])
        return np.where((x >= t[0]) & (x <= t[-1]), pdf, 0.0)

    def sq_nll(self, x, basis, gamma, md, mo=None, gvol=0.0, w=None, mode="auto", out=None):
        """dict(nll, logz, val, g) (include/ttx.h: ttx_sq_nll_batch): the negative log-likelihood -sum_p w_p log(f(x_p)^2 + gamma) +
        (sum_p w_p) log(Z + gvol) of the points x (npts, d) under the squared density of the resident train, and its gradient with
        respect to the cores.  basis as for basis_batch, md and mo as for sq_lognorm_grad, w (npts,) >= 0 or None for all ones.  Host
        arrays give numpy out (g a list of blocks); float64 tensors on the engine's device go by pointer, g is then the flat device
        tensor out (allocated where None)."""
        L, m = load_library(), _eval_mode(mode)
        arr, keepb = self._basis_arr("sq_nll", basis)
        dp, op, keep = self._tridiag_rows("sq_nll", md, mo)
        nll, lz = c_double(), c_double()
        val = self._dev_pair("sq_nll", x, self.d)
        if val is not None:
            import torch
            if w is not None and (type(w).__module__.split(".")[0] != "torch" or w.device != x.device or w.dtype != torch.float64 or not w.is_contiguous() or w.shape != (x.shape[0],)):
                raise ValueError("sq_nll: w must be a contiguous float64 tensor of shape (npts,) on the engine's device")
            if out is None:
                out = torch.empty(int(self.core_offsets()[-1]), dtype=torch.float64, device=x.device)
            elif self._flat_dev("sq_nll", out) is None:
                raise ValueError("sq_nll: out must be a flat float64 tensor on the engine's device")
            torch.cuda.current_stream(x.device).synchronize()
            _check(L.ttx_sq_nll_batch_dev(self._h, x.shape[0], c_void_p(x.data_ptr()), arr, c_void_p(w.data_ptr()) if w is not None else None, float(gamma), dp, op,
                                          float(gvol), m, ctypes.byref(nll), ctypes.byref(lz), c_void_p(val.data_ptr()), c_void_p(out.data_ptr())))
            return dict(nll=nll.value, logz=lz.value, val=val, g=out)
        x, w = (a.cpu().numpy() if type(a).__module__.split(".")[0] == "torch" else a for a in (x, w))
        xa = np.ascontiguousarray(x, dtype=np.float64)
        wa = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
        if xa.ndim != 2 or xa.shape[1] != self.d or (wa is not None and wa.shape != (xa.shape[0],)):
            raise ValueError(f"sq_nll: an array of shape (npts, {self.d}) and (or no) npts weights expected")
        flat, hv = np.zeros(int(self.core_offsets()[-1])), np.zeros(xa.shape[0])
        _check(L.ttx_sq_nll_batch(self._h, xa.shape[0], _dp(xa), arr, _dp(wa), float(gamma), dp, op, float(gvol), m, ctypes.byref(nll), ctypes.byref(lz), _dp(hv), _dp(flat)))
        return dict(nll=nll.value, logz=lz.value, val=hv, g=self._core_blocks(flat))

    def fit_density(self, x, basis, gamma, md, mo=None, gvol=0.0, w=None, mode="auto", max_iter=20, history=5, c1=1e-4, shrink=0.5, max_back=20):
        """Fit the squared density of the resident train to weighted points by maximum likelihood, in place: L-BFGS with a fixed
        history and Armijo backtracking on sq_nll (tests/sq_norm_ref.py: lbfgs restates it operation by operation).  x (npts, d) and
        w are float64 tensors on the engine's device (host arrays are uploaded once); every core-space vector is a flat device
        tensor handled by cores_dot, cores_axpby, cores_get and cores_set, only scalars reach the host.  A rejected trial puts the
        cores back from the kept buffer.  Returns dict(nll (the accepted values, the start first), hist (every trial: (nll, accepted,
        the Armijo bound)), iters)."""
        import torch
        dev = torch.device("cuda", self.device)
        xt = x if (type(x).__module__.split(".")[0] == "torch" and x.is_cuda) else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64), device=dev)
        wt = w if (w is None or (type(w).__module__.split(".")[0] == "torch" and w.is_cuda)) else torch.as_tensor(np.ascontiguousarray(w, dtype=np.float64), device=dev)
        total = int(self.core_offsets()[-1])
        new = lambda: torch.empty(total, dtype=torch.float64, device=dev)          # noqa: E731

        def fun(out):
            return self.sq_nll(xt, basis, gamma, md, mo, gvol, wt, mode, out)["nll"]
        xc, g, q, p, xn, gn = new(), new(), new(), new(), new(), new()
        self.cores_get(xc)
        f = fun(g)
        S, Y, R = [], [], []
        hist, fs = [], [f]
        for _ in range(int(max_iter)):
            q.copy_(g)
            al = []
            for s_, y_, rho in zip(reversed(S), reversed(Y), reversed(R)):
                a = rho * self.cores_dot(s_, q)
                al.append(a)
                self.cores_axpby(-a, y_, 1.0, q)
            if S:
                gam = self.cores_dot(S[-1], Y[-1]) / self.cores_dot(Y[-1], Y[-1])
                self.cores_axpby(gam, q, 0.0, q)
            for (s_, y_, rho), a in zip(zip(S, Y, R), reversed(al)):
                be = rho * self.cores_dot(y_, q)
                self.cores_axpby(a - be, s_, 1.0, q)
            self.cores_axpby(-1.0, q, 0.0, p.copy_(q))
            slope = self.cores_dot(g, p)
            if not slope < 0.0:
                S, Y, R = [], [], []
                self.cores_axpby(-1.0, g, 0.0, p.copy_(g))
                slope = self.cores_dot(g, p)
                if not slope < 0.0:
                    break
            t = 1.0
            if not S:
                gnorm = float(np.sqrt(self.cores_dot(g, g)))
                t = 1.0 / gnorm if gnorm > 1.0 else 1.0
            done = False
            for _b in range(int(max_back)):
                self.cores_axpby(t, p, 1.0, xn.copy_(xc))
                self.cores_set(xn)
                fn = fun(gn)
                ok = bool(np.isfinite(fn) and fn <= f + c1 * t * slope)
                hist.append((fn, ok, f + c1 * t * slope))
                if ok:
                    done = True
                    break
                t = shrink * t
            if not done:
                self.cores_set(xc)
                break
            s_, y_ = new(), new()
            self.cores_axpby(-1.0, xc, 1.0, s_.copy_(xn))
            self.cores_axpby(-1.0, g, 1.0, y_.copy_(gn))
            sy = self.cores_dot(s_, y_)
            if sy > 0.0:
                S.append(s_); Y.append(y_); R.append(1.0 / sy)
                if len(S) > int(history):
                    S.pop(0); Y.pop(0); R.pop(0)
            xc, xn = xn, xc
            g, gn = gn, g
            f = fn
            fs.append(f)
        return dict(nll=fs, hist=hist, iters=len(fs) - 1)

    # ---- ranks grown from data: gradient enrichment (include/ttx.h: ttx_basis_enrich_batch) ---------------
    def enrich_ranks(self, add):
        """k_i of include/ttx.h (ttx_basis_enrich_batch, step 1) for add (a number or d - 1 numbers): what each bond can take"""
        r, n = self.ranks().astype(np.int64), self._n.astype(np.int64)
        a = np.broadcast_to(np.asarray(add, dtype=np.int64), (self.d - 1,))
        if (a < 0).any():
            raise ValueError(f"enrich: add must not be negative (got {a.tolist()})")
        return [int(max(0, min(a[i], r[i] * n[i] - r[i + 1], n[i + 1] * r[i + 2], 128 - r[i + 1]))) for i in range(self.d - 1)]

    def _enrich(self, who, host, dev, head, t, cols, c, add, seed, mode, want_sketch):
        md, nb = _eval_mode(mode), self.d - 1
        k = self.enrich_ranks(add)
        aa = np.ascontiguousarray(np.broadcast_to(np.asarray(add, dtype=np.int64), (nb,)), dtype=np.int32)
        r, n = self.ranks(), self._n
        shapes = [(int(r[i]), int(n[i]), k[i]) for i in range(nb)]
        total = int(sum(int(np.prod(s)) for s in shapes))
        added, gain, yn, h = np.zeros(nb, dtype=np.int32), np.zeros((nb, 128)), np.zeros(nb), c_void_p()
        mid = (_ip(aa), int(seed) & (2 ** 64 - 1), md, ctypes.byref(h), _ip(added), _dp(gain), _dp(yn))
        if self._dev_pair(who, t, cols) is not None:
            import torch
            if type(c).__module__.split(".")[0] != "torch" or c.device != t.device or c.dtype != torch.float64 or not c.is_contiguous() or c.shape != (t.shape[0],):
                raise ValueError(f"{who}: c must be a contiguous float64 tensor of shape (npts,) on the engine's device")
            y = torch.empty(max(total, 1), dtype=torch.float64, device=t.device) if want_sketch else None
            _check(dev(self._h, t.shape[0], c_void_p(t.data_ptr()), *head, c_void_p(c.data_ptr()), *mid, c_void_p(y.data_ptr()) if want_sketch else None))
            flat = y.cpu().numpy() if want_sketch else None
        else:
            t, c = (a.cpu().numpy() if type(a).__module__.split(".")[0] == "torch" else a for a in (t, c))
            ta, ca = np.ascontiguousarray(t, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
            if ta.ndim != 2 or ta.shape[1] != cols or ca.shape != (ta.shape[0],):
                raise ValueError(f"{who}: an array of shape (npts, {cols}) and npts weights expected")
            flat = np.zeros(max(total, 1)) if want_sketch else None
            _check(host(self._h, ta.shape[0], _dp(ta), *head, _dp(ca), *mid, _dp(flat) if want_sketch else None))
        ys = None
        if want_sketch:
            off = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in shapes])])
            ys = [flat[off[i]:off[i + 1]].reshape(shapes[i], order="F") for i in range(nb)]
        info = dict(added=[int(v) for v in added], k=k, gain=[gain[i, :k[i]].copy() for i in range(nb)], ynorm2=yn, y=ys)
        return TTCross._adopt(h, self.device), info

    def enrich(self, x, basis, c, add, seed=0, mode="auto", want_sketch=False):
        """(new train, info): the train with up to add new directions per bond taken from the two-site gradient of a loss at real
        points x (npts, d) (include/ttx.h: ttx_basis_enrich_batch).  c (npts,) is dLoss/df at the points, e.g. w (f - y) for least
        squares.  The new train is a new engine on the same device and the SAME function: the new columns of core i are orthonormal
        directions outside the range of its left unfolding, the new rows of core i + 1 are zeros, so the next fit() can move into
        them.  add: a number or d - 1 numbers; seed picks the sketch; mode "exact", "mfma" or "auto".  info: added (directions every
        bond took; 0 where its sketch was zero or not finite), k (what it could take), gain (per bond the k_i sizes of the new
        directions in the sketch, NaN for a sketch that is not finite), ynorm2 (the sketches' sums of squares) and y (want_sketch:
        the sketches Y_i, (r(i-1), n(i), k_i) each).  Host arrays, or float64 tensors on the engine's device by pointer."""
        L = load_library()
        arr, keep = self._basis_arr("enrich", basis)
        return self._enrich("enrich", L.ttx_basis_enrich_batch, L.ttx_basis_enrich_batch_dev, (arr,), x, self.d, c, add, seed, mode, want_sketch)

    def enrich_tab(self, phi, c, add, seed=0, mode="auto", want_sketch=False):
        """The same with the caller's own tables (include/ttx.h: ttx_basis_enrich_tab): phi (npts, sum n) in basis_tab's layout."""
        L = load_library()
        return self._enrich("enrich_tab", L.ttx_basis_enrich_tab, L.ttx_basis_enrich_tab_dev, (), phi, int(self._n.sum()), c, add, seed, mode, want_sketch)

    def enrich_last(self):
        """dict(ms_table, ms_back, ms_sketch, ms_qr, ms_asm, flops, mode, chunk) of the last enrich / enrich_tab on this engine
        (include/ttx.h: ttx_basis_enrich_last)"""
        ms = [c_double() for _ in range(6)]
        md, ck = c_int32(), c_int64()
        _check(load_library().ttx_basis_enrich_last(self._h, *[ctypes.byref(m) for m in ms], ctypes.byref(md), ctypes.byref(ck)))
        names = {v: k for k, v in EVAL_MODES.items()}
        return dict(ms_table=ms[0].value, ms_back=ms[1].value, ms_sketch=ms[2].value, ms_qr=ms[3].value, ms_asm=ms[4].value, flops=ms[5].value,
                    mode=names.get(md.value), chunk=ck.value)

    def fit_adaptive(self, x, basis, y, w=None, add=1, rmax=None, rounds=4, holdout=None, seed=0, mode="auto", **fit_opts):
        """(train, history): fit with ranks grown from the data.  Each round runs fit() (this engine is fitted in place in the first
        round, every later train is a new engine), forms c = w (f - y) with basis_batch and calls enrich() with add clipped so that
        no rank passes rmax (a number or d - 1 numbers; None: the engine's 128).  It stops after `rounds` fits, when nothing was
        added, when the fit reached its loss_tol, or when the loss on holdout = (x, y[, w]) rose -- and then returns the train of
        the round before.  No second solver: everything is fit, basis_batch and enrich.  history: per round dict(ranks, loss,
        holdout, added).  The train returned is this engine itself where no round added anything and a new engine otherwise; every
        engine in between is closed here, this one never:
            grown, hist = tt.fit_adaptive(x, basis, y, add=2, rmax=16)
            ...
            if grown is not tt:
                grown.close()"""
        nb = self.d - 1
        cap = np.broadcast_to(np.asarray(128 if rmax is None else rmax, dtype=np.int64), (nb,))
        want = np.broadcast_to(np.asarray(add, dtype=np.int64), (nb,))

        def held(tt):
            if holdout is None:
                return None
            res = tt.basis_batch(holdout[0], basis, mode) - holdout[1]
            sq = res * res if len(holdout) < 3 or holdout[2] is None else holdout[2] * (res * res)
            return 0.5 * float(sq.sum())
        cur, prev, prev_ho, hist = self, None, None, []

        def drop(tt):
            if tt is not None and tt is not self:
                tt.close()
        for rd in range(int(rounds)):
            h = cur.fit(x, basis, y, w, mode=mode, **fit_opts)
            ho = held(cur)
            hist.append(dict(ranks=[int(v) for v in cur.ranks()], loss=float(h["loss"][h["iters"]]), holdout=ho, added=None))
            if prev is not None and ho is not None and ho > prev_ho:
                drop(cur)
                return prev, hist
            if rd == int(rounds) - 1 or h["stop"] == "loss_tol":
                break
            res = cur.basis_batch(x, basis, mode) - y
            c = res if w is None else w * res
            room = np.maximum(cap - cur.ranks().astype(np.int64)[1:-1], 0)
            new, info = cur.enrich(x, basis, c, np.minimum(want, room), seed + rd, mode)
            hist[-1]["added"] = info["added"]
            if not any(info["added"]):
                new.close()
                break
            drop(prev)
            prev, prev_ho, cur = cur, ho, new
        if prev is not None and prev is not cur:
            drop(prev)
        return cur, hist

    def enrich_density(self, x, basis, gamma, add, w=None, seed=0, mode="auto", want_sketch=False):
        """enrich() with the data term of sq_nll as the loss: c_p = -2 w_p f_p / (f_p^2 + gamma) / sum_p w_p, f = basis_batch(x,
        basis).  The normaliser log(Z + gvol) also has a two-site gradient; that term is LEFT OUT here and stays open, so the
        directions are those along which the data term alone falls fastest."""
        f = self.basis_batch(x, basis, mode)
        wsum = float(f.shape[0]) if w is None else float(w.sum())
        c = (-2.0 / wsum) * (f / (f * f + gamma))
        if w is not None:
            c = w * c
        return self.enrich(x, basis, c, add, seed, mode, want_sketch)

    # ---- samples from the resident train (include/ttx.h: ttx_sample and its three siblings) --------------
    # the outputs of the index samplers and of the real samplers: name, a row of d per sample (else one number), dtype, always allocated
    _SAMPLE_IND = (("ind", True, "int32", True), ("logq", False, "float64", False), ("val", False, "float64", False))
    _SAMPLE_REAL = (("x", True, "float64", True), ("cell", True, "int32", False), ("logq", False, "float64", False), ("val", False, "float64", False))

    def _sample_call(self, who, host, dev, table, u_or_npts, seed, want, middle):
        """The one call path of sample, sample_sq, sample_real and sample_sq_real (who: the public method's name, the prefix of
        every message).  host, dev: the C entry for host arrays and its _dev form; table: the outputs (_SAMPLE_IND, _SAMPLE_REAL),
        those not always allocated only when named in want; middle(): the ctypes arguments between u and the outputs, formed
        after the check of want.  u_or_npts: a count (uniforms from numpy.random.default_rng(seed)), an array, or a torch tensor:
        one on the engine's device is passed by pointer and gives torch tensors there, one on the host goes through numpy."""
        names = tuple(t[0] for t in table)
        bad = set(want) - set(names)
        if bad:
            raise ValueError(f"{who}: unknown output {sorted(bad)}")
        mid = middle()
        on_torch = type(u_or_npts).__module__.split(".")[0] == "torch"
        if on_torch and u_or_npts.is_cuda:
            import torch
            u = u_or_npts
            if u.device.index != self.device:
                raise ValueError(f"{who}: the tensor lies on {u.device}, the engine on device {self.device}")
            if u.dtype != torch.float64 or not u.is_contiguous() or u.dim() != 2 or u.shape[1] != self.d:
                raise ValueError(f"{who}: a contiguous float64 tensor of shape (npts, {self.d}) expected")
            npts = u.shape[0]
            out = {name: torch.empty((npts, self.d) if row else npts, dtype=getattr(torch, dt), device=u.device) if always or name in want else None
                   for name, row, dt, always in table}
            torch.cuda.current_stream(u.device).synchronize()        # the engine runs on a stream of its own
            _check(dev(self._h, npts, c_void_p(u.data_ptr()), *mid, *[c_void_p(out[k].data_ptr()) if out[k] is not None else None for k in names]))
            return {k: out[k] for k in names if k in want}
        if on_torch:
            u_or_npts = u_or_npts.numpy()
        if np.ndim(u_or_npts) == 0:
            npts = int(u_or_npts)
            if npts < 0:
                raise ValueError(f"{who}: a negative count")
            u = np.random.default_rng(seed).random((npts, self.d))
        else:
            u = np.ascontiguousarray(u_or_npts, dtype=np.float64)
            if u.ndim != 2 or u.shape[1] != self.d:
                raise ValueError(f"{who}: an array of shape (npts, {self.d}) expected")
        npts = u.shape[0]
        out = {name: np.zeros((npts, self.d) if row else npts, dtype=dt) if always or name in want else None for name, row, dt, always in table}
        _check(host(self._h, npts, _dp(u), *mid, *[(_ip if dt == "int32" else _dp)(out[name]) for name, _, dt, _ in table]))
        if on_torch:
            import torch
            return {k: torch.from_numpy(out[k]) for k in names if k in want}
        return {k: out[k] for k in names if k in want}

    def _held_entries(self, v, who, what, dtype):
        """fixed (int32) or cond (float64) of a sampler: None, or d entries"""
        if v is None:
            return None
        a = np.ascontiguousarray(v, dtype=dtype).ravel()
        if a.size != self.d:
            raise ValueError(f"{who}: {self.d} {what} entries expected")
        return a

    def _draw_last(self, entry):
        """dict(ms_head, bytes_head, ms_draw, failed) from ttx_sample_last or ttx_sample_real_last"""
        a, b, c, n = c_double(), c_double(), c_double(), c_int64()
        _check(entry(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(n)))
        return dict(ms_head=a.value, bytes_head=b.value, ms_draw=c.value, failed=int(n.value))

    def _rows_last(self, entry):
        """dict(ms_head, ms_rows, ms_pick, flops, failed, mode) from ttx_sample_sq_last or ttx_sample_sq_real_last"""
        a, b, c, fl, n, md = c_double(), c_double(), c_double(), c_double(), c_int64(), c_int32()
        _check(entry(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(fl), ctypes.byref(n), ctypes.byref(md)))
        names = {v: k for k, v in EVAL_MODES.items()}
        return dict(ms_head=a.value, ms_rows=b.value, ms_pick=c.value, flops=fl.value, failed=int(n.value), mode=names.get(md.value))

    def sample(self, u_or_npts, w=None, fixed=None, seed=None, want=("ind", "logq", "val")):
        """Indices drawn from the train by sequential conditional sampling on the device (include/ttx.h: ttx_sample): for a train
        and weights without sign changes they follow |T(i)| w(i) / Z.  u_or_npts: uniforms of shape (npts, d), or a count, for
        which the uniforms come from numpy.random.default_rng(seed); w as for quad; fixed: d entries, 0 = drawn, f = held at the
        1-based index f.  Returns a dict with the entries named in want: ind (npts, d) int32, 1-based; logq, the log of the
        probability of the drawn index; val, the train's element there (tijk_batch(ind, "exact")).  A failed sample (all its
        conditional weights zero, a NaN or negative u) has an index row of zeros, logq NaN and val 0; sample_last() counts them.
        A contiguous float64 torch tensor on the engine's device is passed by pointer (ttx_sample_dev) and gives torch tensors
        on that device: ind can go straight into tijk_batch."""
        L = load_library()
        return self._sample_call("sample", L.ttx_sample, L.ttx_sample_dev, self._SAMPLE_IND, u_or_npts, seed, want,
                                 lambda: (_dp(self._weights(w, "sample")), _ip(self._held_entries(fixed, "sample", "fixed", np.int32))))

    def sample_last(self):
        """dict(ms_head, bytes_head, ms_draw, failed) of the last sample() on this engine (include/ttx.h: ttx_sample_last)"""
        return self._draw_last(load_library().ttx_sample_last)

    # ---- samples from the square of the resident train (include/ttx.h: ttx_sample_sq) ---------------------
    def sample_sq(self, u_or_npts, w=None, fixed=None, gamma=0.0, mode="auto", seed=None, want=("ind", "logq", "val")):
        """Indices drawn from the SQUARE of the train on the device, the squared-density sampler (include/ttx.h: ttx_sample_sq):
        for any train, signed or not, they follow (T(i)^2 + gamma) w(i) / (Z + gamma prod W_k).  The train is meant to
        approximate the square root of a density (of_trains with a sqrt-abs combiner builds it).  u_or_npts, fixed, seed, want and
        the returned dict are sample()'s; w as for quad, finite and non-negative; gamma >= 0 is the defensive term; mode is
        "exact", "mfma" or "auto" (only the rows of p depend on it; val is tijk_batch(ind, "exact") bit for bit either way).
        sample_sq_last() counts the failed samples.  A contiguous float64 torch tensor on the engine's device is passed by
        pointer (ttx_sample_sq_dev) and gives torch tensors on that device."""
        L = load_library()

        def middle():
            md = _eval_mode(mode)
            return _dp(self._weights(w, "sample_sq")), _ip(self._held_entries(fixed, "sample_sq", "fixed", np.int32)), float(gamma), md
        return self._sample_call("sample_sq", L.ttx_sample_sq, L.ttx_sample_sq_dev, self._SAMPLE_IND, u_or_npts, seed, want, middle)

    def sample_sq_last(self):
        """dict(ms_head, ms_rows, ms_pick, flops, failed, mode) of the last sample_sq() on this engine (include/ttx.h:
        ttx_sample_sq_last); mode is "exact" or "mfma" (None before the first call)"""
        return self._rows_last(load_library().ttx_sample_sq_last)

    # ---- real-valued samples from the interpolant of the train (include/ttx.h: ttx_sample_real) -----------
    def _node_rows(self, nodes, who):
        """nodes: one array for all modes or a list of d -> (the d arrays, the ctypes row pointers).  A ctypes array holds addresses,
        not numpy's owners, so the pointers carry the arrays along (rowp.rows): they live as long as the pointers do."""
        if not isinstance(nodes, (list, tuple)) or (len(nodes) and np.ndim(nodes[0]) == 0):
            nodes = [nodes] * self.d
        if len(nodes) != self.d:
            raise ValueError(f"{who}: {self.d} node rows expected (got {len(nodes)})")
        rows = [np.ascontiguousarray(t, dtype=np.float64) for t in nodes]
        for k, t in enumerate(rows):
            if t.ndim != 1 or t.size != int(self._n[k]):
                raise ValueError(f"{who}: {int(self._n[k])} nodes expected for mode {k + 1} (got shape {t.shape})")
        rowp = (POINTER(c_double) * self.d)(*[_dp(t) for t in rows])
        rowp.rows = rows
        return rows, rowp

    def sample_real(self, u_or_npts, nodes, cond=None, seed=None, want=("x", "cell", "logq", "val")):
        """Real points drawn from the piecewise-linear interpolant of the train of grid values, on the device (include/ttx.h:
        ttx_sample_real): for a train without sign changes they follow the interpolant f(x) / Z that basis_batch(x, ("linear",
        nodes)) evaluates, Z = quad(trapezoid_weights(nodes)).  u_or_npts: uniforms of shape (npts, d), or a count, for which the
        uniforms come from numpy.random.default_rng(seed); nodes: one array for all modes or a list of d; cond: d entries, NaN =
        drawn, a finite number = the mode is held at that coordinate.  Returns a dict with the entries named in want: x (npts, d);
        cell (npts, d) int32, the 1-based cell of a drawn mode and 0 for a held one; logq, the log of the proposal's density at x;
        val, the interpolant at x (basis_batch(x, linear, "exact")).  A failed sample (a conditional without mass, a NaN or
        negative u) has a row of NaN in x, cell 0, logq NaN and val 0; sample_real_last() counts them.  A contiguous float64 torch
        tensor on the engine's device is passed by pointer (ttx_sample_real_dev) and gives torch tensors on that device: x can go
        straight into basis_batch."""
        L = load_library()

        def middle():
            _, rowp = self._node_rows(nodes, "sample_real")       # rowp holds the node arrays until the call is over
            return rowp, _dp(self._held_entries(cond, "sample_real", "cond", np.float64))
        return self._sample_call("sample_real", L.ttx_sample_real, L.ttx_sample_real_dev, self._SAMPLE_REAL, u_or_npts, seed, want, middle)

    def sample_real_last(self):
        """dict(ms_head, bytes_head, ms_draw, failed) of the last sample_real() on this engine (include/ttx.h: ttx_sample_real_last)"""
        return self._draw_last(load_library().ttx_sample_real_last)

    # ---- real-valued samples from the square of the interpolant (include/ttx.h: ttx_sample_sq_real) -------
    def sample_sq_real(self, u_or_npts, nodes, cond=None, gamma=0.0, mode="auto", seed=None, want=("x", "cell", "logq", "val")):
        """Real points drawn from the SQUARE of the piecewise-multilinear interpolant g of the train of grid values, on the device
        (include/ttx.h: ttx_sample_sq_real): for any train, signed or not, they follow (g(x)^2 + gamma) / (Z + gamma V) over the
        drawn modes, Z the integral of g^2 and V the volume of the drawn modes' box.  The train is meant to approximate the square
        root of a density (of_trains with a sqrt-abs combiner builds it).  u_or_npts, nodes, cond, seed, want and the returned dict
        are sample_real()'s: val is basis_batch(x, ("linear", nodes), "exact"), and exp(logq) (Z + gamma V) = val^2 + gamma.
        gamma >= 0 is the defensive term; mode is "exact", "mfma" or "auto" (only the sums of the rows depend on it).
        sample_sq_real_last() counts the failed samples.  A contiguous float64 torch tensor on the engine's device is passed by
        pointer (ttx_sample_sq_real_dev) and gives torch tensors on that device."""
        L = load_library()

        def middle():
            md = _eval_mode(mode)
            _, rowp = self._node_rows(nodes, "sample_sq_real")
            return rowp, _dp(self._held_entries(cond, "sample_sq_real", "cond", np.float64)), float(gamma), md
        return self._sample_call("sample_sq_real", L.ttx_sample_sq_real, L.ttx_sample_sq_real_dev, self._SAMPLE_REAL, u_or_npts, seed, want, middle)

    def sample_sq_real_last(self):
        """dict(ms_head, ms_rows, ms_pick, flops, failed, mode) of the last sample_sq_real() on this engine (include/ttx.h:
        ttx_sample_sq_real_last); mode is "exact" or "mfma" (None before the first call)"""
        return self._rows_last(load_library().ttx_sample_sq_real_last)

    # ---- the way back: the forward Rosenblatt map of the squared interpolant (include/ttx.h: ttx_rosenblatt_sq_real) -------
    _ROSENBLATT = (("u", True, "float64", True), ("cell", True, "int32", False), ("logq", False, "float64", False), ("val", False, "float64", False))

    def rosenblatt_sq_real(self, x, nodes, cond=None, gamma=0.0, mode="auto", want=("u", "cell", "logq", "val")):
        """The forward Rosenblatt map of sample_sq_real()'s proposal at given points, on the device (include/ttx.h:
        ttx_rosenblatt_sq_real): x (npts, d) -> the uniforms u that sample_sq_real maps to x, with logq, the log of the proposal's
        density (g(x)^2 + gamma) / (Z + gamma V) at x, and val = g(x) = basis_batch(x, ("linear", nodes), "exact").  nodes, cond,
        gamma and mode are sample_sq_real()'s and must be the ones the points are judged under.  Returns a dict with the entries
        named in want: u (npts, d), 0.0 on a held mode; cell (npts, d) int32, the 1-based cell of x on a drawn mode and 0 on a held
        one; logq (-inf in a cell without mass); val.  At sample_sq_real()'s own x, in the same mode, logq and val repeat bit for
        bit.  A failed point (a drawn coordinate that is NaN or outside the nodes' range, a conditional without mass) has a row of
        NaN in u, cell 0, logq NaN and val 0; rosenblatt_sq_real_last() counts them.  A contiguous float64 torch tensor on the
        engine's device is passed by pointer (ttx_rosenblatt_sq_real_dev) and gives torch tensors on that device."""
        L = load_library()
        if type(x).__module__.split(".")[0] != "torch" and np.ndim(x) == 0:
            raise ValueError(f"rosenblatt_sq_real: an array of shape (npts, {self.d}) expected")

        def middle():
            md = _eval_mode(mode)
            _, rowp = self._node_rows(nodes, "rosenblatt_sq_real")
            return rowp, _dp(self._held_entries(cond, "rosenblatt_sq_real", "cond", np.float64)), float(gamma), md
        return self._sample_call("rosenblatt_sq_real", L.ttx_rosenblatt_sq_real, L.ttx_rosenblatt_sq_real_dev, self._ROSENBLATT, x, None, want, middle)

    def rosenblatt_sq_real_last(self):
        """dict(ms_head, ms_rows, ms_cdf, flops, failed, mode) of the last rosenblatt_sq_real() on this engine (include/ttx.h:
        ttx_rosenblatt_sq_real_last), kept apart from sample_sq_real_last(); mode is "exact" or "mfma" (None before the first call)"""
        r = self._rows_last(load_library().ttx_rosenblatt_sq_real_last)
        r["ms_cdf"] = r.pop("ms_pick")
        return {k: r[k] for k in ("ms_head", "ms_rows", "ms_cdf", "flops", "failed", "mode")}

    # ---- the largest elements of the resident train (include/ttx.h: ttx_topk) ----------------------------
    def topk(self, k, which="abs", fixed=None, mode="auto"):
        """The k largest elements of the train found by a beam search on the device, with an upper bound on everything the search
        discarded (include/ttx.h: ttx_topk).  which: "abs" (|T| descending), "max" (T descending) or "min" (T ascending) orders
        the rows; fixed: d entries, 0 = searched, f = held at the 1-based index f; mode: "exact", "mfma" or "auto" for the scores
        (topk_last() tells what ran).  Returns dict(ind (nfound, d) int32, 1-based; val, equal to tijk_batch(ind, "exact") bit for
        bit; bound: every element not returned has |T| <= bound up to rounding, NaN if a score was NaN; certified: "all" when
        bound <= min |val| (the rows are proven to be the top nfound by absolute size), "max" when bound <= max |val| (the largest
        is proven; with a single row the two coincide and "max" is reported), else None)."""
        if which not in TOPK_WHICH:
            raise ValueError(f"topk: which must be one of {sorted(TOPK_WHICH)} (got {which!r})")
        k, md = int(k), _eval_mode(mode)
        if not 1 <= k <= 4096:
            raise ValueError(f"topk: k = {k} (1 .. 4096 expected)")
        fx = None
        if fixed is not None:
            fx = np.ascontiguousarray(fixed, dtype=np.int32).ravel()
            if fx.size != self.d:
                raise ValueError(f"topk: {self.d} fixed entries expected")
        ind, val = np.zeros((k, self.d), dtype=np.int32), np.zeros(k)
        nf, bound = c_int32(), c_double()
        _check(load_library().ttx_topk(self._h, k, TOPK_WHICH[which], _ip(fx), md, ctypes.byref(nf), _ip(ind), _dp(val), ctypes.byref(bound)))
        ind, val, b = ind[:nf.value].copy(), val[:nf.value].copy(), bound.value
        av = np.abs(val)
        certified = None
        if nf.value > 1 and b <= av.min():
            certified = "all"
        elif nf.value and b <= av.max():
            certified = "max"
        return dict(ind=ind, val=val, bound=b, certified=certified)

    def topk_last(self):
        """dict(ms_gram, ms_score, ms_select, flops, mode) of the last topk() on this engine (include/ttx.h: ttx_topk_last); mode is
        "exact" or "mfma" (None before the first call)"""
        a, b, c, fl, md = c_double(), c_double(), c_double(), c_double(), c_int32()
        _check(load_library().ttx_topk_last(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(fl), ctypes.byref(md)))
        names = {v: k for k, v in EVAL_MODES.items()}
        return dict(ms_gram=a.value, ms_score=b.value, ms_select=c.value, flops=fl.value, mode=names.get(md.value))

    # ---- tt_lib utilities on the resident TT (lib/tt.f90: ort, svd, norm, dot_product, tijk) --------------
    def ort(self):
        _check(load_library().ttx_ort(self._h))
        return self

    def svd(self, tol, rmax=0):
        _check(load_library().ttx_svd(self._h, float(tol), int(rmax)))
        return self

    def norm(self, tol=None):
        v = c_double()
        _check(load_library().ttx_norm(self._h, -1.0 if tol is None else float(tol), ctypes.byref(v)))
        return v.value

    def lognorm(self, tol=None):
        """dtt_lognrm: log10 of the norm, finite where norm() over- or underflows"""
        v = c_double()
        _check(load_library().ttx_lognrm(self._h, -1.0 if tol is None else float(tol), ctypes.byref(v)))
        return v.value

    def dot(self, other):
        v = c_double()
        _check(load_library().ttx_dot(self._h, other._h, ctypes.byref(v)))
        return v.value

    def zquad(self, w):
        """ztt_quad (lib/dmrgg.f90:1418) batched: w complex array (nf, sum(n)) of rank-1 weights; returns nf complex values."""
        ww = np.ascontiguousarray(np.atleast_2d(np.asarray(w, dtype=np.complex128)))
        if ww.shape[1] != int(self._n.sum()):
            raise ValueError(f"zquad: weight rows of length sum(n) = {int(self._n.sum())} expected (got {ww.shape[1]})")
        out = np.zeros(2 * ww.shape[0])
        _check(load_library().ttx_zquad(self._h, ww.shape[0], _dp(ww.view(np.float64)), _dp(out)))
        return out.view(np.complex128).copy()

    def tijk(self, ind):
        a = np.ascontiguousarray(ind, dtype=np.int32)
        if a.size != self.d:
            raise ValueError(f"tijk: a multi-index of {self.d} entries expected")
        v = c_double()
        _check(load_library().ttx_ijk(self._h, _ip(a), ctypes.byref(v)))
        return v.value

    def tijk_batch(self, ind, mode="auto"):
        """dtt_ijk at a batch of multi-indices (include/ttx.h: ttx_ijk_batch): ind (npts, d), 1-based; mode "exact", "mfma" or
        "auto".  A host array gives a numpy array; a contiguous int32 torch tensor on the engine's device is passed by pointer
        (ttx_ijk_batch_dev: nothing crosses the host link) and gives a float64 torch tensor on that device.  Points with an
        entry outside 1..n(k) get -3.0."""
        L, m = load_library(), _eval_mode(mode)
        if type(ind).__module__.split(".")[0] == "torch":
            import torch
            if not ind.is_cuda:
                return torch.from_numpy(self.tijk_batch(ind.numpy(), mode))
            if ind.device.index != self.device:
                raise ValueError(f"tijk_batch: the tensor lies on {ind.device}, the engine on device {self.device}")
            if ind.dtype != torch.int32 or not ind.is_contiguous() or ind.dim() != 2 or ind.shape[1] != self.d:
                raise ValueError(f"tijk_batch: a contiguous int32 tensor of shape (npts, {self.d}) expected")
            out = torch.empty(ind.shape[0], dtype=torch.float64, device=ind.device)
            torch.cuda.current_stream(ind.device).synchronize()      # the engine runs on a stream of its own
            _check(L.ttx_ijk_batch_dev(self._h, ind.shape[0], c_void_p(ind.data_ptr()), c_void_p(out.data_ptr()), m))
            return out
        a = np.ascontiguousarray(ind, dtype=np.int32)
        if a.ndim != 2 or a.shape[1] != self.d:
            raise ValueError(f"tijk_batch: an array of shape (npts, {self.d}) expected")
        out = np.zeros(a.shape[0])
        _check(L.ttx_ijk_batch(self._h, a.shape[0], _ip(a), _dp(out), m))
        return out

    def value_batch(self, x, mode="auto"):
        """dtt_value (lib/tt.f90:702-728) at a batch of coordinate vectors x (npts, dd) in [0,1]^dd; the digits are formed on the
        device (value_indices restates them on the host).  A negative coordinate gives 0.0."""
        xa = np.ascontiguousarray(x, dtype=np.float64)
        if xa.ndim != 2 or xa.shape[1] < 1:
            raise ValueError("value_batch: an array of shape (npts, dd) expected")
        out = np.zeros(xa.shape[0])
        _check(load_library().ttx_value_batch(self._h, xa.shape[0], xa.shape[1], _dp(xa), _dp(out), _eval_mode(mode)))
        return out

    @property
    def eval_last_mode(self):
        """'exact' or 'mfma': what the last tijk_batch / value_batch ran with (None before the first)."""
        v = load_library().ttx_eval_last_mode(self._h)
        return {0: "exact", 1: "mfma"}.get(v)

    def accchk(self, nlot):
        """dtt_accchk (lib/dmrgg.f90:1081): dict(einf, efro, ainf, afro, pivot) from nlot random samples."""
        e1, e2, a1, a2 = c_double(), c_double(), c_double(), c_double()
        pv = np.zeros(self.d, dtype=np.int32)
        _check(load_library().ttx_accchk(self._h, nlot, ctypes.byref(e1), ctypes.byref(e2), ctypes.byref(a1), ctypes.byref(a2), _ip(pv)))
        return dict(einf=e1.value, efro=e2.value, ainf=a1.value, afro=a2.value, pivot=pv)

    def kernel_stats(self):
        n = (c_int64 * 6)()
        ms = (c_double * 6)()
        by = (c_double * 6)()
        _check(load_library().ttx_kernel_stats(self._h, n, ms, by))
        return {K_NAMES[i]: dict(launches=int(n[i]), ms=float(ms[i]), bytes=float(by[i])) for i in range(6)}


def dtt_dmrgg(n, fun_id, par, accuracy=None, maxrank=None, mybonds=None, pivoting=3, quad=None, tru=None, aux=None,
              nproc=1, device=0, verbose=False):
    """Mirror of `call dtt_dmrgg(arg, fun, par, accuracy, maxrank, mybonds, pivoting, neval, quad, tru)`;
    returns the engine (holding the finalised cores, ranks, neval and per-sweep records)."""
    if maxrank is None:
        raise TTXError("dtt_dmrgg: maxrank is required by the device engine (it sizes HBM storage)")
    return TTCross(n, fun_id, par, maxrank, pivoting=pivoting, accuracy=accuracy, quad=quad, tru=tru, aux=aux,
                   nproc=nproc, mybonds=mybonds, device=device, verbose=verbose).run()


# ---- kernel-level entry points (parity tests) --------------------------------------------------------
def k_residual_argmax(a, F, x, device=0):
    a = np.ascontiguousarray(a, dtype=np.float64)
    F = np.asfortranarray(F, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    m, r = F.shape
    b = np.zeros(m)
    im = c_int32()
    bm = c_double()
    _check(load_library().ttx_k_residual_argmax(device, m, r, _dp(a), F.ctypes.data_as(POINTER(c_double)), _dp(x), _dp(b),
                                                ctypes.byref(im), ctypes.byref(bm)))
    return b, im.value, bm.value


def k_residual_bench(m, r, iters=20, device=0):
    """(avg kernel ms, algorithmic bytes) of the K2 residual + arg-max kernel on an m x r factor in HBM."""
    ms, by = c_double(), c_double()
    _check(load_library().ttx_k_residual_bench(device, m, r, iters, ctypes.byref(ms), ctypes.byref(by)))
    return ms.value, by.value


def k_eval(fun_id, n, par, ind, aux=None, device=0, arith=None):
    n = np.ascontiguousarray(n, dtype=np.int32)
    par = np.ascontiguousarray(par, dtype=np.float64)
    ind = np.ascontiguousarray(ind, dtype=np.int32)
    aux_ = None if aux is None else np.ascontiguousarray(aux, dtype=np.float64)
    out = np.zeros(ind.shape[0])
    L = load_library()
    L.ttx_k_eval_arith.argtypes = L.ttx_k_eval.argtypes + [c_int32]
    _check(L.ttx_k_eval_arith(device, fun_id, n.size, _ip(n), _dp(par), par.size, _dp(aux_), 0 if aux_ is None else aux_.size,
                              ind.shape[0], _ip(ind), _dp(out), 1 if arith in (1, "fast") else 0))
    return out


def k_lottery(npnt, m, n, zcol, zrow, rngpos=0, device=0):
    zc = np.ascontiguousarray(zcol, dtype=np.int32)
    zr = np.ascontiguousarray(zrow, dtype=np.int32)
    pts = np.zeros(2 * npnt, dtype=np.int32)
    _check(load_library().ttx_k_lottery(device, npnt, m, n, zc.size, _ip(zc), _ip(zr), rngpos, _ip(pts)))
    return pts.reshape(2, npnt)


def k_fast_block(fun_id, d, n, par, p, left, right, cap, mode="scratch", aux=None, points=None, device=0):
    """The table evaluators of TTX_ARITH=fast (csrc/ttx_fast.h) on one hand-made bond p (include/ttx.h: ttx_k_fast_block).
    left [rL][p-1] / right [rR][d-p-1]: 1-based mode indices of the pivots; mode 'scratch' or 'chain'; cap: decay-table rows in
    LDS for the lottery route.  Returns near, dv [2][d+1][RM], piv [2][8][RM], the block [rL][n][n][rR] by the three routes
    (lottery, col, row), nfar_col [rR][n], nfar_row [n][rL] and point [npts]."""
    par = np.ascontiguousarray(par, dtype=np.float64)
    aux_ = None if aux is None else np.ascontiguousarray(aux, dtype=np.float64)
    rL, rR = len(left), len(right)
    left = np.ascontiguousarray(left, dtype=np.int32).reshape(rL, p - 1)
    right = np.ascontiguousarray(right, dtype=np.int32).reshape(rR, d - p - 1)
    pts = np.zeros((0, d), dtype=np.int32) if points is None else np.ascontiguousarray(points, dtype=np.int32).reshape(-1, d)
    RM, FD = max(rL, rR), d + 1
    near, dv, piv = np.zeros((2, FD, RM)), np.zeros((2, FD, RM)), np.zeros((2, 8, RM))
    lot, col, row = (np.zeros((rL, n, n, rR)) for _ in range(3))
    nfar, pnt = np.zeros(n * rR + rL * n), np.zeros(max(pts.shape[0], 1))
    L = load_library()
    L.ttx_k_fast_block.argtypes = ([c_int32] * 4 + [POINTER(c_double), c_int32, POINTER(c_double), c_int32, c_int32, c_int32, POINTER(c_int32), c_int32,
                                   POINTER(c_int32), c_int32, c_int32, c_int64, POINTER(c_int32)] + [POINTER(c_double)] * 8)
    _check(L.ttx_k_fast_block(device, fun_id, d, n, _dp(par), par.size, _dp(aux_), 0 if aux_ is None else aux_.size, p, rL, _ip(left), rR, _ip(right),
                              cap, {"scratch": 0, "chain": 1}[mode], pts.shape[0], _ip(pts), _dp(near), _dp(dv), _dp(piv), _dp(lot), _dp(col),
                              _dp(row), _dp(nfar), _dp(pnt)))
    return dict(near=near, dv=dv, piv=piv, lottery=lot, col=col, row=row, nfar_col=nfar[:n * rR].reshape(rR, n),
                nfar_row=nfar[n * rR:].reshape(n, rL), point=pnt[:pts.shape[0]])


def k_exp(x, device=0):
    """The integrands' exp (ttx_exp.h) evaluated on the device."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    _check(load_library().ttx_k_exp(device, x.size, _dp(x), _dp(out)))
    return out


def exp_host(x):
    """The same source instantiated on the host (needs no GPU): pins ttx_exp.h against the run-time libm."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    _check(load_library().ttx_exp_host(x.size, _dp(x), _dp(out)))
    return out


def k_latency_probe(device=0):
    """dict of unit latencies in ns measured on one wave (include/ttx.h: ttx_k_latency_probe)."""
    L = load_library()
    L.ttx_k_latency_probe.argtypes = [c_int32, POINTER(c_double)]
    o = (c_double * 5)()
    _check(L.ttx_k_latency_probe(device, o))
    return dict(fp64_mul_ns=o[0], fp64_mul_add_ns=o[1], l2_roundtrip_ns=o[2], lds_read_ns=o[3], fp64_div_ns=o[4])
