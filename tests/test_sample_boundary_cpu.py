"""ttx_sample / ttx_sample_dev / ttx_sample_last without a GPU: the symbols exist and the refusals that precede any device call
(include/ttx.h) answer TTX_EINVAL."""
import ctypes

import numpy as np

from ttcross_amd import engine as E

EINVAL, ESTATE = 1, 4


def test_the_three_symbols_exist():
    L = E.load_library()
    for name in ("ttx_sample", "ttx_sample_dev", "ttx_sample_last"):
        assert hasattr(L, name)


def test_refusals_before_any_device_call():
    L = E.load_library()
    u, ind = np.zeros((2, 3)), np.zeros((2, 3), np.int32)
    nul_d, nul_i = ctypes.POINTER(ctypes.c_double)(), ctypes.POINTER(ctypes.c_int32)()
    assert L.ttx_sample(None, -1, E._dp(u), nul_d, nul_i, E._ip(ind), nul_d, nul_d) == EINVAL
    assert L.ttx_sample(None, 2, nul_d, nul_d, nul_i, E._ip(ind), nul_d, nul_d) == EINVAL
    assert L.ttx_sample(None, 2, E._dp(u), nul_d, nul_i, nul_i, nul_d, nul_d) == EINVAL
    assert L.ttx_sample_dev(None, -1, None, nul_d, nul_i, None, None, None) == EINVAL
    assert L.ttx_sample_dev(None, 2, None, nul_d, nul_i, None, None, None) == EINVAL
    assert b"ttx_sample_dev" in L.ttx_last_error()
    assert L.ttx_sample_last(None, None, None, None, None) == EINVAL
    # sound arguments and no engine: the state error, still without a device
    assert L.ttx_sample(None, 2, E._dp(u), nul_d, nul_i, E._ip(ind), nul_d, nul_d) == ESTATE
    assert L.ttx_sample(None, 0, nul_d, nul_d, nul_i, nul_i, nul_d, nul_d) == ESTATE
