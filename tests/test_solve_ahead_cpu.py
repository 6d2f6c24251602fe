"""Solve-ahead entry points (mppi_arm, mppi_arm_batch, mppi_disarm, mppi_is_armed): argument checks and exports, no GPU needed."""
import ctypes as C

import pytest

from autorally_amd import capi
from autorally_amd import synthetic as S


@pytest.fixture(scope="module")
def L():
    from autorally_amd import build as B
    B.build()
    return capi.lib()


def test_solve_ahead_symbols_exported(L):
    for name in ("mppi_arm", "mppi_arm_batch", "mppi_disarm", "mppi_is_armed"):
        assert hasattr(L, name)
        assert name in capi.SYMBOLS


def test_null_and_out_of_range_arguments(L):
    assert L.mppi_arm(None, 0.01) == capi.ERR_INVALID
    assert L.mppi_disarm(None) == capi.ERR_INVALID
    assert L.mppi_is_armed(None) == 0
    assert L.mppi_arm_batch(None, 2, 0.01) == capi.ERR_INVALID
    hs = (C.c_void_p * 2)(None, None)
    assert L.mppi_arm_batch(hs, 0, 0.01) == capi.ERR_INVALID   # empty batch
    assert L.mppi_arm_batch(hs, -1, 0.01) == capi.ERR_INVALID
    assert L.mppi_arm_batch(hs, 2, 0.01) == capi.ERR_INVALID   # NULL handles


def test_handle_arguments_without_or_with_a_device(L):
    """Without a device no handle can exist (mppi_create: MPPI_ERR_NO_DEVICE), so every call sees NULL: MPPI_ERR_INVALID.  With
    one, max_wait_s outside (0, 0.1] and a handle twice in one batch are MPPI_ERR_INVALID before anything is enqueued."""
    cfg = S.make_config(128, 50)
    c = capi.make_config_struct(cfg)
    h = C.c_void_p()
    if L.mppi_device_count() == 0:
        assert L.mppi_create(C.byref(c), C.byref(h)) == capi.ERR_NO_DEVICE
        assert L.mppi_arm(h, 0.01) == capi.ERR_INVALID
        assert L.mppi_is_armed(h) == 0
        return
    sol = capi.Solver(cfg)
    for bad in (0.0, -1.0, 0.1000001, 1.0, float("nan")):
        assert L.mppi_arm(sol.h, bad) == capi.ERR_INVALID
        hs = (C.c_void_p * 1)(sol.h)
        assert L.mppi_arm_batch(hs, 1, bad) == capi.ERR_INVALID
    hs = (C.c_void_p * 2)(sol.h, sol.h)
    assert L.mppi_arm_batch(hs, 2, 0.01) == capi.ERR_INVALID  # duplicate handle
    assert not sol.is_armed()
    sol.close()
