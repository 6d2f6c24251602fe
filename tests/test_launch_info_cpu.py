"""mppi_debug_launch_info (how many instances the rollout launch of a handle's latest solve served, and whether it was gated):
export and argument checks, no GPU needed."""
import ctypes as C

import pytest

from autorally_amd import capi
from autorally_amd import synthetic as S


@pytest.fixture(scope="module")
def L():
    from autorally_amd import build as B
    B.build()
    return capi.lib()


def test_launch_info_is_exported_and_the_abi_version_stays(L):
    assert hasattr(L, "mppi_debug_launch_info")
    assert "mppi_debug_launch_info" in capi.SYMBOLS
    assert L.mppi_abi_version() == 5  # an additive debug hook
    assert hasattr(capi.Solver, "debug_launch_info")


def test_null_arguments_are_refused(L):
    n, g = C.c_int(-7), C.c_int(-7)
    assert L.mppi_debug_launch_info(None, C.byref(n), C.byref(g)) == capi.ERR_INVALID
    assert L.mppi_debug_launch_info(None, None, None) == capi.ERR_INVALID
    assert (n.value, g.value) == (-7, -7)  # nothing written
    if L.mppi_device_count() == 0:
        return  # no handle can exist without a device (mppi_create: MPPI_ERR_NO_DEVICE)
    sol = capi.Solver(S.make_config(128, 20))
    try:
        assert L.mppi_debug_launch_info(sol.h, None, C.byref(g)) == capi.ERR_INVALID
        assert L.mppi_debug_launch_info(sol.h, C.byref(n), None) == capi.ERR_INVALID
        assert (n.value, g.value) == (-7, -7)
        assert sol.debug_launch_info() == (0, 0)  # no solve yet
    finally:
        sol.close()
