"""mppi_closed_loop_ticks_batch without a device: the refusals that need no handle, and the host's check behind a device run
(mppi_debug_closed_loop_check) over synthetic logs.  The GPU cases are tests/test_closed_loop_fleet_gpu.py."""
import ctypes as C

import numpy as np
import pytest

from autorally_amd import capi


@pytest.fixture(scope="module")
def L():
    from autorally_amd import build as B
    B.build()
    lib = capi.lib()
    assert hasattr(lib, "mppi_closed_loop_ticks_batch"), "the library has no closed-loop entry"
    return lib


def test_the_binding_declares_the_new_symbols(L):
    for name in ("mppi_closed_loop_ticks_batch", "mppi_debug_closed_loop_info", "mppi_debug_closed_loop_check"):
        assert name in capi.SYMBOLS and name in capi.UNVERSIONED_SYMBOLS
        assert hasattr(L, name), name
    assert L.mppi_abi_version() == 5


def test_arguments_are_refused_before_a_handle_is_touched(L):
    fp = C.POINTER(C.c_float)
    st = np.zeros((2, 7), np.float32)
    stp = st.ctypes.data_as(fp)
    none = C.POINTER(fp)()
    nulls = (C.c_void_p * 2)(None, None)
    call = L.mppi_closed_loop_ticks_batch
    assert call(None, stp, 2, 1, 1, none, none, none) == capi.ERR_INVALID      # no handle array
    assert call(nulls, None, 2, 1, 1, none, none, none) == capi.ERR_INVALID    # no states
    assert call(nulls, stp, 0, 1, 1, none, none, none) == capi.ERR_INVALID     # n < 1
    assert call(nulls, stp, 2, 0, 1, none, none, none) == capi.ERR_INVALID     # n_ticks < 1
    assert call(nulls, stp, 2, 1, 1, none, none, none) == capi.ERR_INVALID     # a NULL handle in the set
    assert np.all(st == 0.0)
    on, ticks = C.c_int(7), C.c_int(7)
    assert L.mppi_debug_closed_loop_info(None, C.byref(on), C.byref(ticks)) == capi.ERR_INVALID
    assert (on.value, ticks.value) == (7, 7)
    with pytest.raises(capi.MppiError) as e:
        capi.closed_loop_ticks_batch([], [], 3, 1)
    assert e.value.status == capi.ERR_INVALID


def _logs(n_ticks, stride):
    etas = np.linspace(1.0, 40.0, n_ticks).astype(np.float32)   # eta == 1 is a good tick: the best rollout alone has weight 1
    controls = np.random.RandomState(3).uniform(-0.99, 0.65, (n_ticks, stride, 2)).astype(np.float32)
    return etas, controls


def test_the_check_passes_good_logs(L):
    for stride in (1, 3):
        etas, controls = _logs(9, stride)
        assert capi.debug_closed_loop_check(etas, controls, stride) == -1


@pytest.mark.parametrize("bad_eta", [0.5, 0.0, -3.0, np.nan, np.inf, -np.inf])
def test_the_check_names_the_first_tick_with_a_bad_eta(L, bad_eta):
    etas, controls = _logs(9, 2)
    etas[6] = bad_eta
    etas[4] = bad_eta
    assert capi.debug_closed_loop_check(etas, controls, 2) == 4


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize("stride,where", [(1, (5, 0, 1)), (3, (2, 2, 0)), (3, (0, 0, 0)), (2, (8, 1, 1))])
def test_the_check_names_the_first_tick_with_a_control_that_is_not_finite(L, bad, stride, where):
    etas, controls = _logs(9, stride)
    controls[where] = bad
    controls[8, stride - 1, 1] = bad   # a later one as well: the FIRST is reported
    assert capi.debug_closed_loop_check(etas, controls, stride) == where[0]


def test_a_bad_eta_and_a_bad_control_report_the_earlier_tick(L):
    etas, controls = _logs(9, 1)
    etas[7] = np.float32(np.nan)
    controls[3, 0, 0] = np.float32(np.nan)
    assert capi.debug_closed_loop_check(etas, controls, 1) == 3
    etas[1] = np.float32(0.25)
    assert capi.debug_closed_loop_check(etas, controls, 1) == 1


def test_the_check_refuses_malformed_arguments(L):
    fp = C.POINTER(C.c_float)
    etas, controls = _logs(4, 1)
    ep, cp = etas.ctypes.data_as(fp), controls.ctypes.data_as(fp)
    bad = C.c_int(-2)
    call = L.mppi_debug_closed_loop_check
    assert call(None, cp, 4, 1, C.byref(bad)) == capi.ERR_INVALID
    assert call(ep, None, 4, 1, C.byref(bad)) == capi.ERR_INVALID
    assert call(ep, cp, 0, 1, C.byref(bad)) == capi.ERR_INVALID
    assert call(ep, cp, 4, 0, C.byref(bad)) == capi.ERR_INVALID
    assert call(ep, cp, 4, 1, None) == capi.ERR_INVALID
    assert bad.value == -2
    with pytest.raises(capi.MppiError):
        capi.debug_closed_loop_check(etas, controls, 2)   # the controls are not [n_ticks][stride][2]
