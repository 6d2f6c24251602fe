"""The batched trace (mppi_trace_rollouts_batch, csrc/rollout_trace.hip, csrc/abi_trace.hip): what can be checked without a GPU.
  1. both symbols are exported, declared in the header and known to the binding; the ABI version stays;
  2. malformed calls are refused with MPPI_ERR_INVALID before any device call and write nothing.  Without a device no handle can
     exist (mppi_create: MPPI_ERR_NO_DEVICE), so the cases that need a real handle -- a handle twice, a negative count, a count
     above K, an index outside [0, K), a missing output pointer -- are tests/test_trace_fleet_gpu.py's; with a device they are
     checked here as well."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import synthetic as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mppi_trace_rollouts_batch", "mppi_debug_trace_info")
FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int)


@pytest.fixture(scope="module")
def L():
    from autorally_amd import build as B
    B.build()
    return capi.lib()


def test_symbols_are_exported_and_the_abi_version_stays(L):
    hdr = open(os.path.join(ROOT, "include", "mppi_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, hdr), "%s is not declared in include/mppi_hip.h" % name
    assert L.mppi_abi_version() == 5  # compatible additions
    assert hasattr(capi, "trace_rollouts_batch") and hasattr(capi.Solver, "debug_trace_info")
    with pytest.raises(capi.MppiError) as e:
        capi.trace_rollouts_batch([], [])   # an empty fleet: the library's answer to n_handles < 1, not an IndexError
    assert e.value.status == capi.ERR_INVALID


def _buffers(n, c, T):
    """n handles' output buffers for c rollouts each, filled with a sentinel, and their pointer arrays"""
    bufs = dict(ks=[np.full(c, -9, np.int32) for _ in range(n)], states=[np.full((c, T, 7), 9.0, np.float32) for _ in range(n)],
                controls=[np.full((c, T, 2), 9.0, np.float32) for _ in range(n)], step_costs=[np.full((c, T), 9.0, np.float32) for _ in range(n)],
                costs=[np.full(c, 9.0, np.float32) for _ in range(n)], first_crash=[np.full(c, -9, np.int32) for _ in range(n)])
    ptrs = {k: ((IP if v[0].dtype == np.int32 else FP) * n)(*[a.ctypes.data_as(IP if a.dtype == np.int32 else FP) for a in v])
            for k, v in bufs.items()}
    return bufs, ptrs


def _untouched(bufs):
    return all(np.all(a == (-9 if a.dtype == np.int32 else 9.0)) for v in bufs.values() for a in v)


def test_malformed_calls_are_refused_and_write_nothing(L):
    bufs, p = _buffers(2, 3, 5)
    out = (p["ks"], p["states"], p["controls"], p["step_costs"], p["costs"], p["first_crash"])
    counts = (C.c_int * 2)(3, 3)
    hs = (C.c_void_p * 2)()  # two null handles
    f = L.mppi_trace_rollouts_batch
    assert f(None, 2, counts, None, *out) == capi.ERR_INVALID
    assert f(hs, 2, None, None, *out) == capi.ERR_INVALID
    assert f(hs, 0, counts, None, *out) == capi.ERR_INVALID
    assert f(hs, -3, counts, None, *out) == capi.ERR_INVALID
    assert f(hs, 2, counts, None, *out) == capi.ERR_INVALID   # a null handle in the set
    assert f(hs, 1, counts, None, *out) == capi.ERR_INVALID
    assert f(hs, 2, counts, None, None, None, None, None, None, None) == capi.ERR_INVALID
    assert _untouched(bufs)
    on = C.c_int(-7)
    assert L.mppi_debug_trace_info(None, C.byref(on)) == capi.ERR_INVALID
    assert L.mppi_debug_trace_info(None, None) == capi.ERR_INVALID
    assert on.value == -7


def test_handle_arguments_without_or_with_a_device(L):
    """With a device: every refusal that needs a real handle comes before the readiness checks (the handles have no solve yet: a
    call that got past the argument checks would answer MPPI_ERR_STATE) and writes nothing."""
    cfg = S.make_config(128, 5)
    if L.mppi_device_count() == 0:
        h = C.c_void_p()
        c = capi.make_config_struct(cfg)
        assert L.mppi_create(C.byref(c), C.byref(h)) == capi.ERR_NO_DEVICE
        return
    sols = [capi.Solver(cfg), capi.Solver(cfg)]
    try:
        bufs, p = _buffers(2, 3, 5)
        out = (p["ks"], p["states"], p["controls"], p["step_costs"], p["costs"], p["first_crash"])
        f = L.mppi_trace_rollouts_batch
        hs = (C.c_void_p * 2)(sols[0].h, sols[1].h)
        twice = (C.c_void_p * 2)(sols[0].h, sols[0].h)
        ok = (C.c_int * 2)(3, 3)
        good, bad_hi, bad_lo = np.array([0, 127, 127], np.int32), np.array([0, 128, 1], np.int32), np.array([0, -1, 1], np.int32)
        assert f(twice, 2, ok, None, *out) == capi.ERR_INVALID
        assert f(hs, 2, (C.c_int * 2)(3, -1), None, *out) == capi.ERR_INVALID
        big = _buffers(2, 129, 5)[1]
        assert f(hs, 2, (C.c_int * 2)(3, 129), None, big["ks"], big["states"], None, None, None, None) == capi.ERR_INVALID  # above K, chosen by weight
        for bad in (bad_hi, bad_lo):
            ks = (IP * 2)(good.ctypes.data_as(IP), bad.ctypes.data_as(IP))
            assert f(hs, 2, ok, ks, *out) == capi.ERR_INVALID
        hole = (FP * 2)(bufs["states"][0].ctypes.data_as(FP), None)
        assert f(hs, 2, ok, None, p["ks"], hole, None, None, None, None) == capi.ERR_INVALID   # a missing output pointer
        assert f(hs, 2, (C.c_int * 2)(3, 0), None, p["ks"], hole, None, None, None, None) == capi.ERR_STATE  # ... of a handle that traces nothing: no argument error
        assert f(hs, 2, ok, None, *out) == capi.ERR_STATE      # well-formed: no solve yet
        assert _untouched(bufs)
    finally:
        for s in sols:
            s.close()
