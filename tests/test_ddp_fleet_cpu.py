"""The batched DDP pass (mppi_compute_feedback_gains_batch, csrc/ddp_fleet.hip): what can be checked without a GPU.
  1. the three symbols are exported, declared in the header and known to the binding; the ABI version stays;
  2. null or short arguments and n < 1 are refused with MPPI_ERR_INVALID;
  3. csrc/tanhf_scalar.hpp -- the text the kernel runs on the device -- compiled for the host returns libm's tanhf bit for bit over
     the stride tests/test_host_math.py uses (every 5th of the 2^32 bit patterns; NaN payloads aside)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from autorally_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mppi_compute_feedback_gains_batch", "mppi_debug_ddp_info", "mppi_debug_device_tanhf")


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
    assert hasattr(capi, "compute_feedback_gains_batch") and hasattr(capi.Solver, "debug_ddp_info")


def test_null_and_short_arguments_are_refused(L):
    fp = C.POINTER(C.c_float)
    st = np.zeros((2, 7), np.float32)
    stp = st.ctypes.data_as(fp)
    hs = (C.c_void_p * 2)()  # two null handles
    f = L.mppi_compute_feedback_gains_batch
    assert f(None, stp, None, None, 2) == capi.ERR_INVALID
    assert f(hs, None, None, None, 2) == capi.ERR_INVALID
    assert f(hs, stp, None, None, 0) == capi.ERR_INVALID
    assert f(hs, stp, None, None, -3) == capi.ERR_INVALID
    assert f(hs, stp, None, None, 2) == capi.ERR_INVALID      # a null handle in the set
    assert f(hs, stp, None, None, 1) == capi.ERR_INVALID
    on = C.c_int(-7)
    assert L.mppi_debug_ddp_info(None, C.byref(on)) == capi.ERR_INVALID
    assert L.mppi_debug_ddp_info(None, None) == capi.ERR_INVALID
    assert on.value == -7  # nothing written
    x = np.zeros(4, np.float32)
    y = np.full(4, 9.0, np.float32)
    xp, yp = x.ctypes.data_as(fp), y.ctypes.data_as(fp)
    assert L.mppi_debug_device_tanhf(0, None, yp, 4) == capi.ERR_INVALID
    assert L.mppi_debug_device_tanhf(0, xp, None, 4) == capi.ERR_INVALID
    assert L.mppi_debug_device_tanhf(0, xp, yp, 0) == capi.ERR_INVALID
    assert L.mppi_debug_device_tanhf(-1, xp, yp, 4) == capi.ERR_INVALID
    assert np.all(y == 9.0)
    if L.mppi_device_count() == 0:
        assert L.mppi_debug_device_tanhf(0, xp, yp, 4) == capi.ERR_NO_DEVICE  # no CPU fallback


def test_scalar_tanhf_text_returns_libm_bits_on_the_host(tmp_path):
    exe = str(tmp_path / "tanhf_scalar_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fopenmp",
                           os.path.join(ROOT, "tools", "host", "tanhf_scalar_check.cpp"), "-o", exe])
    r = subprocess.run([exe, "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 differ" in r.stdout, r.stdout
    n = int(r.stdout.split(":")[1].split("inputs")[0])
    assert n >= (1 << 32) // 5
