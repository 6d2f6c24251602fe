"""The batched nominal replay (mppi_nominal_traj_batch, csrc/nominal_fleet.hip): what can be checked without a GPU.
  1. both symbols are exported, declared in the header and known to the binding; the ABI version stays;
  2. malformed calls are refused with MPPI_ERR_INVALID and write nothing;
  3. a condition on the inputs of tests/test_nominal_fleet_gpu.py, not a measurement: for every problem of tests/nominal_cases.py
     the oracle's fp32 nominal_traj stays within 1e-5 of the float64 replay (the problems are not chaotic: the GPU test's 1e-4 bound
     has an order of magnitude of room), and clamping fires at both limits in at least three instances;
  4. finishControlFleetOnDevice of host/mppi_controller_hip.hpp compiles and links for the network controller."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from autorally_amd import capi
from oracle import oracle as O
from tests import nominal_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "autorally_amd")
NAMES = ("mppi_nominal_traj_batch", "mppi_debug_nominal_info")


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
    assert hasattr(capi, "nominal_traj_batch") and hasattr(capi.Solver, "debug_nominal_info")
    with pytest.raises(capi.MppiError) as e:
        capi.nominal_traj_batch([], [])   # an empty fleet: the library's answer to n < 1, not an IndexError
    assert e.value.status == capi.ERR_INVALID


def test_malformed_calls_are_refused_and_write_nothing(L):
    fp = C.POINTER(C.c_float)
    st = np.zeros((2, 7), np.float32)
    stp = st.ctypes.data_as(fp)
    xs = [np.full((5, 7), 9.0, np.float32) for _ in range(2)]
    us = [np.full((5, 2), 9.0, np.float32) for _ in range(2)]
    xsp = (fp * 2)(*[a.ctypes.data_as(fp) for a in xs])
    usp = (fp * 2)(*[a.ctypes.data_as(fp) for a in us])
    none2 = (fp * 2)()       # two null output pointers
    hs = (C.c_void_p * 2)()  # two null handles
    f = L.mppi_nominal_traj_batch
    assert f(None, stp, xsp, usp, 2) == capi.ERR_INVALID
    assert f(hs, None, xsp, usp, 2) == capi.ERR_INVALID
    assert f(hs, stp, None, usp, 2) == capi.ERR_INVALID
    assert f(hs, stp, xsp, None, 2) == capi.ERR_INVALID
    assert f(hs, stp, xsp, usp, 0) == capi.ERR_INVALID
    assert f(hs, stp, xsp, usp, -3) == capi.ERR_INVALID
    assert f(hs, stp, xsp, usp, 2) == capi.ERR_INVALID   # a null handle in the set
    assert f(hs, stp, xsp, usp, 1) == capi.ERR_INVALID
    # (with real handles: a handle twice and a NULL output pointer in the set are tests/test_nominal_fleet_gpu.py's)
    assert f(hs, stp, none2, usp, 2) == capi.ERR_INVALID
    assert f(hs, stp, xsp, none2, 2) == capi.ERR_INVALID
    assert all(np.all(a == 9.0) for a in xs + us)         # nothing written
    on = C.c_int(-7)
    assert L.mppi_debug_nominal_info(None, C.byref(on)) == capi.ERR_INVALID
    assert L.mppi_debug_nominal_info(None, None) == capi.ERR_INVALID
    assert on.value == -7


def test_the_fleets_problems_are_well_conditioned_and_clamp():
    """A condition on the inputs: the fp32 replay of EVERY problem is within 1e-5 of its float64 replay, so that a device replay
    that differs from the host's by an ulp of sin / cos in a few steps cannot come near the GPU test's 1e-4.  It reads the oracle and
    Ref64 only, so unlike the other new tests it does not depend on the library's new entry: it guards the problem list."""
    both = 0
    for i, p in enumerate(NC.problems()):
        cfg = p["cfg"]
        xs, us = O.Oracle(cfg).nominal_traj(p["x0"], p["U"])
        x64, u64 = NC.replay64(cfg, p["x0"], p["U"])
        err = float(np.max(np.abs(xs.astype(np.float64) - x64)))
        lo, hi = np.asarray(cfg["u_lo"], np.float32), np.asarray(cfg["u_hi"], np.float32)
        at_lo, at_hi = bool(np.any(p["U"] < lo)), bool(np.any(p["U"] > hi))
        print("NOMFLEET inputs %s: oracle fp32 against float64 %.2e (bound 1e-5); clamped at the lower limit %s, at the upper %s" % (
            NC.tag(i), err, at_lo, at_hi))
        assert np.all(np.isfinite(xs))
        assert err <= 1e-5, NC.tag(i)
        np.testing.assert_array_equal(us.astype(np.float64), u64)   # the clamp is exact
        np.testing.assert_array_equal(xs[0].view(np.uint32), p["x0"].view(np.uint32))
        both += int(at_lo and at_hi)
    assert both >= 3, both


def test_the_host_layer_has_the_device_replay(tmp_path):
    """finishControlFleetOnDevice beside finishControlFleet: instantiated for the network controller and linked against the library."""
    src, exe = str(tmp_path / "nominal_host.cpp"), str(tmp_path / "nominal_host")
    with open(src, "w") as f:
        f.write('#include "mppi_controller_hip.hpp"\n'
                "using C = mppi_host::MPPIController;\n"
                "void (*finish)(C *const *, int) = &C::finishControlFleetOnDevice;\n"
                "int main() { C::finishControlFleetOnDevice(nullptr, 0); return finish == nullptr; }\n")
    from autorally_amd import build as B
    B.build()
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DMPPI_NPZ_ZLIB", "-I" + os.path.join(PKG, "host"), src, "-o", exe,
                           "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG, "-lz", "-lpthread"])
    assert subprocess.run([exe], timeout=60).returncode == 0   # an empty fleet: nothing is called, no device is needed
