"""The fused closing stages of a fleet's tick (mppi_nominal_and_gains_batch, csrc/nominal_gains_fleet.hip): what can be checked
without a GPU.
  1. both symbols are exported, declared in the header and known to the binding; the ABI version stays;
  2. malformed calls are refused with MPPI_ERR_INVALID and write nothing;
  3. conditions on the inputs of tests/test_nominal_gains_fleet_gpu.py, not measurements: every problem of
     tests/nominal_gains_cases.py factorises in oracle.ddp_feedback_gains when it tracks the oracle's own nominal trajectory, at
     least four instances clamp at a limit, and the heading leaves 0 in every instance (none of them is built to keep it there);
  4. finishTickFleetOnDevice of host/mppi_controller_hip.hpp compiles and links for the network controller."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from autorally_amd import capi
from tests import nominal_cases as NC
from tests import nominal_gains_cases as NG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "autorally_amd")
NAMES = ("mppi_nominal_and_gains_batch", "mppi_debug_nominal_and_gains_info")


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
    assert hasattr(capi, "nominal_and_gains_batch") and hasattr(capi.Solver, "debug_nominal_and_gains_info")
    with pytest.raises(capi.MppiError) as e:
        capi.nominal_and_gains_batch([], [])   # an empty fleet: the library's answer to n < 1, not an IndexError
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
    f = L.mppi_nominal_and_gains_batch
    assert f(None, stp, xsp, usp, 2) == capi.ERR_INVALID
    assert f(hs, None, xsp, usp, 2) == capi.ERR_INVALID
    assert f(hs, stp, None, usp, 2) == capi.ERR_INVALID
    assert f(hs, stp, xsp, None, 2) == capi.ERR_INVALID
    assert f(hs, stp, xsp, usp, 0) == capi.ERR_INVALID
    assert f(hs, stp, xsp, usp, -3) == capi.ERR_INVALID
    assert f(hs, stp, xsp, usp, 2) == capi.ERR_INVALID   # a null handle in the set
    assert f(hs, stp, xsp, usp, 1) == capi.ERR_INVALID
    # (a NULL output pointer is checked behind the handle beside it: with null handles the refusal is the handle's; a NULL output
    # pointer and a handle twice among REAL handles are tests/test_nominal_gains_fleet_gpu.py's)
    assert f(hs, stp, none2, usp, 2) == capi.ERR_INVALID
    assert f(hs, stp, xsp, none2, 2) == capi.ERR_INVALID
    assert all(np.all(a == 9.0) for a in xs + us)         # nothing written
    fused = C.c_int(-7)
    assert L.mppi_debug_nominal_and_gains_info(None, C.byref(fused)) == capi.ERR_INVALID
    assert L.mppi_debug_nominal_and_gains_info(None, None) == capi.ERR_INVALID
    assert fused.value == -7


def test_the_fleets_problems_factorise_clamp_and_turn():
    """Conditions on the inputs.  It reads the oracle only, so unlike the other new tests it does not depend on the library's new
    entry: it guards the problem list."""
    probs, orc = NG.problems(), NG.oracle_results()   # oracle_results raises where a factorisation fails
    assert len(probs) == len(NC.FLEET) == len(orc)
    clamped = 0
    for i, (p, (xs, us, ref)) in enumerate(zip(probs, orc)):
        cfg = p["cfg"]
        lo, hi = np.asarray(cfg["u_lo"], np.float32), np.asarray(cfg["u_hi"], np.float32)
        at_limit = bool(np.any(p["U"] < lo) or np.any(p["U"] > hi))
        turn = float(np.max(np.abs(xs[:, 2])))
        print("NOMGAINS inputs %s: factorises, total cost %.4g; clamps at a limit %s; largest |heading| %.3f; zeros in Q %d, Qf %s" % (
            NC.tag(i), ref["total_cost"], at_limit, turn, int(np.sum(p["Q"] == 0.0)), "on" if np.any(p["Qf"] != 0) else "off"))
        assert all(np.all(np.isfinite(ref[k])) for k in ("feedback", "feedforward", "x", "u")) and np.isfinite(ref["total_cost"]), NC.tag(i)
        assert np.any(xs[:, 2] != 0.0), NC.tag(i) + ": the heading leaves 0"
        assert np.any(p["Q"] == 0.0), NC.tag(i)
        clamped += int(at_limit)
    assert clamped >= 4, clamped
    assert any(np.any(p["Qf"] != 0) for p in probs) and any(np.all(p["Qf"] == 0) for p in probs)


def test_the_host_layer_has_the_fused_finish(tmp_path):
    """finishTickFleetOnDevice beside finishControlFleetOnDevice and computeFeedbackGainsFleet: instantiated for the network
    controller and linked against the library."""
    src, exe = str(tmp_path / "finish_tick_host.cpp"), str(tmp_path / "finish_tick_host")
    with open(src, "w") as f:
        f.write('#include "mppi_controller_hip.hpp"\n'
                "using C = mppi_host::MPPIController;\n"
                "void (*finish)(C *const *, int) = &C::finishTickFleetOnDevice;\n"
                "int main() { C::finishTickFleetOnDevice(nullptr, 0); return finish == nullptr; }\n")
    from autorally_amd import build as B
    B.build()
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-DMPPI_NPZ_ZLIB", "-I" + os.path.join(PKG, "host"), src, "-o", exe,
                           "-L" + PKG, "-lmppi_hip", "-Wl,-rpath," + PKG, "-lz", "-lpthread"])
    assert subprocess.run([exe], timeout=60).returncode == 0   # an empty fleet: nothing is called, no device is needed
