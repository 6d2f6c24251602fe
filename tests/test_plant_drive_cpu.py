"""A plant of its own (mppi_set_plant_model, mppi_plant_drive_batch, mppi_closed_loop_sim_batch): what can be checked without a GPU.
  1. the symbols are exported, declared in the header and known to the binding; the ABI version stays;
  2. malformed calls are refused with MPPI_ERR_INVALID and write nothing (mppi_set_plant_model's refusals and its set / clear need a
     handle, which needs a device: they are tests/test_plant_drive_gpu.py's);
  3. the HOST TEXT of the drive law (mppi_debug_plant_drive_host: plant_drive_host of csrc/abi_host.hip, no handle) against a float64
     restatement of the law written with numpy on tests/ref64.Ref64.state_deriv (tests/plant_drive_cases.drive64), fed the same fp32
     sequences and gains: within 1e-5 for EVERY problem and call the GPU tests use -- the project's condition on inputs
     (tests/test_nominal_fleet_cpu.py), so that the GPU test's 1e-4 has an order of magnitude of room;
  4. the law's branches are hit, proven on the inputs: the clamp, a feedback correction above 1e-3, the NaN fallback (one NaN gain),
     the j == 0 rule (control_seq[hi] = inf is never read at substeps = 1).
Each case prints what it measured."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from autorally_amd import capi
from oracle import oracle as O
from tests import plant_drive_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mppi_set_plant_model", "mppi_debug_plant_model_info", "mppi_plant_drive_batch", "mppi_debug_plant_drive_info",
         "mppi_debug_plant_drive_host", "mppi_closed_loop_sim_batch")
HOST_BOUND = 1e-5


@pytest.fixture(scope="module")
def L():
    from autorally_amd import build as B
    B.build()
    lib = capi.lib()
    assert hasattr(lib, "mppi_plant_drive_batch"), "the library has no plant drive"
    return lib


def test_symbols_are_exported_and_the_abi_version_stays(L):
    hdr = open(os.path.join(ROOT, "include", "mppi_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        assert hasattr(L, name), name
        assert name in capi.SYMBOLS and name in capi.UNVERSIONED_SYMBOLS
        assert re.search(r"\b%s\s*\(" % name, hdr), "%s is not declared in include/mppi_hip.h" % name
    assert L.mppi_abi_version() == 5  # compatible additions
    for f in ("plant_drive_batch", "closed_loop_sim_batch", "debug_plant_drive_host"):
        assert hasattr(capi, f), f
    for f in ("set_plant_model", "debug_plant_model_info", "debug_plant_drive_info"):
        assert hasattr(capi.Solver, f), f
    for call in (lambda: capi.plant_drive_batch([], [], [], 1, 1), lambda: capi.closed_loop_sim_batch([], [], 1, 1, 1)):
        with pytest.raises(capi.MppiError) as e:
            call()   # an empty fleet: the library's answer to n < 1
        assert e.value.status == capi.ERR_INVALID


def test_malformed_calls_are_refused_and_write_nothing(L):
    fp = C.POINTER(C.c_float)
    st = np.zeros((2, 7), np.float32)
    out = np.full((2, 7), 9.0, np.float32)
    stp, outp = st.ctypes.data_as(fp), out.ctypes.data_as(fp)
    xs = [np.full((5, 7), 9.0, np.float32) for _ in range(2)]
    us = [np.full((5, 2), 9.0, np.float32) for _ in range(2)]
    ap = [np.full((4, 2), 9.0, np.float32) for _ in range(2)]
    xsp, usp, app = ((fp * 2)(*[a.ctypes.data_as(fp) for a in arrs]) for arrs in (xs, us, ap))
    none2 = (fp * 2)()
    hs = (C.c_void_p * 2)()   # two null handles
    f = L.mppi_plant_drive_batch
    assert f(None, stp, xsp, usp, 2, 1, 1, 0, outp, app) == capi.ERR_INVALID
    assert f(hs, None, xsp, usp, 2, 1, 1, 0, outp, app) == capi.ERR_INVALID
    assert f(hs, stp, None, usp, 2, 1, 1, 0, outp, app) == capi.ERR_INVALID
    assert f(hs, stp, xsp, None, 2, 1, 1, 0, outp, app) == capi.ERR_INVALID
    assert f(hs, stp, xsp, usp, 0, 1, 1, 0, outp, app) == capi.ERR_INVALID
    assert f(hs, stp, xsp, usp, 2, 1, 1, 0, None, app) == capi.ERR_INVALID
    assert f(hs, stp, xsp, usp, 2, 1, 1, 0, outp, app) == capi.ERR_INVALID     # a null handle in the set
    assert f(hs, stp, none2, usp, 2, 1, 1, 0, outp, app) == capi.ERR_INVALID
    g = L.mppi_closed_loop_sim_batch
    nofpp = C.POINTER(fp)()
    assert g(None, stp, 2, 1, 1, 1, 0, nofpp, app, nofpp) == capi.ERR_INVALID
    assert g(hs, None, 2, 1, 1, 1, 0, nofpp, app, nofpp) == capi.ERR_INVALID
    assert g(hs, stp, 0, 1, 1, 1, 0, nofpp, app, nofpp) == capi.ERR_INVALID
    assert g(hs, stp, 2, 0, 1, 1, 0, nofpp, app, nofpp) == capi.ERR_INVALID    # n_ticks < 1
    assert g(hs, stp, 2, 1, 1, 0, 0, nofpp, app, nofpp) == capi.ERR_INVALID    # substeps < 1
    assert g(hs, stp, 2, 1, 1, 17, 0, nofpp, app, nofpp) == capi.ERR_INVALID   # substeps > 16
    assert g(hs, stp, 2, 1, 1, 1, 0, nofpp, app, nofpp) == capi.ERR_INVALID    # a null handle in the set
    assert np.all(out == 9.0) and np.all(st == 0.0) and all(np.all(a == 9.0) for a in xs + us + ap)
    n = C.c_int(-7)
    layers = (C.c_int * 3)(6, 8, 4)
    th = np.zeros(92, np.float32)
    assert L.mppi_set_plant_model(None, layers, 3, th.ctypes.data_as(fp), 92, 0) == capi.ERR_INVALID
    assert L.mppi_debug_plant_model_info(None, C.byref(n)) == capi.ERR_INVALID
    assert L.mppi_debug_plant_drive_info(None, C.byref(n)) == capi.ERR_INVALID
    assert n.value == -7


def test_the_host_text_refuses_malformed_arguments(L):
    p = PC.problems()[1]
    xs, us, K = _inputs(1)
    args = dict(layers=p["plant"]["layers"], theta=p["plant"]["theta"], negate_yaw_der=False, dt=0.02, u_lo=p["cfg"]["u_lo"],
                u_hi=p["cfg"]["u_hi"], x=p["x_plant"], state_seq=xs, control_seq=us, feedback=K, periods=2, substeps=3)
    capi.debug_plant_drive_host(**args)
    for change in (dict(periods=0), dict(periods=PC.T), dict(substeps=0), dict(substeps=17), dict(dt=0.0), dict(layers=[5, 24, 4]),
                   dict(layers=[6, 24, 3]), dict(layers=[6, 300, 4]), dict(theta=p["plant"]["theta"][:-1]), dict(state_seq=None)):
        with pytest.raises(capi.MppiError) as e:
            capi.debug_plant_drive_host(**dict(args, **change))
        assert e.value.status == capi.ERR_INVALID, change


@functools.lru_cache(maxsize=None)
def _inputs(i):
    """Problem i's nominal solution and gains from the CPU oracle (fp32): what the nominal calls and the DDP pass deliver."""
    p = PC.problems()[i]
    orc = O.Oracle(p["cfg"])
    xs, us = orc.nominal_traj(p["x0"], p["U"])
    K = orc.ddp_feedback_gains(p["x0"], xs, us, Q=PC.DDP_Q, R=PC.DDP_R, Qf=PC.DDP_QF)["feedback"]
    return xs, us, K


def _host(p, xs, us, K, periods, substeps):
    pc = p["plant_cfg"]
    return capi.debug_plant_drive_host(pc["layers"], pc["theta"], pc["negate_yaw_der"], np.float32(1.0 / PC.HZ), p["cfg"]["u_lo"],
                                       p["cfg"]["u_hi"], p["x_plant"], xs, us, K, periods, substeps)


def test_the_host_text_is_within_1e_5_of_the_float64_restatement_for_every_gpu_case(L):
    clamped = corrected = 0
    worst = 0.0
    for i, p in enumerate(PC.problems()):
        xs, us, K = _inputs(i)
        assert np.all(np.isfinite(K))
        for periods, substeps, feedback in PC.CALLS:
            k = K if feedback else None
            got_x, got_u = _host(p, xs, us, k, periods, substeps)
            ref_x, ref_u, facts = PC.drive64(p["plant_cfg"], p["cfg"]["u_lo"], p["cfg"]["u_hi"], p["x_plant"], xs, us, k, periods, substeps)
            ex, eu = float(np.max(np.abs(got_x - ref_x))), float(np.max(np.abs(got_u - ref_u)))
            print("PLANTDRIVE inputs %s P=%d m=%d feedback=%d: host text against float64: state %.2e, applied controls %.2e (bound 1e-5); "
                  "largest |du| %.2e, clamp %s" % (PC.tag(i), periods, substeps, feedback, ex, eu, facts["max_du"], facts["clamped"]))
            assert np.all(np.isfinite(got_x)) and np.all(np.isfinite(got_u))
            assert ex <= HOST_BOUND and eu <= HOST_BOUND, (PC.tag(i), periods, substeps, feedback)
            clamped += int(facts["clamped"])
            corrected += int(facts["max_du"] > 1e-3)
            worst = max(worst, ex)
    assert clamped >= 3 and corrected >= 3, (clamped, corrected)
    print("PLANTDRIVE inputs: worst host-text distance %.2e; the clamp changed a control in %d runs, a correction above 1e-3 in %d" % (
        worst, clamped, corrected))


def test_the_flat_problems_keep_the_heading_at_zero(L):
    """The inputs of the GPU test's exact-bits case: with the plant's output neuron 3 zeroed and psi = s6 = 0 the host text's heading
    stays exactly 0 with feedback on, for m = 1 and m = 3 -- a correction goes into the controls only."""
    for i, p in enumerate(PC.problems(flat=True)):
        orc = O.Oracle(p["cfg"])
        xs, us = orc.nominal_traj(p["x0"], p["U"])
        K = orc.ddp_feedback_gains(p["x0"], xs, us, Q=PC.DDP_Q, R=PC.DDP_R, Qf=PC.DDP_QF)["feedback"]
        for m in (1, 3):
            x, _ = _host(p, xs, us, K, 2, m)
            assert x[2] == 0.0 and x[6] == 0.0, (PC.tag(i), m)
            assert abs(float(x[0] - p["x_plant"][0])) > 1e-3, "the car moves"


def test_a_nan_gain_falls_back_to_feed_forward(L):
    p = PC.problems()[1]
    xs, us, K = _inputs(1)
    bad = K.copy()
    bad[0, 1, 3] = np.float32(np.nan)   # one NaN gain in row 0: du[1] is NaN in step 0 (j == 0, row 0 alone)
    assert np.isnan(bad).sum() == 1
    with_nan = _host(p, xs, us, bad, 1, 1)
    forward = _host(p, xs, us, None, 1, 1)
    with_gain = _host(p, xs, us, K, 1, 1)
    np.testing.assert_array_equal(with_nan[1].view(np.uint32), forward[1].view(np.uint32))   # BOTH controls fall back, as the reference's
    np.testing.assert_array_equal(with_nan[0].view(np.uint32), forward[0].view(np.uint32))
    assert np.any(with_gain[1] != forward[1]), "the finite gains do change the applied control"
    ref = PC.drive64(p["plant_cfg"], p["cfg"]["u_lo"], p["cfg"]["u_hi"], p["x_plant"], xs, us, bad, 1, 1)
    assert ref[2]["nan_fallback"]
    assert float(np.max(np.abs(with_nan[0] - ref[0]))) <= HOST_BOUND
    # interpolated rows: at m = 3 the NaN of row 0 reaches steps 0, 1 and 2 (a weight of 1, 2/3, 1/3) -- all three are feed-forward
    nan3, fwd3 = _host(p, xs, us, bad, 1, 3), _host(p, xs, us, None, 1, 3)
    np.testing.assert_array_equal(nan3[1].view(np.uint32), fwd3[1].view(np.uint32))


def test_nothing_is_interpolated_at_j_zero(L):
    """control_seq[hi] = inf: at substeps = 1 every step has j == 0 and row hi is never read -- (1 - 0) v[lo] + 0 * inf would be NaN."""
    p = PC.problems()[2]
    xs, us, K = _inputs(2)
    periods = 2
    spiked = us.copy()
    spiked[periods] = np.float32(np.inf)    # row hi of the last step
    assert np.all(np.isinf(spiked[periods])) and np.all(np.isfinite(spiked[:periods]))
    a, b = _host(p, xs, spiked, K, periods, 1), _host(p, xs, us, K, periods, 1)
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    np.testing.assert_array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert np.all(np.isfinite(a[0]))
    # and at substeps = 2 the row IS read: the interpolated control is inf, the clamp takes it to the upper limit
    c = _host(p, xs, spiked, None, periods, 2)
    np.testing.assert_array_equal(c[1][-1], np.asarray(p["cfg"]["u_hi"], np.float32))
