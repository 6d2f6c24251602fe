"""The rollout trace (mppi_trace_rollouts / mppi_top_rollouts) without a GPU: the refusals that need no device, and the
reference side of tests/test_trace_gpu.py measured alone -- TOL_STATE and the cap of undecided rollouts come from here, not
from anything a kernel computes.

TOL_STATE: for every case of the GPU file the fp32 oracle (orc_update_state, the reference's arithmetic, mode 1) and the float64
loop (trace_cases.loop64: Ref64.state_deriv over ref64's clamp) are stepped over the SAME applied controls, those of the
oracle; the largest per-component |difference| over all rollouts and steps was 5.13e-6 (y, patchwork, basis functions, T = 37).
TOL_STATE is ten times that, the factor tests/measure_branch_deltas.py gives the oracle's own deviation."""
import ctypes as C

import numpy as np
import pytest

from autorally_amd import capi
from tests import scenes as SC
from tests import trace_cases as TC


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()


def test_null_handle_and_argument_refusals():
    L = capi.lib()
    k = (C.c_int * 2)(0, 1)
    assert L.mppi_trace_rollouts(None, k, 2, None, None, None, None, None) == capi.ERR_INVALID
    assert L.mppi_trace_rollouts(None, None, 0, None, None, None, None, None) == capi.ERR_INVALID
    assert L.mppi_top_rollouts(None, 1, k) == capi.ERR_INVALID
    assert L.mppi_top_rollouts(None, 0, None) == capi.ERR_INVALID
    assert "mppi_trace_rollouts" in capi.SYMBOLS and "mppi_top_rollouts" in capi.SYMBOLS
    assert L.mppi_abi_version() == 5


def test_running_mean_fold_is_the_kernels():
    """fold_step_costs against the formula written out in Python floats on a few sequences (a constant, a ramp, a cap)."""
    rows = np.array([[0.0, 3.0, 3.0, 3.0, 3.0], [0.0, 1.0, 2.5, 1e12, 7.0], [0.0, 0.1, 0.2, 0.3, 0.4]], np.float32)
    got = TC.fold_step_costs(rows)
    for r, g in zip(rows, got):
        J = np.float32(0.0)
        for t in range(1, len(r)):
            J = np.float32(float(J) + float(np.float32(r[t] - J)) / t)
        assert J.view(np.uint32) == g.view(np.uint32)
    assert got[0] == np.float32(3.0)


@pytest.mark.parametrize("case", TC.CASES, ids=TC.CASE_IDS)
def test_tol_state_covers_the_oracles_own_deviation(case):
    scene, net, T, stride, _ = case
    cfg = TC.problem(scene, net, T, stride)[0]
    V = TC.oracle_V(scene, net, T, stride)
    s64 = TC.states64(scene, net, T, stride)
    assert np.all(np.isfinite(s64))
    dev = np.abs(TC.loop32(cfg, V).astype(np.float64) - s64).max(axis=(0, 1))
    print("TRACE_TOL %s: fp32 oracle against float64, per component %s, max %.3e (TOL_STATE %.1e = x%.1f)" % (
        "%s-%s-T%d-s%d" % case[:4], np.array2string(dev, precision=2), dev.max(), TC.TOL_STATE, TC.TOL_STATE / dev.max()))
    assert dev.max() <= TC.MEASURED_STATE_DEV * 1.0001
    assert 10.0 * dev.max() <= TC.TOL_STATE
    assert TC.TOL_STATE <= 10.0 * TC.MEASURED_STATE_DEV * 1.02   # ten times the measurement, not more


@pytest.mark.parametrize("case", TC.CASES, ids=TC.CASE_IDS)
def test_start_poses_stay_inside_the_undecided_cap(case):
    """At most UNDECIDED_CAP of K undecided per case; the branch scenes do fire their branches at this K."""
    scene, net, T, stride, _ = case
    tr = TC.trace64(scene, net, T, stride)
    n_und = int(TC.K - tr["decided"].sum())
    print("TRACE_DECIDED %s: %d undecided, %d rollouts see the flag" % ("%s-%s-T%d-s%d" % case[:4], n_und, int((tr["first"] >= 0).sum())))
    assert n_und <= SC.UNDECIDED_CAP * TC.K


def test_the_branch_scenes_fire_at_this_size():
    flagged = {s: 0 for s in ("patchwork", "tilt_l1", "tilt_l2")}
    clear = dict(flagged)
    for scene, net, T, stride, _ in TC.CASES:
        if scene in flagged:
            first = TC.trace64(scene, net, T, stride)["first"]
            flagged[scene] += int((first >= 0).sum())
            clear[scene] += int((first < 0).sum())
    assert all(v > 0 for v in flagged.values()) and all(v > 0 for v in clear.values()), (flagged, clear)


def test_every_model_form_horizon_and_stride_is_a_case():
    assert {c[2] for c in TC.CASES} == {2, 5, 37} and {c[3] for c in TC.CASES} == {0, 1, 3}
    assert {c[0] for c in TC.CASES} == {"oval", "patchwork", "tilt_l1", "tilt_l2"}
    forms = {(c[1], v) for c in TC.CASES for v in c[4]}
    want = {("32x2", "row_exact"), ("32x2", "quad"), ("32x2", "valu"), ("64x2", "m44_chain"), ("64x2", "oct"), ("16-24", "lds44"),
            ("32x3", "lds44"), ("33-97-66", "lds128"), ("129", "valu_lds"), ("256-7", "valu_lds"), ("200-256", "valu_lds"),
            ("256x2", "valu_lds"), ("none", "valu_lds"), ("8deep", "valu_lds"), ("bf", "bf3"), ("bf", "quad"), ("bf", "fused"),
            ("32x2", "row_tree"), ("64x2", "m44"), ("32x2", "multi4_tree"), ("197-67", "valu_lds"), ("128x2", "valu_lds"),
            ("16-256", "valu_lds"), ("64-200", "valu_lds"), ("70-193", "valu_lds"), ("24-150", "valu_lds"), ("100-140", "valu_lds")}
    assert want <= forms, want - forms
    assert len(TC.NETS["8deep"]) == capi.MAX_LAYERS
    # three and four chains per lane over more than one chunk of 8 inputs, image in LDS and in global memory (64 KB with tiles)
    def wide(net, chains):
        L = TC.NETS[net]
        return any(-(-nout // 64) == chains and nin >= 16 for nin, nout in zip(L[:-1], L[1:]))

    def in_lds(net):
        L = TC.NETS[net]
        return 8192 + 4 * sum((a + 1) * b for a, b in zip(L[:-1], L[1:])) <= 65536
    served = {c[1] for c in TC.CASES if c[1] not in TC.NO_ROLLOUT_KERNEL and c[1] != "bf" and TC.NETS[c[1]]}
    for chains in (3, 4):
        assert any(wide(n, chains) and in_lds(n) for n in served) and any(wide(n, chains) and not in_lds(n) for n in served), chains
