"""The row forms with the dynamics waves' hand-over per CHUNK of four steps (rollout_row.hip: row_step / row_dynamics): the
sequence word published once per aligned chunk, the control wave's count read once per chunk, ring slots as compile-time
offsets.  Nothing of a solve's arithmetic changed, so every bit must be what it was.

Shapes: horizons around the chunk (T - 1 network steps: every remainder mod 4, T <= 4, one chunk short of / beyond the
16-step ring, the headline's 100 and its neighbours) x rollouts from four groups (K = 64, the smallest K mppi_create accepts) to one group per CU and beyond.
  * "row_exact" against another exact form (the single-wave MFMA form) on the same inputs, bit for bit;
  * "row_tree": V, costs and U bit for bit against the arrays of the build BEFORE the change, recorded once as SHA-256 per
    shape (tests/golden/row_chunked_parent.json, written by tools/record_row_chunked_golden.py), and the two bars of
    tests/test_row_tree_gpu.py (its own oracle mode, the nominal oracle);
  * generator noise, the gated launch (mppi_arm; chained ticks) and a two-handle batch against the plain explicit solve;
  * mppi_debug_inject_handover_fault for every role of the group at one T = 1 and one T = 3 (mod 4): the call returns
    MPPI_ERR_HIP, the next solve on the handle is good.  (The hook starts one wave with an exhausted poll budget: its waits
    give up, the group's costs become NaN, the kernel runs to its end.)
"""
import hashlib
import json
import os

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import synthetic as S
from oracle import oracle as O
from tests.helpers import noise_for, rel_err, warm_U

pytestmark = pytest.mark.gpu

TS = [2, 3, 4, 5, 17, 50, 99, 100, 101, 103]
KS = [64, 128, 1920, 4096]  # 64 is the smallest K there is: mppi_create takes multiples of 64 only (see the test below)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_chunked_parent.json")
WAIT = 0.1  # the longest gate wait mppi_arm accepts


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def sha(x):
    return hashlib.sha256(np.ascontiguousarray(x, dtype=np.float32).tobytes()).hexdigest()


def inputs(K, T):
    cfg = S.make_config(K, T, track="oval")
    return cfg, warm_U(cfg), noise_for(cfg, 1234)


def solve(cfg, U0, eps, variant):
    """one solve on explicit noise: results + applied controls + the name of the form that ran"""
    sol = capi.Solver(cfg)
    sol.set_rollout_variant(variant)
    sol.set_control_seq(U0)
    sol.set_control_hist(np.zeros(4, np.float32))
    sol.set_noise(eps)
    sol.compute_control(cfg["start_state"])
    got = sol.get_results()
    got["V"] = sol.get_applied_controls()
    got["variant"] = sol.rollout_variant()
    sol.close()
    return got


def test_sixteen_rollouts_are_not_a_shape():
    """One group alone (K = 16) cannot be asked for: mppi_create rejects a K that is not a multiple of 64, for every
    form.  The smallest shape of this file is therefore K = 64, four groups."""
    with pytest.raises(capi.MppiError) as e:
        capi.Solver(S.make_config(16, 5, track="oval"))
    assert e.value.status == capi.ERR_INVALID


def _same(a, b, keys=("costs", "U"), what=""):
    for k in keys:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg="%s %s" % (what, k))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("T", TS)
def test_row_exact_is_bit_identical_to_the_single_wave_form(K, T):
    cfg, U0, eps = inputs(K, T)
    row = solve(cfg, U0, eps, "row_exact")
    assert "row8w_h32" in row["variant"]
    other = solve(cfg, U0, eps, "fused")
    assert "fused" in other["variant"]
    _same(row, other, ("V", "costs", "U"), "K=%d T=%d" % (K, T))


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("T", TS)
def test_row_tree_keeps_the_recorded_bits_and_its_bars(K, T):
    with open(GOLDEN) as f:
        want = json.load(f)["K%d_T%d" % (K, T)]
    cfg, U0, eps = inputs(K, T)
    got = solve(cfg, U0, eps, "row_tree")
    assert "row8w_tree" in got["variant"]
    # ---- the build before the change, bit for bit
    assert sha(got["V"]) == want["V"]
    assert sha(got["costs"]) == want["costs"]
    assert sha(got["U"]) == want["U"]
    # ---- the bars of tests/test_row_tree_gpu.py: its own oracle mode ...
    hist = np.zeros(4, np.float32)
    ref2 = O.Oracle(cfg, fma_mode=2, nthreads=8).compute_control(cfg["start_state"], U0, hist, eps)
    ref1 = O.Oracle(cfg, fma_mode=1, nthreads=8).compute_control(cfg["start_state"], U0, hist, eps)
    np.testing.assert_array_equal(_bits(got["V"]), _bits(ref2["V"][-1]))
    err2 = rel_err(got["costs"], ref2["costs"])
    print("K=%d T=%d own mode: flipped %d, p99 %.3e, |dU| %.3e" % (K, T, int(np.sum(err2 > 1e-4)), float(np.percentile(err2, 99)),
                                                                 float(np.max(np.abs(got["U"] - ref2["U"])))))
    assert int(np.sum(err2 > 1e-4)) <= max(K // 200, 1), float(err2.max())
    assert float(np.percentile(err2, 99)) < 5e-6
    assert float(np.abs(got["w"] - ref2["w"]).sum()) / float(ref2["w"].sum()) < 1e-4
    assert np.max(np.abs(got["U"] - ref2["U"])) <= 1e-4
    assert abs(got["traj_cost"] - ref2["traj_cost"]) <= 1e-4 * abs(ref2["traj_cost"])
    # ---- ... and the nominal oracle (the reference's summation order)
    np.testing.assert_array_equal(_bits(got["V"]), _bits(ref1["V"][-1]))
    err1 = rel_err(got["costs"], ref1["costs"])
    assert int(np.sum(err1 > 1e-4)) <= max(K // 200, 1), float(err1.max())
    assert np.max(np.abs(got["U"] - ref1["U"])) <= 1e-4
    assert abs(got["traj_cost"] - ref1["traj_cost"]) <= 1e-4 * abs(ref1["traj_cost"])


@pytest.mark.parametrize("variant", ["row_tree", "row_exact"])
@pytest.mark.parametrize("K", [128, 1920])
@pytest.mark.parametrize("T", TS)
def test_generator_gate_and_batch_change_no_bit(K, T, variant):
    cfg, U0, eps = inputs(K, T)
    one = solve(cfg, U0, eps, variant)
    what = "%s K=%d T=%d" % (variant, K, T)
    # ---- the noise wave's draws instead of explicit noise
    sol = capi.Solver(cfg)
    sol.set_rollout_variant(variant)
    sol.set_control_seq(U0)
    sol.seed(1234, 0)
    sol.compute_control(cfg["start_state"])
    _same(sol.get_results(), one, what=what + " generator")
    # ---- two controllers in one launch, distinct states
    st2 = cfg["start_state"].copy()
    st2[4] += 0.7
    other = capi.Solver(cfg)
    other.set_rollout_variant(variant)
    for s_ in (sol, other):
        s_.set_control_seq(U0)
        s_.set_control_hist(np.zeros(4, np.float32))
        s_.set_noise(eps)
    capi.compute_control_batch([sol, other], np.stack([cfg["start_state"], st2]))
    _same(sol.get_results(), one, what=what + " batch[0]")
    _same(other.get_results(), solve(dict(cfg, start_state=st2), U0, eps, variant), what=what + " batch[1]")
    sol.close()
    other.close()


def _ticks(cfg, U0, variant, n, how):
    """n control ticks in generator mode from drifting states: plain solves, armed solves, or one chained call"""
    sol = capi.Solver(cfg)
    sol.set_rollout_variant(variant)
    sol.set_control_seq(U0)
    sol.seed(7, 0)
    opt = int(cfg["opt_stride"])
    out = []
    if how == "chained":
        sol.control_ticks(cfg["start_state"], n, opt)
        r = sol.get_results()
        out.append(dict(U=r["U"].copy(), costs=r["costs"].copy(), seq=sol.get_control_seq().copy()))
    else:
        for i in range(n):
            state = cfg["start_state"].copy()
            if how != "fixed":
                state[4] += 0.05 * i
            if how == "armed" and i > 0:
                sol.arm(WAIT)
                assert sol.is_armed()
            sol.compute_control(state)
            sol.slide_control_seq(opt)
            r = sol.get_results()
            out.append(dict(U=r["U"].copy(), costs=r["costs"].copy(), seq=sol.get_control_seq().copy()))
    sol.close()
    return out


@pytest.mark.parametrize("variant", ["row_tree", "row_exact"])
@pytest.mark.parametrize("K", [128, 4096])
@pytest.mark.parametrize("T", TS)
def test_gated_launches_change_no_bit(K, T, variant):
    """mppi_arm with a new state every tick, and the chained ticks of mppi_control_ticks, against plain solves.  The plain
    handle runs its whole sequence first (a gated kernel holds its CUs until its gate opens)."""
    cfg = S.make_config(K, T, track="oval")
    U0 = warm_U(cfg)
    n = 4
    plain = _ticks(cfg, U0, variant, n, "plain")
    armed = _ticks(cfg, U0, variant, n, "armed")
    for i in range(n):
        _same(armed[i], plain[i], ("costs", "U", "seq"), "%s K=%d T=%d armed tick %d" % (variant, K, T, i))
    fixed = _ticks(cfg, U0, variant, n, "fixed")
    chained = _ticks(cfg, U0, variant, n, "chained")
    _same(chained[0], fixed[-1], ("costs", "U", "seq"), "%s K=%d T=%d chained ticks" % (variant, K, T))


@pytest.mark.parametrize("variant", ["row_tree", "row_exact"])
@pytest.mark.parametrize("T", [101, 103])  # T - 1 network steps: a last chunk of 4 / of 2; T = 1 and 3 (mod 4)
@pytest.mark.parametrize("wave", [1, 2, 3, 4, 5, 6, 7, 8])  # dynamics waves 1..4, pose, cost, control, noise
def test_a_failed_hand_over_is_reported_for_every_role(wave, T, variant):
    cfg = S.make_config(256, T, track="oval")
    sol = capi.Solver(cfg)
    sol.set_rollout_variant(variant)
    sol.compute_control(cfg["start_state"])
    good = sol.get_results()
    assert np.all(np.isfinite(good["costs"])) and np.all(np.isfinite(good["U"]))
    sol.debug_inject_handover_fault(wave, 32)
    with pytest.raises(capi.MppiError) as e:
        sol.compute_control(cfg["start_state"])
    assert e.value.status == capi.ERR_HIP and "hand-over" in str(e.value)
    sol.debug_inject_handover_fault(0, 0)  # back to normal: the handle keeps working
    sol.reset_controls()
    sol.seed(cfg.get("seed", 1234), 0)
    sol.compute_control(cfg["start_state"])
    again = sol.get_results()
    _same(again, good, what="after the fault")
    sol.close()
