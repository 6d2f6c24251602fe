"""The "bf_row" rollout form (csrc/rollout_bf_row.hip): the basis-function model in the row form's group -- a rollout's sixteen
(output, y-thread) cells on one DPP row, four rollouts per dynamics wavefront, four dynamics wavefronts and the four riders of
csrc/group_roles.hpp per 16 rollouts.  By name only; its contract is the BITS of "bf3" (and of "quad" and "fused"), plus what
"bf3" does not have: the gated kernel behind mppi_arm, mppi_arm_batch and the chained mppi_control_ticks.
  1. names and the refusal on a network handle;
  2. bits of "bf3" with explicit noise: every chunk remainder and ring wrap of T, strides 0 / 1 / 3, control cost on and off,
     l1_cost, an affine and a projective transform, oval / ring / ramp, K = 2560 at T = 100, at and beyond two groups per CU;
  3. generator mode (three consecutive solves) against "bf3" and "fused"; two iterations;
  4. every rollout on the flip-free ramp against tests/ref64.py;
  5. the edge scenes "bf3" is held on, then +inf, NaN and 1e30 in s3..s6 of the start state: bits of "bf3";
  6. hand-over faults of all eight roles; 7. solve-ahead; 8. two handles in one launch; 9. mppi_trace_rollouts.
Every comparison with "bf3" is uint32-equal; non-finite values are compared as bits."""
import functools
import os

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import params as P
from autorally_amd import synthetic as S
from tests import edge_cases as EC
from tests import ref64 as R
from tests import scenes as SC
from tests.helpers import noise_for, rel_err, warm_U
from tests.scenes import TOL64

pytestmark = pytest.mark.gpu

U32 = np.uint32
V = "bf_row"
NAME = "basis_funcs25_row8w"
BF3_NAME = "basis_funcs25_valu_3w"
# T: the four remainders of the riders' chunks of four (21, 22, 23, 24), fewer steps than a chunk (2), one wrap of the 16-step
# ring (17 .. 24) and two (37)
TS = [2, 5, 17, 21, 22, 23, 24, 37]
CTRL_COST = dict(steering_coeff=0.3, throttle_coeff=0.25)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


@functools.lru_cache(maxsize=None)
def _cus():
    """The device's CU count, asked as tests/test_every_rollout_gpu.py asks it: in a child process (torch brings a HIP runtime
    of its own)."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    n = int(out.stdout.split()[-1])
    assert 32 <= n <= 1024, n
    return n


@functools.lru_cache(maxsize=None)
def _bf_W():
    return P.load_bf_npz(os.path.join(os.path.dirname(__file__), "golden", "models", "basis_function_09_12_2018.npz"))


def _solver(cfg, variant, U0, eps=None, seed=None, hist=None):
    sol = capi.Solver(cfg)
    try:
        if variant != "auto":
            sol.set_rollout_variant(variant)
        sol.set_control_seq(U0)
        sol.set_control_hist(np.zeros(4, np.float32) if hist is None else hist)
        if eps is not None:
            sol.set_noise(eps)
        else:
            sol.seed(seed, 0)
    except Exception:
        sol.close()
        raise
    return sol


def _results(sol):
    got = sol.get_results()
    got["V"] = sol.get_applied_controls()
    got["variant"] = sol.rollout_variant()
    return got


def _solve(cfg, variant, U0, eps=None, seed=None, state=None, hist=None):
    sol = _solver(cfg, variant, U0, eps, seed, hist)
    try:
        sol.compute_control(cfg["start_state"] if state is None else state)
        return _results(sol)
    finally:
        sol.close()


def _same_bits(a, b, what, keys=("costs", "w", "V", "U")):
    for key in keys:
        np.testing.assert_array_equal(a[key].view(U32), b[key].view(U32), err_msg="%s: %s" % (what, key))
    assert np.float32(a["traj_cost"]).view(U32) == np.float32(b["traj_cost"]).view(U32), (what, a["traj_cost"], b["traj_cost"])


def _pair_bits(cfg, U0, what, others=("bf3",), **kw):
    got = _solve(cfg, V, U0, **kw)
    assert got["variant"] == NAME, got["variant"]
    for v in others:
        ref = _solve(cfg, v, U0, **kw)
        assert ref["variant"] != NAME
        _same_bits(got, ref, "%s vs %s" % (what, v))
    return got


# ------------------------------------------------------------------------------------------------------------------ 1
def test_names_and_the_refusal_on_a_network_handle():
    cfg = S.make_config(64, 5, track="oval", bf_W=_bf_W())
    sol = capi.Solver(cfg)
    try:
        assert sol.rollout_variant() == BF3_NAME
        sol.set_rollout_variant(V)
        assert sol.rollout_variant() == NAME
        sol.set_rollout_variant("auto")
        assert sol.rollout_variant() == BF3_NAME
        assert sol.form_candidates() == ["bf3", "quad", "fused"]
    finally:
        sol.close()
    sol = capi.Solver(S.make_config(64, 5, track="oval"))
    try:
        before = sol.rollout_variant()
        with pytest.raises(capi.MppiError) as e:
            sol.set_rollout_variant(V)
        assert e.value.status == capi.ERR_UNSUPPORTED, e.value.status
        assert "bf_row" in str(e.value)
        assert sol.rollout_variant() == before
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------------------------ 2
def _scene(track, K, T, stride, ctrl, l1=False):
    """oval and ring: an affine costmap transform; ramp: the projective one of tests/scenes.py"""
    bf_W = _bf_W()
    if track == "ramp":
        cfg = SC.ramp_config(K, T, bf_W=bf_W, opt_stride=stride)
        U0 = SC.ramp_U(cfg, seed=K % 31 + T)
    else:
        cfg = S.make_config(K, T, track=track, bf_W=bf_W, opt_stride=stride)
        U0 = warm_U(cfg)
    cfg["cost"] = dict(cfg["cost"], l1_cost=bool(l1), **(CTRL_COST if ctrl else dict(steering_coeff=0.0, throttle_coeff=0.0)))
    return cfg, U0


# (track, optimization_stride, control cost, l1_cost): every stride, both cost settings and both transforms on every (K, T)
VARIATIONS = [("oval", 1, False, False), ("oval", 0, True, False), ("ring", 3, True, True), ("ring", 1, False, False),
              ("ramp", 3, False, False), ("ramp", 0, True, True)]


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("K", [64, 192])
def test_bits_of_bf3_with_explicit_noise(K, T):
    """Costs, weights, V, U and the trajectory cost as uint32, the noise-free rollout 0 and the pure-noise tail k >= k99 among
    them."""
    for track, stride, ctrl, l1 in VARIATIONS:
        cfg, U0 = _scene(track, K, T, stride, ctrl, l1)
        affine = np.all(np.asarray(cfg["r_c1"])[2:] == 0) and np.all(np.asarray(cfg["r_c2"])[2:] == 0) and np.asarray(cfg["trs"])[2] == 1
        assert affine == (track != "ramp")
        got = _pair_bits(cfg, U0, "K=%d T=%d %s stride=%d ctrl=%s l1=%s" % (K, T, track, stride, ctrl, l1), eps=noise_for(cfg, 4321 + T))
        assert np.all(np.isfinite(got["costs"]))
        print("BF_ROW bits K=%d T=%d %s stride=%d ctrl=%d l1=%d: equal to bf3; costs %.4g .. %.4g, %d distinct" % (
            K, T, track, stride, ctrl, l1, float(got["costs"].min()), float(got["costs"].max()), len(np.unique(got["costs"]))))


def test_bits_of_bf3_at_the_reference_shape():
    cfg, U0 = _scene("oval", 2560, 100, 1, True)
    got = _pair_bits(cfg, U0, "K=2560 T=100", eps=noise_for(cfg, 77))
    assert len(np.unique(got["costs"])) > 1280


def test_bits_of_bf3_at_and_beyond_two_groups_per_cu():
    cap = 2 * _cus() * 16
    for K in (cap, cap + 64):
        cfg, U0 = _scene("ramp", K, 21, 1, True)
        _pair_bits(cfg, U0, "K=%d T=21" % K, eps=noise_for(cfg, 99))


# ------------------------------------------------------------------------------------------------------------------ 3
def test_generator_mode_three_consecutive_solves():
    """The group's noise wave draws what "bf3"'s control wave and the stand-alone generator in front of "fused" draw."""
    cfg, U0 = _scene("oval", 192, 21, 1, True)
    runs = {}
    for v in (V, "bf3", "fused"):
        sol = _solver(cfg, v, U0, seed=5)
        try:
            out = []
            for _ in range(3):
                sol.compute_control(cfg["start_state"])
                out.append(_results(sol))
                sol.slide_control_seq(1)
            runs[v] = out
        finally:
            sol.close()
    assert runs[V][0]["variant"] == NAME and runs["fused"][0]["variant"] == "basis_funcs25_valu"
    for i in range(3):
        for v in ("bf3", "fused"):
            _same_bits(runs[V][i], runs[v][i], "solve %d vs %s" % (i, v))
    assert not np.array_equal(runs[V][0]["U"], runs[V][2]["U"])


def test_two_iterations():
    cfg, U0 = _scene("oval", 192, 22, 1, True)
    cfg["num_iters"] = 2
    _pair_bits(cfg, U0, "two iterations, explicit", eps=noise_for(cfg, 11))
    _pair_bits(cfg, U0, "two iterations, generator", seed=9)


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("K,T", [(64, 21), (192, 21), (64, 100), (192, 100)])
def test_every_rollout_against_float64(K, T):
    cfg = SC.ramp_config(K, T, bf_W=_bf_W())
    U0 = SC.ramp_U(cfg, seed=K % 31 + T)
    eps = noise_for(cfg, 1000 + T)
    got = _solve(cfg, V, U0, eps)
    assert got["variant"] == NAME
    costs_r, _, crash_r = R.Ref64(cfg).rollouts(cfg["start_state"], U0, eps[0])
    assert not np.any(crash_r)
    assert len(np.unique(got["costs"])) > K // 2, "the rollouts of this case are not distinct"
    e64 = rel_err(got["costs"], costs_r)
    k64 = int(np.argmax(e64))
    print("BF_ROW ref64 K=%d T=%d: max %.2e (k=%d, margin x%.1f)" % (K, T, e64[k64], k64, TOL64 / max(e64[k64], 1e-30)))
    assert float(e64[k64]) <= TOL64, ("ref64", k64, float(e64[k64]), int(np.sum(e64 > TOL64)))


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("scene", EC.SCENES)
def test_the_edge_scenes_bf3_is_held_on(scene):
    """tests/edge_cases.py on the basis-function model: off the map, the crawl (u_x on both sides of the model's 0.1 switch),
    the cap, the far headings; the shapes of tests/test_edge_rollouts_gpu.py, the border also at T = 100 (a rollout that left the
    map comes back)."""
    for K, T in EC.shapes(scene):
        for part in EC.parts(scene, "bf"):
            cfg, U0, eps = EC.problem(scene, part, "bf", K, T)
            _pair_bits(cfg, U0, "%s/%s K=%d T=%d" % (scene, part, K, T), eps=eps)


@pytest.mark.parametrize("value", [np.inf, np.nan, 1e30], ids=["inf", "nan", "1e30"])
def test_non_finite_and_huge_start_states(value):
    """+inf, NaN and 1e30 in s3 .. s6 of the start state, one at a time (+inf in s3 and s6 reaches the plain basis functions:
    the value itself, not value / 1)."""
    cfg = SC.ramp_config(64, 21, bf_W=_bf_W())
    U0, eps = SC.ramp_U(cfg), noise_for(cfg, 31)
    for i in (3, 4, 5, 6):
        state = np.array(cfg["start_state"], np.float32)
        state[i] = value
        got, ref = (_solve(cfg, v, U0, eps, state=state, hist=EC.START_HIST) for v in (V, "bf3"))
        _same_bits(got, ref, "s%d = %r" % (i, value))


# ------------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("wave", range(1, 9))
def test_a_starved_wave_fails_the_solve_loudly(wave):
    """Roles as for the row form: 1 .. 4 dynamics waves, then pose, cost, control, noise wave (mppi_debug_inject_handover_fault)."""
    cfg, U0 = _scene("oval", 64, 21, 1, True)
    ref = _solve(cfg, "bf3", U0, seed=1234)
    sol = _solver(cfg, V, U0, seed=1234)
    try:
        sol.debug_inject_handover_fault(wave, 32)
        with pytest.raises(capi.MppiError) as e:
            sol.compute_control(cfg["start_state"])
        assert e.value.status == capi.ERR_HIP
        assert np.all(np.isnan(sol.rollout_only(cfg["start_state"])))  # the kernel alone: every workgroup poisoned its costs
        sol.debug_inject_handover_fault(0, 0)
        sol.set_control_seq(U0)
        sol.set_control_hist(np.zeros(4, np.float32))
        sol.seed(1234, 0)
        sol.compute_control(cfg["start_state"])
        _same_bits(_results(sol), ref, "after the fault of role %d" % wave)
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------------------------ 7
def _tick_loop(cfg, armed, n=20):
    """n ticks with a new state every tick (the nominal trajectory's next state); armed: mppi_arm before every compute."""
    sol = capi.Solver(cfg)
    out = []
    try:
        sol.set_rollout_variant(V)
        sol.seed(77, 0)
        state = np.array(cfg["start_state"], np.float32)
        for _ in range(n):
            if armed:
                sol.arm(0.1)
                assert sol.is_armed()
                assert sol.debug_launch_info() == (1, 1)
            sol.compute_control(state)
            assert not sol.is_armed()
            out.append(sol.get_results())
            sol.slide_control_seq(cfg["opt_stride"])
            state = sol.nominal_traj(state)[0][1].copy()
        if armed:  # armed, called off, solved as if it never was: the generator is where it was
            sol.arm(0.1)
            assert sol.is_armed()
            sol.disarm()
            assert not sol.is_armed()
        sol.compute_control(state)
        out.append(sol.get_results())
    finally:
        sol.close()
    return out


@pytest.mark.parametrize("K", [64, 1920])
def test_armed_loop_equals_the_unarmed_loop(K):
    cfg = S.make_config(K, 21, track="oval", bf_W=_bf_W(), opt_stride=1)
    a, b = _tick_loop(cfg, True), _tick_loop(cfg, False)
    assert len(a) == len(b) == 21
    for i, (x, y) in enumerate(zip(a, b)):
        _same_bits(x, y, "tick %d" % i, keys=("costs", "w", "U"))
    assert not np.array_equal(a[0]["U"], a[5]["U"])


@pytest.mark.parametrize("K", [64, 1920])
def test_chained_control_ticks_equal_the_unchained_loop(K):
    cfg = S.make_config(K, 21, track="oval", bf_W=_bf_W(), opt_stride=1)
    st, opt, n = cfg["start_state"], 1, 20
    sols = [capi.Solver(cfg) for _ in range(3)]
    try:
        for sol in sols:
            sol.set_rollout_variant(V)
            sol.seed(77, 0)
        sols[1].debug_set_chained_ticks(0)
        sols[0].control_ticks(st, n, opt)   # chained: every solve but the first armed one tick ahead
        assert not sols[0].is_armed()
        assert sols[0].debug_launch_info() == (1, 1), "the chained ticks ran gated"
        sols[1].control_ticks(st, n, opt)   # every solve launched when its turn comes
        assert sols[1].debug_launch_info() == (1, 0)
        for _ in range(n):
            sols[2].compute_control(st)
            sols[2].slide_control_seq(opt)
        res = []
        for sol in sols:
            assert sol.rollout_variant() == NAME
            res.append((sol.get_control_seq(), sol.get_control_hist()))
            sol.compute_control(st)
            res[-1] += (sol.get_results(),)
        for U, hist, r in res[1:]:
            np.testing.assert_array_equal(res[0][0].view(U32), U.view(U32))
            np.testing.assert_array_equal(res[0][1].view(U32), hist.view(U32))
            _same_bits(res[0][2], r, "after the ticks", keys=("costs", "w", "U"))
        assert np.all(np.isfinite(res[0][2]["U"]))
    finally:
        for sol in sols:
            sol.close()


# ------------------------------------------------------------------------------------------------------------------ 8
def _pair(Ks, T=21):
    """Two controllers: their own K, costmap instance, cost parameters and seed"""
    return [S.make_config(K, T, track="oval", bf_W=_bf_W(), opt_stride=1, instance=i, seed=77 + i,
                          cost=dict(P.DEFAULT_COST, desired_speed=6.0 + i, speed_coeff=4.25 + i, **CTRL_COST)) for i, K in enumerate(Ks)]


@pytest.mark.parametrize("armed", [False, True], ids=["plain", "armed"])
@pytest.mark.parametrize("Ks,together", [((64, 128), True), ((2560, 2560), False)], ids=["64+128", "2x2560"])
def test_two_handles_in_mppi_compute_control_batch(Ks, together, armed):
    """K = 64 and 128 with different cost parameters and seeds: ONE rollout launch (the smaller instance's surplus workgroups
    return early), gated after mppi_arm_batch.  2 x 2560 is more than one dynamics wave per SIMD: solved, and armed, handle by
    handle.  Either way each handle's bits are those of its own solo solve."""
    cfgs = _pair(Ks)
    solo = [_solve(cfg, V, warm_U(cfg), seed=500 + i) for i, cfg in enumerate(cfgs)]  # first: a gated kernel holds its CUs
    sols = []
    try:
        for i, cfg in enumerate(cfgs):
            sols.append(_solver(cfg, V, warm_U(cfg), seed=500 + i))
        n = 2 if together else 1
        if armed:
            capi.arm_batch(sols, 0.1)
            assert all(s.is_armed() for s in sols)
            assert [s.debug_launch_info() for s in sols] == [(n, 1)] * 2
        capi.compute_control_batch(sols, [cfg["start_state"] for cfg in cfgs])
        assert not any(s.is_armed() for s in sols)
        infos = [s.debug_launch_info() for s in sols]
        print("BF_ROW batch Ks=%s armed=%s: launch info %s" % (Ks, armed, infos))
        assert infos == [(n, 1 if armed else 0)] * 2
        for i, s in enumerate(sols):
            got = _results(s)
            assert got["variant"] == NAME
            _same_bits(got, solo[i], "instance %d armed=%s" % (i, armed))
    finally:
        for s in sols:
            s.close()


# ------------------------------------------------------------------------------------------------------------------ 9
def test_the_trace_of_a_bf_row_solve():
    """mppi_trace_rollouts replays chosen rollouts of the last solve: costs[i] == costs[ks[i]] of mppi_get_results bit for bit
    (control-cost coefficients 0: the library refuses the trace's cost outputs otherwise)."""
    cfg, U0 = _scene("oval", 192, 37, 1, False)
    ks = np.array([0, 1, 15, 16, 17, 63, 64, 100, 190, 191, 5, 5], np.int32)
    sol = _solver(cfg, V, U0, eps=noise_for(cfg, 3))
    try:
        sol.compute_control(cfg["start_state"])
        got = _results(sol)
        tr = sol.trace_rollouts(ks)
    finally:
        sol.close()
    assert got["variant"] == NAME
    np.testing.assert_array_equal(np.ascontiguousarray(tr["costs"]).view(U32), got["costs"][ks].view(U32))
    lo, hi = np.asarray(cfg["u_lo"], np.float32), np.asarray(cfg["u_hi"], np.float32)
    np.testing.assert_array_equal(np.ascontiguousarray(tr["controls"]).view(U32), np.clip(got["V"][ks], lo, hi).view(U32))
