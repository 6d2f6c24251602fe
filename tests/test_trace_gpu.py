"""mppi_trace_rollouts / mppi_top_rollouts on the device (csrc/rollout_trace.hip: one wavefront per traced rollout, one lane per
neuron; one lane per rollout for the basis functions), tied to the real rollout kernels and to float64.

Per case of tests/trace_cases.py (K = 128, T in {2, 5, 37}, stride in {0, 1, 3}; oval, patchwork, tilt-slide; every model and
form of the list there) ALL K rollouts are traced, plus a shuffled subset with duplicates:
  1. costs == costs[ks] of mppi_get_results BIT FOR BIT on every order-exact form -- the forms whose name the oracle's mode 1
     (the reference's order in every layer) states, tests/helpers.oracle_mode_for.  The re-associating forms are held on states
     and controls only: the automatic "row_tree", "m44" and "multi4_tree", and "m44_chain", which keeps the hidden layers' order
     but sums the OUTPUT layer as a butterfly (include/mppi_hip.h, oracle mode 3) -- for those the number of rollouts whose cost
     differs and the largest relative difference on the decided rollouts are printed, not asserted;
     controls == clip(V) bit for bit, states[:, 0] == the solve's state, V == the oracle's V (what the cached float64 loop ran on);
  2. states within TOL_STATE of the float64 loop, every rollout and step (TOL_STATE: tests/test_trace_cpu.py);
  3. first_crash == ref64's `first` on every decided rollout (at most 10 % undecided: asserted on the CPU);
  4. step_costs folded on the host as running_mean reproduce costs bit for bit.
Then sequencing, the armed handle, the refusals, mppi_top_rollouts and one time bar against the parent's only kernel that
serves every layer list."""
import time

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import synthetic as S
from tests import trace_cases as TC
from tests.helpers import noise_for, oracle_mode_for, rel_err, warm_U

pytestmark = pytest.mark.gpu

U32 = np.uint32
K = TC.K
WAIT = 0.1   # as tests/test_solve_ahead_gpu.py: the longest gate wait mppi_arm accepts


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(U32)


def _solver(cfg, variant, U0, eps=None, seed=None):
    sol = capi.Solver(cfg)
    if variant not in (None, "auto"):
        sol.set_rollout_variant(variant)
    if U0 is not None:
        sol.set_control_seq(U0)
    if eps is not None:
        sol.set_noise(eps)
    elif seed is not None:
        sol.seed(seed, 0)
    return sol


def _same_trace(a, b, what=""):
    assert sorted(a) == sorted(b)
    for k in a:
        np.testing.assert_array_equal(np.ascontiguousarray(a[k]).view(U32), np.ascontiguousarray(b[k]).view(U32), err_msg="%s %s" % (what, k))


def _form_cases(served):
    return [pytest.param(c, v, id="%s-%s-T%d-s%d-%s" % (c[:4] + (v,))) for c in TC.CASES for v in c[4]
            if (c[1] not in TC.NO_ROLLOUT_KERNEL) == served]


@pytest.mark.parametrize("case,variant", _form_cases(True))
def test_trace_of_every_rollout(case, variant):
    _hold_case(case, variant)


@pytest.mark.parametrize("case,variant", _form_cases(False))
def test_lists_no_rollout_kernel_serves(case, variant):
    """6-200-256-4 and 6-256-256-4 (trace_cases.NO_ROLLOUT_KERNEL): mppi_create accepts them, "valu_lds" -- the only rollout form
    for lists this wide -- cannot hold them in the LDS and the solve fails at its launch: there is nothing to trace, and the
    trace says so (MPPI_ERR_STATE).  If a solve of such a list succeeds one day, the case is held to the full bar."""
    cfg, U0, eps = TC.problem(*case[:4])
    sol = _solver(cfg, variant, U0, eps)
    try:
        try:
            sol.compute_control(cfg["start_state"])
            solved = True
        except capi.MppiError as e:
            solved = False
            assert e.status == capi.ERR_HIP, e
            with pytest.raises(capi.MppiError) as e2:
                sol.trace_rollouts([0, 1])
            assert e2.value.status == capi.ERR_STATE
    finally:
        sol.close()
    print("TRACE %s: a solve of this list %s" % ("%s-%s-T%d-s%d" % case[:4], "ran" if solved else "is refused by the rollout launch: no trace"))
    if solved:
        _hold_case(case, variant)


def _hold_case(case, variant):
    scene, net, T, stride, _ = case
    cfg, U0, eps = TC.problem(scene, net, T, stride)
    sol = _solver(cfg, variant, U0, eps)
    try:
        sol.compute_control(cfg["start_state"])
        name = sol.rollout_variant()
        res = sol.get_results()
        V = sol.get_applied_controls()
        tr = sol.trace_rollouts(np.arange(K))
        rng = np.random.RandomState(T + stride)
        sub = np.concatenate([rng.permutation(K)[:41], [0, K - 1, K - 1, 5, 5, 5]]).astype(np.int32)
        rng.shuffle(sub)
        trs = sol.trace_rollouts(sub)
        top = sol.top_rollouts(17)
    finally:
        sol.close()
    exact = oracle_mode_for(name) == 1
    # the shuffled subset with duplicates is the full trace, gathered
    _same_trace(trs, {k: v[sub] for k, v in tr.items()}, "subset")
    # 1. tied to the real kernels
    np.testing.assert_array_equal(_bits(V), _bits(TC.oracle_V(scene, net, T, stride)))
    lo, hi = np.asarray(cfg["u_lo"], np.float32), np.asarray(cfg["u_hi"], np.float32)
    np.testing.assert_array_equal(_bits(tr["controls"]), _bits(np.clip(V, lo, hi)))
    np.testing.assert_array_equal(_bits(tr["states"][:, 0]), _bits(np.tile(np.asarray(cfg["start_state"], np.float32), (K, 1))))
    ref = TC.trace64(scene, net, T, stride)
    dec = ref["decided"]
    n_diff = int(np.sum(_bits(tr["costs"]) != _bits(res["costs"])))
    # 2. states against float64
    dev = np.abs(tr["states"].astype(np.float64) - TC.states64(scene, net, T, stride))
    # 3. the flag
    wrong = dec & (tr["first_crash"] != ref["first"])
    # 4. the fold
    fold = TC.fold_step_costs(tr["step_costs"])
    print("TRACE %s form=%s (%s): costs differ on %d of %d (decided: max rel %.1e); states max dev %.2e (TOL_STATE x%.1f) per component %s; %d decided, "
          "%d of them flagged, first_crash wrong on %d; fold differs on %d" % (
              "%s-%s-T%d-s%d" % case[:4], name, "exact" if exact else "re-associating", n_diff, K,
              float(np.where(dec, rel_err(tr["costs"], res["costs"]), 0.0).max()), dev.max(),
              TC.TOL_STATE / max(dev.max(), 1e-30), np.array2string(dev.max(axis=(0, 1)), precision=1), int(dec.sum()),
              int(np.sum(dec & (ref["first"] >= 0))), int(wrong.sum()), int(np.sum(_bits(fold) != _bits(tr["costs"])))))
    if exact:
        np.testing.assert_array_equal(_bits(tr["costs"]), _bits(res["costs"]))
    assert np.all(tr["step_costs"][:, 0] == 0.0)
    assert dev.max() <= TC.TOL_STATE
    assert not wrong.any(), (np.nonzero(wrong)[0][:8], tr["first_crash"][wrong][:8], ref["first"][wrong][:8])
    np.testing.assert_array_equal(_bits(fold), _bits(tr["costs"]))
    # 8. mppi_top_rollouts
    np.testing.assert_array_equal(top, np.argsort(-res["w"], kind="stable")[:17])


def _shipped_case():
    c = TC.CASES[0]
    return c, TC.problem(*c[:4])


def test_slide_and_set_control_seq_change_nothing():
    case, (cfg, U0, eps) = _shipped_case()
    sol = _solver(cfg, "row_exact", U0, eps)
    try:
        sol.compute_control(cfg["start_state"])
        ks = np.arange(0, K, 3)
        a = sol.trace_rollouts(ks)
        sol.slide_control_seq(1)
        b = sol.trace_rollouts(ks)
        sol.set_control_seq(np.zeros((cfg["T"], 2), np.float32))
        c = sol.trace_rollouts(ks)
        costs = sol.get_results()["costs"]
    finally:
        sol.close()
    _same_trace(a, b, "after slide")
    _same_trace(a, c, "after set_control_seq")
    np.testing.assert_array_equal(_bits(a["costs"]), _bits(costs[ks]))


def test_trace_waits_for_a_pending_solve():
    case, (cfg, U0, eps) = _shipped_case()
    st2 = np.array(cfg["start_state"], np.float32)
    st2[0] += 0.37
    st2[4] = 4.25
    sol = _solver(cfg, "row_exact", U0, eps)
    try:
        sol.compute_control(cfg["start_state"])
        first = sol.trace_rollouts(np.arange(K))
        sol.set_control_seq(U0)
        sol.set_noise(eps)
        sol.compute_control_async(st2)
        tr = sol.trace_rollouts(np.arange(K))   # no synchronize in between: the trace collects the pending solve
        costs = sol.get_results()["costs"]
    finally:
        sol.close()
    np.testing.assert_array_equal(_bits(tr["states"][:, 0]), _bits(np.tile(st2, (K, 1))))
    np.testing.assert_array_equal(_bits(tr["costs"]), _bits(costs))
    assert np.any(_bits(tr["costs"]) != _bits(first["costs"]))


def test_trace_is_the_last_iteration_of_two():
    scene, net, T, stride, _ = TC.CASES[0]
    cfg = TC.config(scene, net, T, stride, num_iters=2)
    eps = noise_for(cfg, 77)
    sol = _solver(cfg, "row_exact", warm_U(cfg), eps)
    try:
        sol.debug_capture_iterations(1)
        sol.compute_control(cfg["start_state"])
        its = sol.debug_get_iterations(with_V=True)
        tr = sol.trace_rollouts(np.arange(K))
        costs = sol.get_results()["costs"]
    finally:
        sol.close()
    np.testing.assert_array_equal(_bits(tr["costs"]), _bits(its["costs"][1]))
    np.testing.assert_array_equal(_bits(tr["costs"]), _bits(costs))
    assert np.any(_bits(its["costs"][0]) != _bits(its["costs"][1]))
    lo, hi = np.asarray(cfg["u_lo"], np.float32), np.asarray(cfg["u_hi"], np.float32)
    np.testing.assert_array_equal(_bits(tr["controls"]), _bits(np.clip(its["V"][1], lo, hi)))


def _snap(s):
    r = s.get_results()
    return dict(U=r["U"].copy(), costs=r["costs"].copy(), w=r["w"].copy())


def _armed_run(cfgs, trace_while_armed):
    """n handles (one: mppi_arm; two: mppi_arm_batch): solve, slide, [arm, trace while armed,] solve again from the next
    state.  Returns (traces, seconds each trace took, results of the second solve)."""
    sols = []
    try:
        for i, cfg in enumerate(cfgs):
            s = capi.Solver(cfg)
            s.seed(7 + i, 0)
            sols.append(s)
        states = [np.array(c["start_state"], np.float32) for c in cfgs]
        ks = np.arange(0, cfgs[0]["K"], cfgs[0]["K"] // 64).astype(np.int32)
        if len(sols) == 1:
            sols[0].compute_control(states[0])
        else:
            capi.compute_control_batch(sols, states)
        for s, c in zip(sols, cfgs):
            s.slide_control_seq(int(c["opt_stride"]))
        traces, secs = [], []
        if trace_while_armed:
            if len(sols) == 1:
                sols[0].arm(WAIT)
            else:
                capi.arm_batch(sols, WAIT)
            assert all(s.is_armed() for s in sols)
            for s in sols:
                t0 = time.perf_counter()
                traces.append(s.trace_rollouts(ks))
                secs.append(time.perf_counter() - t0)
            assert all(s.is_armed() for s in sols), "the trace disarmed the handle"
        else:
            traces = [s.trace_rollouts(ks) for s in sols]
        nxt = [st + np.float32(0.01) * np.arange(7, dtype=np.float32) for st in states]
        if len(sols) == 1:
            sols[0].compute_control(nxt[0])
        else:
            capi.compute_control_batch(sols, nxt)
        if trace_while_armed:
            assert sols[0].debug_launch_info() == (len(sols), 1), sols[0].debug_launch_info()
        return traces, secs, [_snap(s) for s in sols]
    finally:
        for s in sols:
            s.close()


@pytest.mark.parametrize("which", ["row_4096", "m44_pair_1920"])
def test_trace_while_armed(which):
    """The bound and the reasoning of test_applied_controls_while_armed: the trace of the LAST solve did not sit behind the gated
    kernels' deadline (WAIT), the handle stays armed, and the compute that opens the gate gives the bits of the run that was
    never armed or traced in between.  The un-armed reference run goes first (a gated kernel holds its CUs)."""
    if which == "row_4096":
        cfgs = [S.make_config(4096, 100, track="oval")]
    else:
        cfgs = [S.make_config(1920, 100, track="oval", layers=[6, 64, 64, 4], instance=i) for i in range(2)]
    want_tr, _, want = _armed_run(cfgs, False)
    got_tr, secs, got = _armed_run(cfgs, True)
    print("TRACE_ARMED %s: %s s per trace of 64 rollouts while armed (bound %.3f)" % (which, ["%.4f" % s for s in secs], WAIT / 2))
    for a, b in zip(got_tr, want_tr):
        _same_trace(a, b, "armed")
    assert max(secs) < WAIT / 2, secs
    for a, b in zip(got, want):
        for k in a:
            np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=k)


def test_refusals():
    case, (cfg, U0, eps) = _shipped_case()
    sol = _solver(cfg, "row_exact", U0, eps)
    try:
        for call in (lambda: sol.trace_rollouts([0]), lambda: sol.top_rollouts(1)):
            with pytest.raises(capi.MppiError) as e:
                call()
            assert e.value.status == capi.ERR_STATE
        sol.compute_control(cfg["start_state"])
        for bad in ([-1], [K], [3, K, 4]):
            with pytest.raises(capi.MppiError) as e:
                sol.trace_rollouts(bad)
            assert e.value.status == capi.ERR_INVALID
        L = sol.L
        assert L.mppi_trace_rollouts(sol.h, None, 1, None, None, None, None, None) == capi.ERR_INVALID
        assert L.mppi_trace_rollouts(sol.h, None, -1, None, None, None, None, None) == capi.ERR_INVALID
        assert L.mppi_trace_rollouts(sol.h, None, 0, None, None, None, None, None) == capi.OK
        assert L.mppi_top_rollouts(sol.h, K + 1, None) == capi.ERR_INVALID
        assert sol.trace_rollouts([])["states"].shape == (0, cfg["T"], 7)
        plain = sol.trace_rollouts([0, 9, K - 1])
        # a control cost on: the cost outputs are refused with the reason, the rest is served and is what it was
        sol.set_cost_params(dict(cfg["cost"], steering_coeff=0.7))
        with pytest.raises(capi.MppiError) as e:
            sol.trace_rollouts([0, 9, K - 1])
        assert e.value.status == capi.ERR_UNSUPPORTED and "control cost" in str(e.value)
        served = sol.trace_rollouts([0, 9, K - 1], with_costs=False)
    finally:
        sol.close()
    assert sorted(served) == ["controls", "first_crash", "states"]
    _same_trace(served, {k: plain[k] for k in served}, "control cost on")


def test_tracing_64_rollouts_takes_no_longer_than_one_generic_rollout_launch():
    """One bar against the parent's code on the same handle (6-32-32-32-4, K = 1920, T = 100): "valu_lds" is the parent's only
    kernel that serves every layer list.  Median of 5 after one warm-up of each."""
    cfg = S.make_config(1920, 100, track="oval", layers=[6, 32, 32, 32, 4])
    sol = capi.Solver(cfg)
    try:
        sol.set_rollout_variant("valu_lds")
        sol.seed(7, 0)
        sol.compute_control(cfg["start_state"])
        ks = np.arange(0, 1920, 30).astype(np.int32)
        assert ks.size == 64

        def med(fn):
            fn()
            t = []
            for _ in range(5):
                t0 = time.perf_counter()
                fn()
                t.append(time.perf_counter() - t0)
            return float(np.median(t))
        t_trace = med(lambda: sol.trace_rollouts(ks))
        t_roll = med(lambda: sol.rollout_only(cfg["start_state"]))
    finally:
        sol.close()
    print("TRACE_TIME 64 rollouts traced: %.3f ms; one rollout_only on valu_lds: %.3f ms" % (1e3 * t_trace, 1e3 * t_roll))
    assert t_trace <= t_roll


def test_host_selftest_calls_the_controller():
    """The host layer's traceRollouts / getSampledTrajectories run once in host_selftest, on a controller that exists only where
    a device does: here the program must have taken that path (the un-marked tests/test_host_layer.py accepts either)."""
    import os
    import subprocess
    import tempfile
    from autorally_amd import build as B
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    golden = os.path.join(root, "tests", "golden")
    exe = [p for p in B.build_host() if os.path.basename(p) == "host_selftest"][0]
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([exe, os.path.join(golden, "models", "autorally_nnet_09_12_2018.npz"),
                            os.path.join(root, "autorally_amd", "host", "launch", "path_integral_nn.launch"), tmp,
                            os.path.join(golden, "costmap_track_converter.npz")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "sampled trajectories: best rollout" in r.stdout and "host selftest OK" in r.stdout, r.stdout[-500:]
