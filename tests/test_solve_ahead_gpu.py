"""Solve-ahead (mppi_arm / mppi_arm_batch, csrc/abi_solve.hip): the next solve is enqueued gated and opened by the next compute
call with a NEW state every tick.  Every comparison is against a second handle making the same calls without arming, bit for bit.

The reference handle runs its whole sequence FIRST: a gated kernel holds the CUs it occupies until its gate opens, so a
reference solve enqueued between an arm and its compute would wait for the armed handle's deadline (and the armed solve would
then be called off instead of opened -- the path these tests exist to check)."""
import ctypes as C
import time

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import synthetic as S

pytestmark = pytest.mark.gpu

WAIT = 0.1  # the longest gate wait mppi_arm accepts: the Python calls between an arm and its compute stay far inside it


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1


def _solver(cfg, variant=None):
    s = capi.Solver(cfg)
    if variant:
        s.set_rollout_variant(variant)
    s.seed(7, 0)
    return s


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _snap(s):
    r = s.get_results()
    return dict(U=r["U"].copy(), costs=r["costs"].copy(), w=r["w"].copy(), traj_cost=np.float32(r["traj_cost"]),
                hist=s.get_control_hist().copy())


def _same(got, want, what):
    for k in ("U", "costs", "w", "hist"):
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg="%s: %s" % (what, k))
    assert _bits(got["traj_cost"]) == _bits(want["traj_cost"]), what


def _next_state(s, state, opt):
    ss, _ = s.nominal_traj(state)
    return ss[min(opt, ss.shape[0] - 1)].copy()


CASES = [
    ("row", 4096, 100, None, None, "row"),
    ("row_exact", 1920, 100, None, "row_exact", "row"),
    ("m44", 512, 100, [6, 64, 64, 4], None, "m44"),
    ("m44_deep", 1920, 100, [6, 64, 64, 64, 64, 4], None, "m44"),
    ("multi4_tree_gen", 16384, 64, None, None, "multi4_tree"),
]


def _cfg(K, T, layers):
    return S.make_config(K, T, track="oval", layers=layers) if layers else S.make_config(K, T, track="oval")


def _reference_run(cfg, variant, n):
    """n ticks of compute -> slide(opt) from the start state, the next state from the nominal trajectory: states and results"""
    ref = _solver(cfg, variant)
    opt = int(cfg["opt_stride"])
    state, states, res = cfg["start_state"].copy(), [], []
    for _ in range(n):
        states.append(state)
        ref.compute_control(state)
        res.append(_snap(ref))
        ref.slide_control_seq(opt)
        state = _next_state(ref, state, opt)
    ref.close()
    return states, res


@pytest.mark.parametrize("pattern", ["idle", "pending"])
@pytest.mark.parametrize("name,K,T,layers,variant,form", CASES, ids=[c[0] for c in CASES])
def test_armed_ticks_with_a_new_state_every_tick(name, K, T, layers, variant, form, pattern):
    """20 ticks, the state of each the nominal trajectory's state at the optimization stride of the one before.
    idle: arm -> compute -> slide; pending: compute_async -> arm -> synchronize -> slide -> compute_async ..."""
    cfg = _cfg(K, T, layers)
    n, opt = 20, int(cfg["opt_stride"])
    states, want = _reference_run(cfg, variant, n)
    a = _solver(cfg, variant)
    assert form in a.rollout_variant()
    if pattern == "idle":
        for i in range(n):
            if i > 0:
                a.arm(WAIT)
                assert a.is_armed()
            a.compute_control(states[i])
            assert not a.is_armed()
            _same(_snap(a), want[i], "%s tick %d" % (name, i))
            a.slide_control_seq(opt)
    else:
        a.compute_control_async(states[0])
        for i in range(n):
            if i + 1 < n:
                a.arm(WAIT)
                assert a.is_armed()
            a.synchronize()
            _same(_snap(a), want[i], "%s tick %d" % (name, i))  # costs / weights read while armed
            a.slide_control_seq(opt)
            if i + 1 < n:
                assert a.is_armed()
                a.compute_control_async(states[i + 1])
                assert not a.is_armed()
    a.close()


def test_armed_batch_with_two_states_and_varying_strides():
    """The two controllers of the reference's deployment (K = 1920, 6-32-32-4) in ONE gated launch (mppi_arm_batch +
    mppi_compute_control_batch): actual and predicted state differ every tick, the strides vary between 0, 1 and 2.
    30 ticks; then the batch armed in the other order: the batch call calls that off and solves unarmed."""
    cfgs = [S.make_config(1920, 100, track="oval", seed=5), S.make_config(1920, 100, track="oval", seed=6)]
    n, extra = 30, 2
    rng = np.random.RandomState(3)
    strides = [int(rng.choice([0, 1, 2])) for _ in range(n + extra)]

    def run(armed):
        sols = [capi.Solver(c) for c in cfgs]
        for s in sols:
            s.seed(int(s.cfg["seed"]), 0)
        actual = cfgs[0]["start_state"].copy()
        pred = actual.copy()
        pred[4] += 0.25
        out = []
        for i in range(n + extra):
            if armed and i > 0:
                capi.arm_batch(sols if i < n else sols[::-1], WAIT)
                assert all(s.is_armed() for s in sols)
            capi.compute_control_batch(sols, [actual, pred])
            assert not any(s.is_armed() for s in sols)
            out.append([_snap(s) for s in sols])
            st = strides[i]
            ssa, _ = sols[0].nominal_traj(actual)
            ssp, _ = sols[1].nominal_traj(pred)
            for s in sols:
                s.slide_control_seq(st)
            actual, pred = ssa[max(st, 1)].copy(), ssp[1].copy()
        for s in sols:
            s.close()
        return out

    want = run(False)
    got = run(True)
    for i in range(n + extra):
        for q in range(2):
            _same(got[i][q], want[i][q], "batch tick %d controller %d" % (i, q))


def _set_nn(s):
    th = np.ascontiguousarray(s.cfg["theta"], dtype=np.float32)
    s._ck(s.L.mppi_set_nn_params(s.h, th.ctypes.data_as(C.POINTER(C.c_float)), th.size))


SETTERS = {
    "nn_params": _set_nn,
    "update_model": lambda s: s.update_model(list(s.cfg["layers"]), _update_model_data(s.cfg)),
    "cost_params": lambda s: s.set_cost_params(dict(s.cfg["cost"], desired_speed=6.0)),
    "costmap_transform": lambda s: s.set_costmap_transform(s.cfg["r_c1"], s.cfg["r_c2"], s.cfg["trs"]),
    "costmap_channel": lambda s: s.set_costmap_channel(0, np.ascontiguousarray(s.cfg["map_rgba"][..., 0])),
    "control_limits": lambda s: s.set_control_limits((-0.9, -0.5), (0.9, 0.6)),
    "seed": lambda s: s.seed(11, 3),
    "set_noise": lambda s: s.set_noise(np.random.RandomState(4).standard_normal((s.K, s.T, 2)).astype(np.float32)),
    "generate_noise": lambda s: s.generate_noise(),
    "rollout_only": lambda s: s.rollout_only(s.cfg["start_state"]),
    "rollout_variant": lambda s: s.set_rollout_variant("auto"),
    "stage_timing_off": lambda s: s.enable_stage_timing(0),
    "capture_off": lambda s: s.debug_capture_iterations(0),
    "cost_raster": lambda s: s.debug_cost_raster(0.0, -10.0, 0.0, 10, 10, 20),
    "dynamics": lambda s: s.debug_dynamics(np.zeros((4, 7), np.float32), np.zeros((4, 2), np.float32)),
    "control_ticks": lambda s: s.control_ticks(s.cfg["start_state"], 1, 1),
}


def _update_model_data(cfg):
    """packed theta [W1|b1|W2|b2|..] -> the [W1|W2|..|b1|b2|..] layout of updateModel"""
    th, L = np.asarray(cfg["theta"], np.float32), list(cfg["layers"])
    ws, bs, off = [], [], 0
    for l in range(len(L) - 1):
        nw, nb = L[l] * L[l + 1], L[l + 1]
        ws.append(th[off:off + nw])
        bs.append(th[off + nw:off + nw + nb])
        off += nw + nb
    return np.concatenate(ws + bs)


IMPLICIT = [(k, 4096, 100) for k in SETTERS] + [(k, 16384, 64) for k in ("seed", "generate_noise", "cost_params", "rollout_only",
                                                                          "set_noise", "control_ticks")]


@pytest.mark.parametrize("setter,K,T", IMPLICIT, ids=["%s-K%d" % (s, K) for s, K, _ in IMPLICIT])
def test_every_setter_calls_the_armed_solve_off(setter, K, T):
    """arm, then a call that changes what the armed solve would compute: the handle is no longer armed, and that solve and the
    three after it (armed again) equal the never-armed handle's -- the generator stream went on where it was."""
    cfg = S.make_config(K, T, track="oval")
    opt = int(cfg["opt_stride"])

    def run(armed):
        s = _solver(cfg)
        state, out = cfg["start_state"].copy(), []
        for i in range(6):
            if armed and i > 0:
                s.arm(WAIT)
                assert s.is_armed()
            if i == 2:
                SETTERS[setter](s)
                assert not s.is_armed()
            s.compute_control(state)
            out.append(_snap(s))
            s.slide_control_seq(opt)
            state = _next_state(s, state, opt)
        s.close()
        return out

    want = run(False)
    got = run(True)
    for i in range(6):
        _same(got[i], want[i], "%s tick %d" % (setter, i))


@pytest.mark.parametrize("K,T", [(4096, 100), (16384, 64)])
def test_disarm_and_close_do_not_wait_for_the_deadline(K, T):
    cfg = S.make_config(K, T, track="oval")
    opt = int(cfg["opt_stride"])
    states, want = _reference_run(cfg, None, 3)
    a = _solver(cfg)
    a.compute_control(states[0])
    _same(_snap(a), want[0], "tick 0")
    a.slide_control_seq(opt)
    a.arm(WAIT)
    t0 = time.perf_counter()
    a.disarm()
    dt = time.perf_counter() - t0
    assert not a.is_armed()
    assert dt < 0.005, dt
    a.compute_control(states[1])  # behind the called-off solve, on the same stream
    _same(_snap(a), want[1], "after disarm")
    a.slide_control_seq(opt)
    a.arm(WAIT)
    t0 = time.perf_counter()
    a.close()
    assert time.perf_counter() - t0 < 0.05  # the called-off kernels end at once (poisoned), not at the deadline


def test_a_late_gate_solves_unarmed():
    """The gated kernels wait at most max_wait_s; a compute that comes later calls the expired solve off and solves unarmed."""
    cfg = S.make_config(4096, 100, track="oval")
    opt = int(cfg["opt_stride"])
    states, want = _reference_run(cfg, None, 3)
    a = _solver(cfg)
    a.compute_control(states[0])
    a.slide_control_seq(opt)
    a.arm(0.005)
    time.sleep(0.05)
    a.compute_control(states[1])
    got = _snap(a)
    assert np.all(np.isfinite(got["U"]))
    _same(got, want[1], "late gate")
    a.slide_control_seq(opt)
    a.arm(WAIT)
    a.compute_control(states[2])
    _same(_snap(a), want[2], "armed after the late gate")
    a.close()


def test_an_armed_solve_that_fails_leaves_the_host_copies_alone():
    """The armed solve's wait runs out of time (ERR_HIP): U and hist on the host are those from before the call, finite; once
    the lost work has drained the handle solves again from them, as a fresh handle given the same U / hist does."""
    cfg = S.make_config(4096, 100, track="oval")
    opt, st = int(cfg["opt_stride"]), cfg["start_state"]
    a = _solver(cfg)
    for i in range(3):
        if i:
            a.arm(WAIT)
        a.compute_control(st)
        a.slide_control_seq(opt)
    U0, h0 = a.get_control_seq().copy(), a.get_control_hist().copy()
    a.arm(WAIT)
    a.set_wait_timeout(1e-6)
    with pytest.raises(capi.MppiError) as e:
        a.compute_control(st)
    assert e.value.status == capi.ERR_HIP
    a.set_wait_timeout(30.0)
    np.testing.assert_array_equal(_bits(a.get_control_seq()), _bits(U0))
    np.testing.assert_array_equal(_bits(a.get_control_hist()), _bits(h0))
    assert np.all(np.isfinite(U0)) and np.all(np.isfinite(h0))
    deadline = time.perf_counter() + 5.0
    while True:
        try:
            a.seed(9, 0)
            break
        except capi.MppiError:
            assert time.perf_counter() < deadline
            time.sleep(0.001)
    ref = capi.Solver(cfg)
    ref.set_control_seq(U0)
    ref.set_control_hist(h0)
    ref.seed(9, 0)
    want = []
    for i in range(3):
        ref.compute_control(st)
        want.append(_snap(ref))
        ref.slide_control_seq(opt)
    ref.close()
    for i in range(3):
        a.arm(WAIT)
        a.compute_control(st)
        _same(_snap(a), want[i], "after the drain, tick %d" % i)
        a.slide_control_seq(opt)
    a.close()


def _bf_cfg(golden_dir):
    import os
    from autorally_amd import params as P
    W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    return S.make_config(2560, 100, track="oval", bf_W=W)


@pytest.mark.parametrize("case", ["num_iters", "basis_function", "quad"])
def test_forms_without_a_gated_form_are_unsupported(case, golden_dir):
    variant = None
    if case == "num_iters":
        cfg = S.make_config(1920, 100, track="oval", num_iters=2)
    elif case == "basis_function":
        cfg = _bf_cfg(golden_dir)
    else:
        cfg, variant = S.make_config(1920, 100, track="oval"), "quad"
    states, want = _reference_run(cfg, variant, 2)
    a = _solver(cfg, variant)
    a.compute_control(states[0])
    a.slide_control_seq(int(cfg["opt_stride"]))
    with pytest.raises(capi.MppiError) as e:
        a.arm(WAIT)
    assert e.value.status == capi.ERR_UNSUPPORTED
    assert not a.is_armed()
    a.compute_control(states[1])
    _same(_snap(a), want[1], case)
    a.close()


def test_applied_controls_while_armed():
    """mppi_get_applied_controls while armed: the last solve's, without waiting on the gated kernels."""
    cfg = S.make_config(4096, 100, track="oval")
    ref, a = _solver(cfg), _solver(cfg)
    st = cfg["start_state"]
    ref.compute_control(st)
    V = ref.get_applied_controls()
    ref.close()
    a.compute_control(st)
    a.slide_control_seq(int(cfg["opt_stride"]))
    a.arm(WAIT)
    t0 = time.perf_counter()
    got = a.get_applied_controls()
    assert time.perf_counter() - t0 < 0.05
    assert a.is_armed()
    np.testing.assert_array_equal(_bits(got), _bits(V))
    a.disarm()
    a.close()
