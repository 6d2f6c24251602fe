"""The two controllers of a tick in ONE rollout launch for the 64-wide form ("m44": 6-64-64-4, 6-64x4-4) and the free-form one
("lds44", forced, one layer list): mppi_compute_control_batch, mppi_arm_batch, mppi_control_ticks_batch.

A batched instance runs the group body of its single launch with its own argument block, so every comparison is bit for bit
(uint32) against two handles solved one by one; mppi_debug_launch_info says whether the launch was shared (instances == 2) and
gated.  Shapes: two different K per pair (the smaller instance's workgroups return early), T = 37 (longer than the 16-step rings,
no multiple of 4), distinct costmaps, seeds and start states per handle, optimization stride 1 and 2.

Where a test arms, the stand-alone reference runs its whole sequence first: a gated kernel holds its CUs until its gate opens."""
import functools
import os

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import params as P
from autorally_amd import synthetic as S

pytestmark = pytest.mark.gpu

WAIT = 0.1
KS, T = (128, 320), 37
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (layer list, variant forced by name or None, "m44" / "lds" as it shows in mppi_rollout_variant)
NETS = {
    "m44_64x2": ([6, 64, 64, 4], None, "m44_split"),
    "m44_64x4": ([6, 64, 64, 64, 64, 4], None, "m44_split"),
    "lds44_32x3": ([6, 32, 32, 32, 4], "lds44", "mfma4x4x1_lds"),
    "lds44_16_24": ([6, 16, 24, 4], "lds44", "mfma4x4x1_lds"),
}
CTRL_COST = dict(P.DEFAULT_COST, steering_coeff=0.3, throttle_coeff=0.25)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1


@functools.lru_cache(maxsize=None)
def _model(net):
    layers = NETS[net][0]
    if net == "lds44_16_24":  # the model the reference's training pipeline wrote
        return P.load_model_npz(os.path.join(GOLDEN, "models", "trained_writer_6_16_24_4.npz"))
    return P.synthetic_model(layers, seed=4)


@functools.lru_cache(maxsize=None)
def _cfg(net, i, K=None, T_=T, opt=1, ctrl=False, projective=False):
    """Controller i of a pair: its own K, costmap instance (rotated, shifted track: another start state too) and seed"""
    layers, theta = _model(net)
    assert list(layers) == NETS[net][0]
    cfg = S.make_config(K or KS[i % 2], T_, layers=list(layers), theta=theta, track="oval", instance=i, seed=77 + i, opt_stride=opt,
                        cost=dict(CTRL_COST) if ctrl else dict(P.DEFAULT_COST))
    if projective:  # third components of the columns non-trivial (costs.cu:373-377 divides by w)
        cfg["r_c1"] = (cfg["r_c1"][0], cfg["r_c1"][1], 0.001)
        cfg["r_c2"] = (cfg["r_c2"][0], cfg["r_c2"][1], -0.002)
    return cfg


def _solver(cfg, variant):
    s = capi.Solver(cfg)
    if variant:
        s.set_rollout_variant(variant)
    return s


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _snap(s):
    r = s.get_results()
    return dict(U=r["U"].copy(), costs=r["costs"].copy(), w=r["w"].copy(), traj_cost=np.float32(r["traj_cost"]),
                hist=s.get_control_hist().copy(), V=s.get_applied_controls().copy())


def _same(got, want, what):
    for k in ("U", "hist", "costs", "w", "V"):
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg="%s: %s" % (what, k))
    assert _bits(got["traj_cost"]) == _bits(want["traj_cost"]), what


def _state(cfg, tick):
    return cfg["start_state"] + np.float32(0.01 * tick) * np.arange(7, dtype=np.float32)


def _stride(tick):
    return 1 if tick % 3 else 2


def _noise(cfg, seed):
    return np.random.RandomState(seed).standard_normal((cfg["K"], cfg["T"], 2)).astype(np.float32)


def _launch_infos(sols):
    return [s.debug_launch_info() for s in sols]


def _close(sols):
    for s in sols:
        s.close()


def _alone(cfgs, variants, n_ticks, explicit_from=None):
    """Every controller on a handle of its own, solved one by one: [tick][controller] snapshots.  Tick t solves from
    _state(cfg, t), then slides by _stride(t); from tick explicit_from on with explicit noise."""
    out = [[None] * len(cfgs) for _ in range(n_ticks)]
    for i, (cfg, v) in enumerate(zip(cfgs, variants)):
        s = _solver(cfg, v)
        for t in range(n_ticks):
            if explicit_from is not None and t >= explicit_from:
                s.set_noise(_noise(cfg, 900 + 10 * t + i))
            s.compute_control(_state(cfg, t))
            assert s.debug_launch_info() == (1, 0)
            out[t][i] = _snap(s)
            s.slide_control_seq(_stride(t))
        s.close()
    return out


@functools.lru_cache(maxsize=None)
def _alone_pair(net, opt, n_ticks, explicit_from=None):
    return _alone([_cfg(net, 0, opt=opt), _cfg(net, 1, opt=opt)], [NETS[net][1]] * 2, n_ticks, explicit_from)


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("opt", [1, 2])
@pytest.mark.parametrize("net", list(NETS))
def test_the_pair_shares_a_launch_and_equals_stand_alone_handles(net, opt):
    """Five ticks of solve + slide in generator mode (blocking and asynchronous batch calls alternate, the states change every
    tick), then two ticks with explicit noise: U, hist, costs, weights, V and the trajectory cost are those of two handles
    solved one by one, and every batched solve was ONE rollout launch for both (not gated)."""
    n, explicit_from = 7, 5
    want = _alone_pair(net, opt, n, explicit_from)
    cfgs = [_cfg(net, 0, opt=opt), _cfg(net, 1, opt=opt)]
    bat = [_solver(c, NETS[net][1]) for c in cfgs]
    try:
        assert all(NETS[net][2] in s.rollout_variant() for s in bat)
        assert _launch_infos(bat) == [(0, 0), (0, 0)]  # no solve yet
        for t in range(n):
            if t >= explicit_from:
                for i, (s, c) in enumerate(zip(bat, cfgs)):
                    s.set_noise(_noise(c, 900 + 10 * t + i))
            capi.compute_control_batch(bat, [_state(c, t) for c in cfgs], blocking=(t % 2 == 0))
            assert _launch_infos(bat) == [(2, 0), (2, 0)], "tick %d" % t
            for i, s in enumerate(bat):
                _same(_snap(s), want[t][i], "%s opt %d tick %d controller %d" % (net, opt, t, i))
                s.slide_control_seq(_stride(t))
    finally:
        _close(bat)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("state_kind", ["finite", "inf_x", "nan_speed"])
@pytest.mark.parametrize("partner", ["control_cost", "projective"])
@pytest.mark.parametrize("net", ["m44_64x2", "lds44_32x3"])
def test_a_mixed_pair_equals_the_single_solves_also_for_non_finite_states(net, partner, state_kind):
    """control_cost: a controller without control cost beside one with it is still ONE launch, of the kernel with the term: the
    term of the instance without it is 0 x du x (u - du) / nu^2 = +0 whatever its STATE is (its controls are finite).
    projective: an affine costmap transform beside a projective one -- the superset would divide by a w computed from the
    state, different bits for a non-finite one -- falls back to per-handle solves.  Same bits as the single solves either way."""
    a = _cfg(net, 0)
    b = _cfg(net, 1, ctrl=True, projective=(partner == "projective"))
    sa, sb = a["start_state"].copy(), b["start_state"].copy()
    if state_kind == "inf_x":
        sa[0] = np.inf
    elif state_kind == "nan_speed":
        sa[4] = np.nan
    v = NETS[net][1]
    ref, bat = [_solver(a, v), _solver(b, v)], [_solver(a, v), _solver(b, v)]
    try:
        outs = []
        for pair, batched in ((ref, False), (bat, True)):
            try:
                if batched:
                    capi.compute_control_batch(pair, [sa, sb])
                else:
                    pair[0].compute_control(sa)
                    pair[1].compute_control(sb)
                outs.append([_snap(s) for s in pair])
            except capi.MppiError as e:
                outs.append(("error", e.status))
        if isinstance(outs[0], tuple) or isinstance(outs[1], tuple):
            assert outs[0] == outs[1], outs  # the same loud failure both ways
        else:
            want_n = 2 if partner == "control_cost" else 1
            assert _launch_infos(bat) == [(want_n, 0), (want_n, 0)]
            for i in range(2):
                _same(outs[1][i], outs[0][i], "%s %s %s controller %d" % (net, partner, state_kind, i))
    finally:
        _close(ref + bat)


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("scenario", ["plain", "disarm_one", "setter", "other_order"])
@pytest.mark.parametrize("net", ["m44_64x4", "lds44_16_24"])
def test_the_armed_pair_is_one_gated_launch(net, scenario):
    """mppi_arm_batch + mppi_compute_control_batch with a new state every tick, six ticks: after arming both handles are armed
    and their next rollout is ONE gated launch for both; results are those of the unarmed stand-alone loop.  At tick 3, after
    arming -- disarm_one: mppi_disarm on ONE handle calls the launch off for both; setter: so does a setter on one of them;
    other_order: armed with the handles in the other order, the batch call calls that off and solves.  Same bits in every case."""
    n, opt = 6, 1
    want = _alone_pair(net, opt, n)
    cfgs = [_cfg(net, 0, opt=opt), _cfg(net, 1, opt=opt)]
    bat = [_solver(c, NETS[net][1]) for c in cfgs]
    try:
        for t in range(n):
            opened = t > 0
            if t > 0:
                special = scenario != "plain" and t == 3
                capi.arm_batch(bat[::-1] if (special and scenario == "other_order") else bat, WAIT)
                assert all(s.is_armed() for s in bat)
                assert _launch_infos(bat) == [(2, 1), (2, 1)], "tick %d" % t
                if special and scenario == "disarm_one":
                    bat[1].disarm()
                    assert not any(s.is_armed() for s in bat)
                elif special and scenario == "setter":
                    bat[0].set_cost_params(dict(cfgs[0]["cost"]))
                    assert not any(s.is_armed() for s in bat)
                opened = not special
            capi.compute_control_batch(bat, [_state(c, t) for c in cfgs])
            assert not any(s.is_armed() for s in bat)
            assert _launch_infos(bat) == [(2, 1 if opened else 0)] * 2, "tick %d" % t
            for i, s in enumerate(bat):
                _same(_snap(s), want[t][i], "%s %s tick %d controller %d" % (net, scenario, t, i))
                s.slide_control_seq(_stride(t))
    finally:
        _close(bat)


# ------------------------------------------------------------------------------------------------------------------ 4
def test_control_ticks_batch_on_an_m44_pair_equals_the_call_by_call_loop():
    net, opt, n = "m44_64x4", 2, 4
    cfgs = [_cfg(net, 0, opt=opt), _cfg(net, 1, opt=opt)]
    states = [c["start_state"] for c in cfgs]
    ref, bat = [_solver(c, None) for c in cfgs], [_solver(c, None) for c in cfgs]
    try:
        for s, st in zip(ref, states):
            for _ in range(n):
                s.compute_control(st)
                s.slide_control_seq(opt)
        capi.control_ticks_batch(bat, states, n, opt)
        assert _launch_infos(bat) == [(2, 0), (2, 0)]
        for r, b in zip(ref, bat):
            np.testing.assert_array_equal(_bits(b.get_control_seq()), _bits(r.get_control_seq()))
            np.testing.assert_array_equal(_bits(b.get_control_hist()), _bits(r.get_control_hist()))
        for s, st in zip(ref, states):
            s.compute_control(st)
        capi.compute_control_batch(bat, states)
        for i, (r, b) in enumerate(zip(ref, bat)):
            _same(_snap(b), _snap(r), "the solve after the ticks, controller %d" % i)
    finally:
        _close(ref + bat)


# ------------------------------------------------------------------------------------------------------------------ 5
def _fallback_cases():
    return {
        # name: [(net, K, T, variant)]
        "lds44_different_lists": [("lds44_32x3", 128, T, "lds44"), ("lds44_16_24", 320, T, "lds44")],
        "m44_beside_lds44": [("m44_64x2", 128, T, None), ("lds44_32x3", 320, T, "lds44")],
        "m44_chain": [("m44_64x2", 128, T, "m44_chain"), ("m44_64x2", 320, T, "m44_chain")],
        "three_m44": [("m44_64x2", 128, T, None), ("m44_64x2", 320, T, None), ("m44_64x2", 128, T, None)],
        "more_groups_than_cus": [("m44_64x2", 1920, 20, None), ("m44_64x2", 3968, 20, None)],
    }


@pytest.mark.parametrize("case", list(_fallback_cases()))
def test_batches_without_a_shared_launch_fall_back_to_per_handle_solves(case):
    """Different layer lists, different forms, the one-chain form (no batched kernel), three handles (the batched kernels serve
    the pair of a tick), more groups than CUs: every handle is solved by a launch of its own, with its own bits."""
    spec = _fallback_cases()[case]
    cfgs = [_cfg(net, i, K=K, T_=T_) for i, (net, K, T_, _) in enumerate(spec)]
    variants = [v for _, _, _, v in spec]
    n = 2
    want = _alone(cfgs, variants, n)
    bat = [_solver(c, v) for c, v in zip(cfgs, variants)]
    try:
        for t in range(n):
            capi.compute_control_batch(bat, [_state(c, t) for c in cfgs])
            assert _launch_infos(bat) == [(1, 0)] * len(bat)
            for i, s in enumerate(bat):
                _same(_snap(s), want[t][i], "%s tick %d controller %d" % (case, t, i))
                s.slide_control_seq(_stride(t))
    finally:
        _close(bat)
