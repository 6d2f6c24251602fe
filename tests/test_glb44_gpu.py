"""The "glb44" rollout form (csrc/rollout_glb44.hip): every layer list mppi_create accepts for the network model -- hidden widths
up to 256, an image of any size -- on "lds128"'s group (512 threads per 16 rollouts, four dynamics waves on v_mfma_f32_4x4x1, the
riders, the gate, the pair launch), the head of the image and the first R quads of its stream resident in LDS, the other quads read
from the image in global memory.  The form is EXACT: its arithmetic is the oracle's mode 1, its bits are those of "valu_lds", of
"lds128" and of "glb16", for every R ("glb44_r<N>").
  1. every rollout of every layer list against ref64 and the mode-1 oracle on the flip-free ramp (tests/scenes.py);
  2. bit-identity with "valu_lds" (the widest lists: with "glb16"): ring, oval and ramp, explicit noise and the generator, two
     iterations;
  3. the seam between resident and streamed quads at every kind of quad, against "lds128", "glb16" and "glb44_r0";
  4. a -inf yaw rate on ragged lists (a padded neuron's activation is SET to 0, in every half);
  5. live updates follow "glb16" bit for bit;
  6. the armed loop and chained control ticks equal the plain loop;
  7. two handles of one list and one cap share a launch, gated or not; different lists or caps are solved one by one;
  8. refusals, names, "auto", the trace;
  9. not slower than "glb16" at K = 1920, T = 100 on 6-128-128-128-4.
Each case prints what it measured.

The references of 1. are computed on the host and the mode-1 oracle is held to ref64 there BEFORE the GPU result is looked at
(tests/test_glb16_gpu.py: _references, shared with that file): with the synthetic weights of tests/scenes.py (gentle_model) every
(list, shape) below passes that check, so no (list, scene, seed) had to be replaced."""
import os
from unittest import mock

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import params as P
from autorally_amd import synthetic as S
from tests import branch_cases as BC
from tests import edge_cases as EC
from tests.helpers import noise_for, oracle_mode_for, rel_err, warm_U
from tests.scenes import TOL64, TOL_MODE
from tests.test_glb16_gpu import _references, _scene
from tests.test_glb44_pack import AHEAD, glb44_packer, halves, head_quads, layer_quads, resident_quads, stream_quads  # noqa: F401 (a fixture)
from tests.test_lds44_gpu import _results, _same_bits, _solve, _solver, _update_data

pytestmark = pytest.mark.gpu

U32 = np.uint32
V = "glb44"
DEEP8 = [6, 20, 70, 9, 130, 33, 65, 4]
W128X3 = [6, 128, 128, 128, 4]
W128X4 = [6, 128, 128, 128, 128, 4]
# three halves with one neuron in the third; four halves; a partial quad in the third input set in front of four halves; one
# half in front of three; four sets into one half; ragged four halves and sets; the largest two-layer list; 4 and 2 halves; one
# set in front of four halves; eight entries; two halves with an image beyond the LDS (twice); a fully resident list
NETS = [[6, 129, 4], [6, 193, 4], [6, 129, 193, 4], [6, 6, 192, 4], [6, 256, 7, 4], [6, 200, 256, 4], [6, 256, 256, 4], [6, 197, 67, 4],
        [6, 16, 256, 4], DEEP8, W128X3, W128X4, [6, 33, 97, 66, 4]]
SHAPES = [(64, 17), (1984, 2), (1984, 60)]
EXTRA_LISTS = {"129": [6, 129, 4], "200-256": [6, 200, 256, 4]}  # names for tests/edge_cases.py, while this file runs
SHARED = 34928  # bytes of m44_group.hpp's shared state in front of the image (tests/test_glb44_pack.py checks the rule with it)


def _id(net):
    return "-".join(map(str, net))


def glb44_name(net):
    return "mfma4x4x1_glb_l%d_w%d" % (len(net) - 2, max(net[1:-1]))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    with mock.patch.dict(BC.NET_LAYERS, EXTRA_LISTS):
        yield


# ------------------------------------------------------------------------------------------------------------------ 1
def _hold(tag, net, K, T, variant=V):
    """The every-rollout bar of tests/test_glb16_gpu.py: the name, V bit-equal to the mode-1 oracle, EVERY cost within TOL64 of
    ref64 and TOL_MODE of the oracle, on costs that differ from rollout to rollout, no crash flag, no count allowance."""
    cfg, U0, eps, costs_o, V_o, costs_r = _references(tuple(net), K, T, True)
    sol = _solver(cfg, variant, U0, eps)
    try:
        sol.compute_control(cfg["start_state"])
        got = _results(sol)
    finally:
        sol.close()
    assert got["variant"] == glb44_name(net), got["variant"]
    assert oracle_mode_for(got["variant"]) == 1
    assert len(np.unique(got["costs"])) > K // 2, "the rollouts of this case are not distinct"
    np.testing.assert_array_equal(got["V"].view(U32), V_o.view(U32))
    eo, e64 = rel_err(got["costs"], costs_o), rel_err(got["costs"], costs_r)
    ko, k64 = int(np.argmax(eo)), int(np.argmax(e64))
    print("GLB44 %s net=%s K=%d T=%d: oracle max %.2e (k=%d), %d of %d costs bit-equal to the oracle, %d distinct; ref64 max %.2e (k=%d, margin x%.1f)" % (
        tag, _id(net), K, T, eo[ko], ko, int(np.sum(got["costs"].view(U32) == costs_o.view(U32))), K, len(np.unique(got["costs"])),
        e64[k64], k64, TOL64 / max(e64[k64], 1e-30)))
    assert float(e64[k64]) <= TOL64, ("ref64", k64, float(e64[k64]), int(np.sum(e64 > TOL64)))
    assert float(eo[ko]) <= TOL_MODE, ("oracle mode 1", ko, float(eo[ko]), int(np.sum(eo > TOL_MODE)))
    return cfg, got


@pytest.mark.parametrize("K,T", SHAPES)
@pytest.mark.parametrize("net", NETS, ids=_id)
def test_every_rollout_of_every_layer_list(net, K, T):
    _hold("every", net, K, T)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("net,other", [([6, 129, 4], "valu_lds"), ([6, 193, 4], "valu_lds"), ([6, 197, 67, 4], "valu_lds"), (DEEP8, "valu_lds"),
                                       ([6, 256, 256, 4], "glb16"), (W128X4, "glb16")], ids=lambda x: _id(x) if isinstance(x, list) else x)
def test_bit_identical_to_the_generic_kernel(net, other):
    """Costs, weights, V, U and the trajectory cost of "glb44" are those of "valu_lds" as uint32: on the ring and the oval
    (crashes, thresholds) and on the ramp, with explicit noise and with the generator's draws (the in-kernel noise wave against
    the stand-alone generator), with two iterations.  K = 256, T = 13.  The generic kernel is too slow for the widest lists here:
    those are compared with "glb16", which tests/test_glb16_gpu.py holds to "valu_lds"."""
    for track in ("ring", "oval", "ramp"):
        cfg, U0 = _scene(track, net, num_iters=2)
        eps = noise_for(cfg, 4321)
        for mode, kw in (("explicit", dict(eps=eps)), ("generator", dict(seed=97))):
            got = _solve(cfg, V, U0, **kw)
            assert got["variant"] == glb44_name(net)
            ref = _solve(cfg, other, U0, **kw)
            assert ref["variant"] != got["variant"]
            _same_bits(got, ref, "%s %s %s vs %s" % (_id(net), track, mode, other))
        print("GLB44 bits net=%s %s iters=2: equal to %s; costs %.4g .. %.4g, %d distinct" % (
            _id(net), track, other, float(got["costs"].min()), float(got["costs"].max()), len(np.unique(got["costs"]))))
        assert np.all(np.isfinite(got["costs"]))


# ------------------------------------------------------------------------------------------------------------------ 3
def seam_caps(net):
    """Caps N ("glb44_r<N>": quads below N resident) that end R at every kind of quad of the stream: 0 and 1; the first and the
    last quad of every layer; between two halves' quads of one k-quad (the first, the second and the last k-quad); at every set
    boundary (k-quad 16 / 32 / 48) and one quad to either side; on every layer boundary; inside the output layer; all of the
    stream with and without the zero quads; one below the uncapped R."""
    lq, n_w = layer_quads(net), len(net) - 1
    caps, b = {0, 1}, 0
    for j in range(1, n_w):
        H = halves(net[j + 1]) if j < n_w - 1 else 1
        nq = lq[j] // H
        caps |= {b, b + 1, b + H, b + H + 1, b + lq[j] - 1, b + lq[j]}
        if H > 1:
            caps |= {b + lq[j] - H + 1}
        for s in range(1, 4):
            if 16 * s < nq:
                caps |= {b + 16 * s * H - 1, b + 16 * s * H, b + 16 * s * H + 1}
        if j == n_w - 1:
            caps |= {b + nq // 2, b + nq // 2 + 1}
        b += lq[j]
    assert b + AHEAD == stream_quads(net)
    r = resident_quads(net, SHARED)
    caps |= {b + AHEAD - 1, b + AHEAD, r - 1, r}
    return sorted(c for c in caps if 0 <= c <= r)


@pytest.mark.parametrize("net,other", [([6, 33, 97, 66, 4], "lds128"), ([6, 128, 128, 4], "lds128"), ([6, 200, 256, 4], "glb16")],
                         ids=lambda x: _id(x) if isinstance(x, list) else x)
def test_the_seam_at_every_kind_of_quad(net, other):
    """K = 256, T = 13 on the oval: "glb44", "glb44_r0" and "glb44_r<N>" for every N of seam_caps equal the other form bit for bit."""
    cfg, U0 = _scene("oval", net)
    eps = noise_for(cfg, 77)
    ref, full = _solve(cfg, other, U0, eps), _solve(cfg, V, U0, eps)
    assert ref["variant"] != full["variant"] == glb44_name(net)
    _same_bits(full, ref, "%s glb44 vs %s" % (_id(net), other))
    caps = seam_caps(net)
    r = resident_quads(net, SHARED)
    assert (r == stream_quads(net)) == (other == "lds128"), "a list lds128 serves is fully resident without a cap"
    assert caps[0] == 0 and caps[-1] == r and r - 1 in caps
    for n in caps:
        got = _solve(cfg, "glb44_r%d" % n, U0, eps)
        assert got["variant"] == glb44_name(net)
        _same_bits(got, ref, "%s glb44_r%d vs %s" % (_id(net), n, other))
    print("GLB44 seam net=%s: R = %d of %d quads; %d caps %s equal to %s and glb44" % (_id(net), r, stream_quads(net), len(caps), caps, other))


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("K", EC.START_KS)
@pytest.mark.parametrize("name", list(EXTRA_LISTS))
def test_a_minus_inf_yaw_rate_on_ragged_lists(name, K):
    """tests/edge_cases.py's start state "yaw_rate_minus_inf" on 6-129-4 (one neuron in the third half) and 6-200-256-4 (eight in
    the fourth): the zero weights of a neuron that does not exist times -inf are NaN; its activation is SET to 0, in every half.
    The bar is edge_cases.hold_start_state's: the mode-1 oracle's costs, V bit-equal, U behind ref64's tail stages."""
    cfg, U0, eps, state = EC.start_state_problem(name, K, "yaw_rate_minus_inf")
    for variant in (V, "glb44_r1"):
        sol = _solver(cfg, variant, U0, eps, hist=EC.START_HIST)
        try:
            sol.compute_control(state)
            got = _results(sol)
        finally:
            sol.close()
        EC.hold_start_state(variant, name, K, "yaw_rate_minus_inf", got, glb44_name(EXTRA_LISTS[name]))


# ------------------------------------------------------------------------------------------------------------------ 5
def test_live_updates_follow_glb16():
    """A solve after each of mppi_set_nn_params, mppi_update_model and a variant switch away and back on 6-128-128-128-4: the image
    follows the model -- every solve equals the same sequence on "glb16" bit for bit."""
    net = W128X3
    cfg, U0 = _scene("oval", net, K=256, T=20)
    eps = noise_for(cfg, 99)
    _, theta2 = P.synthetic_model(list(net), seed=11)
    _, theta3 = P.synthetic_model(list(net), seed=12)
    trace = {}
    for variant in (V, "glb16"):
        sol = _solver(cfg, variant, U0, eps)
        out = []

        def solve():
            sol.set_control_seq(U0)
            sol.set_noise(eps)
            sol.compute_control(cfg["start_state"])
            out.append(_results(sol))
        try:
            solve()
            sol.set_nn_params(np.asarray(theta3, np.float32))
            solve()
            sol.update_model(list(net), _update_data(list(net), np.asarray(theta2, np.float32)))
            solve()
            sol.set_rollout_variant("glb16" if variant == V else V)
            sol.set_rollout_variant(variant)
            solve()
        finally:
            sol.close()
        trace[variant] = out
    names = [o["variant"] for o in trace[V]]
    assert names == [glb44_name(net)] * 4, names
    for i, (a, b) in enumerate(zip(trace[V], trace["glb16"])):
        _same_bits(a, b, "%s after update %d" % (_id(net), i))
    for i in range(1, 3):  # every update changed the solve
        assert not np.array_equal(trace[V][i]["costs"], trace[V][i - 1]["costs"]), i
    print("GLB44 live updates net=%s: 4 solves equal to glb16, names %s" % (_id(net), names))


# ------------------------------------------------------------------------------------------------------------------ 6
N_TICKS = 6


def _tick_loop(cfg, variant, armed, n=N_TICKS):
    """n ticks with a new state every tick (the nominal trajectory's next state); armed: mppi_arm before every compute."""
    sol = capi.Solver(cfg)
    out = []
    try:
        sol.set_rollout_variant(variant)
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
@pytest.mark.parametrize("net", [W128X3, [6, 200, 256, 4]], ids=_id)
def test_armed_loop_equals_the_unarmed_loop(net, K):
    cfg = S.make_config(K, 20, layers=list(net), track="oval", opt_stride=1)
    a, b = _tick_loop(cfg, V, True), _tick_loop(cfg, V, False)
    assert len(a) == len(b) == N_TICKS + 1
    for i, (x, y) in enumerate(zip(a, b)):
        _same_bits(x, y, "%s tick %d" % (_id(net), i), keys=("costs", "w", "U"))
    assert not np.array_equal(a[0]["U"], a[N_TICKS - 1]["U"])
    print("GLB44 armed loop net=%s K=%d: %d armed ticks and the solve after a disarm equal the unarmed loop" % (_id(net), K, N_TICKS))


@pytest.mark.parametrize("K", [64, 1920])
@pytest.mark.parametrize("net", [W128X3, [6, 200, 256, 4]], ids=_id)
def test_chained_control_ticks_equal_the_unchained_loop(net, K):
    """mppi_control_ticks with a new state every tick: chained (every solve but the first armed one tick ahead), unchained, and
    the same ticks call by call."""
    cfg = S.make_config(K, 20, layers=list(net), track="oval", opt_stride=1)
    st, opt, n = cfg["start_state"], 1, N_TICKS
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
            assert sol.rollout_variant() == glb44_name(net)
            res.append((sol.get_control_seq(), sol.get_control_hist()))
            sol.compute_control(st)
            res[-1] += (sol.get_results(),)
        for U, hist, r in res[1:]:
            np.testing.assert_array_equal(res[0][0].view(U32), U.view(U32))
            np.testing.assert_array_equal(res[0][1].view(U32), hist.view(U32))
            _same_bits(res[0][2], r, "after the ticks", keys=("costs", "w", "U"))
        assert np.all(np.isfinite(res[0][2]["U"]))
        print("GLB44 chained ticks net=%s K=%d: %d chained ticks equal the unchained and the call-by-call loop" % (_id(net), K, n))
    finally:
        for sol in sols:
            sol.close()


# ------------------------------------------------------------------------------------------------------------------ 7
CTRL_COST = dict(P.DEFAULT_COST, steering_coeff=0.3, throttle_coeff=0.25)


def _pair(nets, K=1920, T=20):
    """Two controllers: their own costmap instance, cost parameters (the second with a control cost) and seed"""
    return [S.make_config(K, T, layers=list(net), track="oval", opt_stride=1, instance=i, seed=77 + i,
                          cost=dict(CTRL_COST) if i else dict(P.DEFAULT_COST)) for i, net in enumerate(nets)]


@pytest.mark.parametrize("armed", [False, True], ids=["plain", "armed"])
@pytest.mark.parametrize("net", [W128X3, [6, 200, 256, 4]], ids=_id)
def test_two_handles_of_one_list_share_a_launch(net, armed):
    """mppi_compute_control_batch on two handles forced to "glb44" with the same layer list and cap, K = 1920, different costs
    (one with a control cost) and seeds: ONE rollout launch, gated when armed by mppi_arm_batch, and each handle's bits are those
    of its own single solve."""
    cfgs = _pair((net, net))
    solo = [_solve(cfg, V, warm_U(cfg), seed=500 + i) for i, cfg in enumerate(cfgs)]  # first: a gated kernel holds its CUs
    sols = []
    try:
        for i, cfg in enumerate(cfgs):
            sols.append(_solver(cfg, V, warm_U(cfg), seed=500 + i))
        if armed:
            capi.arm_batch(sols, 0.1)
            assert all(s.is_armed() for s in sols)
            assert [s.debug_launch_info() for s in sols] == [(2, 1), (2, 1)]
        capi.compute_control_batch(sols, [cfg["start_state"] for cfg in cfgs])
        assert not any(s.is_armed() for s in sols)
        infos = [s.debug_launch_info() for s in sols]
        print("GLB44 batch net=%s armed=%s: launch info %s" % (_id(net), armed, infos))
        assert infos == [(2, 1 if armed else 0)] * 2
        for i, s in enumerate(sols):
            got = _results(s)
            assert got["variant"] == glb44_name(net)
            _same_bits(got, solo[i], "instance %d armed=%s" % (i, armed))
    finally:
        for s in sols:
            s.close()


@pytest.mark.parametrize("what", ["lists", "caps"])
def test_two_handles_of_different_lists_or_caps_are_solved_one_by_one(what):
    nets = (W128X3, [6, 128, 128, 64, 4]) if what == "lists" else (W128X3, W128X3)
    variants = (V, V) if what == "lists" else (V, "glb44_r5")
    cfgs = _pair(nets)
    solo = [_solve(cfg, v, warm_U(cfg), seed=500 + i) for i, (cfg, v) in enumerate(zip(cfgs, variants))]
    sols = []
    try:
        for i, (cfg, v) in enumerate(zip(cfgs, variants)):
            sols.append(_solver(cfg, v, warm_U(cfg), seed=500 + i))
        capi.compute_control_batch(sols, [cfg["start_state"] for cfg in cfgs])
        infos = [s.debug_launch_info() for s in sols]
        print("GLB44 batch of two %s: launch info %s" % (what, infos))
        assert infos == [(1, 0), (1, 0)]
        for i, s in enumerate(sols):
            got = _results(s)
            assert got["variant"] == glb44_name(nets[i])
            _same_bits(got, solo[i], "instance %d" % i)
    finally:
        for s in sols:
            s.close()


# ------------------------------------------------------------------------------------------------------------------ 8
def test_refusals_leave_the_handle_as_it_was(golden_dir):
    bf_W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    cases = [("bf", S.make_config(256, 20, track="oval", bf_W=bf_W), V, capi.ERR_UNSUPPORTED, "glb44"),
             ("6-4", S.make_config(256, 20, layers=[6, 4], track="oval"), V, capi.ERR_UNSUPPORTED, "glb44"),
             ("6-4", S.make_config(256, 20, layers=[6, 4], track="oval"), "glb44_r0", capi.ERR_UNSUPPORTED, "glb44")]
    wide = S.make_config(256, 20, layers=[6, 129, 4], track="oval")
    cases += [("malformed", wide, name, capi.ERR_INVALID, "unknown variant")
              for name in ("glb44_", "glb44_r", "glb44_rx", "glb44x", "glb44_r-1", "glb44_r1x", "glb44_r 1", "glb44r1", "glb44_R1", "glb44_r+1")]
    for tag, cfg, name, status, text in cases:
        sol = capi.Solver(cfg)
        try:
            sol.seed(5, 0)
            before = sol.rollout_variant()
            sol.compute_control(cfg["start_state"])
            first = sol.get_results()
            with pytest.raises(capi.MppiError) as e:
                sol.set_rollout_variant(name)
            print("GLB44 refusal %s %r: status %d, %s" % (tag, name, e.value.status, e.value))
            assert e.value.status == status, (tag, name, e.value.status)
            assert text in str(e.value), str(e.value)
            assert sol.rollout_variant() == before
            sol.reset_controls()
            sol.seed(5, 0)
            sol.compute_control(cfg["start_state"])
            _same_bits(sol.get_results(), first, tag, keys=("costs", "w", "U"))
        finally:
            sol.close()


def test_names_and_auto_afterwards():
    for net in ([6, 129, 4], [6, 200, 256, 4], DEEP8, [6, 64, 64, 4]):
        sol = capi.Solver(S.make_config(256, 20, layers=net, track="oval"))
        try:
            auto = sol.rollout_variant()
            candidates = sol.form_candidates()
            for name in (V, "glb44_r0", "glb44_r000012", "glb44_r999999999"):
                sol.set_rollout_variant(name)
                assert sol.rollout_variant() == glb44_name(net)
                assert "m44" not in sol.rollout_variant() and "_tree" not in sol.rollout_variant()
                assert oracle_mode_for(sol.rollout_variant()) == 1
            sol.set_rollout_variant("auto")
            assert sol.rollout_variant() == auto  # the automatic choice has not changed
            assert sol.form_candidates() == candidates
            print("GLB44 names net=%s: %s, auto %s" % (_id(net), glb44_name(net), auto))
        finally:
            sol.close()
    assert glb44_name([6, 200, 256, 4]) == "mfma4x4x1_glb_l2_w256" and glb44_name(DEEP8) == "mfma4x4x1_glb_l6_w130"


def test_the_trace_of_a_solve_has_its_costs():
    net = [6, 200, 256, 4]
    cfg = S.make_config(256, 23, layers=list(net), track="oval")
    sol = _solver(cfg, V, warm_U(cfg), seed=31)
    try:
        sol.compute_control(cfg["start_state"])
        got = sol.get_results()
        tr = sol.trace_rollouts(np.arange(cfg["K"]))
        same = int(np.sum(tr["costs"].view(U32) == got["costs"].view(U32)))
        print("GLB44 trace net=%s: %d of %d traced costs bit-equal to the solve's, %d rollouts crash" % (
            _id(net), same, cfg["K"], int(np.sum(tr["first_crash"] >= 0))))
        np.testing.assert_array_equal(tr["costs"].view(U32), got["costs"].view(U32))
        assert sol.rollout_variant() == glb44_name(net)
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------------------------ 9
def test_not_slower_than_glb16():
    """6-128-128-128-4, K = 1920, T = 100: the median rollout stage (the kernel's own dispatch time, every 2nd solve timed) of 20
    timed solves per form, the forms alternating in blocks inside one process.  The wide lists are rows of tools/glb44_table.py,
    not assertions."""
    cfg = S.make_config(1920, 100, layers=list(W128X3), track="oval")
    st = cfg["start_state"]
    sols = {}
    try:
        for v in (V, "glb16"):
            sols[v] = capi.Solver(cfg)
            sols[v].set_rollout_variant(v)
            for _ in range(3):  # code objects loaded, every buffer touched
                sols[v].compute_control(st)
        samples = {v: [] for v in sols}
        for block in range(4):
            for v, sol in sols.items():
                for _ in range(5):
                    sol.enable_stage_timing(2)
                    sol.reset_stage_times()
                    for _ in range(2):
                        sol.compute_control(st)
                        sol.slide_control_seq(1)
                    t = sol.get_stage_times()
                    sol.enable_stage_timing(0)
                    assert t["n_solves"] == 1, t
                    samples[v].append(1e3 * t["rollout_ms"])
        med = {v: float(np.median(x)) for v, x in samples.items()}
        print("GLB44 speed net=%s K=1920 T=100: glb44 %.1f us, glb16 %.1f us, ratio %.2f (20 samples each)" % (
            _id(W128X3), med[V], med["glb16"], med["glb16"] / med[V]))
        assert med[V] <= med["glb16"], med
    finally:
        for sol in sols.values():
            sol.close()
