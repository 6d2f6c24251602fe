"""The "fleet16" rollout form (csrc/rollout_fleet16.hip): the wavefront, the image and the bits of "lds16" with the argument block
read from device memory, so that 2..64 handles of one layer list share ONE generator, ONE rollout and ONE tail launch per
iteration of mppi_compute_control_batch.  Whatever the set, every handle's results are bit for bit those of its own solve.
  1. bits: a fleet of 5 against every handle solved alone with "valu_lds" and with "lds16", one and two iterations;
  2. sizes: 2 and 64 share, 65 does not, 1 through the batch call and through mppi_compute_control;
  3. sets that fall back to handle-by-handle solves; a handle without parameters;
  4. the generator streams stay in step over ticks; a handle leaves and rejoins; two fleets alternate;
  5. no gated form, refusals, the trace, live updates;
  6. the every-rollout bar on one instance of a fleet;
  7. (timing) sharing the launches beats not sharing them in the same form.
Each case prints what it measured."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import params as P
from autorally_amd import synthetic as S
from tests import scenes as SC
from tests import test_lds16_gpu as L16
from tests.helpers import noise_for, warm_U
from tests.test_lds44_gpu import _results, _same_bits, _solver, _update_data

pytestmark = pytest.mark.gpu

U32 = np.uint32
V = "fleet16"
NETS = [[6, 5, 7, 4], [6, 32, 32, 4], [6, 64, 64, 64, 64, 4], [6, 33, 97, 66, 4], [6, 128, 128, 128, 4]]
KS = (192, 64, 4096, 1984, 64)   # the largest is not first; 64 and 1984 leave absent waves in the last workgroup
TS = (17, 2, 43, 60, 17)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _id(net):
    return "-".join(map(str, net))


def fleet_name(net):
    return "mfma16x16x4_fleet_l%d_w%d" % (len(net) - 2, max(net[1:-1]))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


def _close(sols):
    for s in sols:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 1
def _instance(i, net, K, T, iters):
    """Instance i of the mixed fleet: the ring, the oval or the ramp; its own state, weights, cost parameters, nu, gamma and
    limits; explicit noise (even i) or a seed.  One thing the instances share beside the layer list: the projective costmap
    transform and a control cost (the ramp has both), since one kernel instance serves the launch."""
    track = ("ring", "oval", "ramp")[i % 3]
    if track == "ramp":
        cfg = SC.ramp_config(K, T, layers=list(net), num_iters=iters)
        U0 = SC.ramp_U(cfg, seed=3 + i)
    else:
        cfg = S.make_config(K, T, layers=list(net), track=track, num_iters=iters)
        U0 = warm_U(cfg, seed=3 + i)
        r_c1, r_c2 = np.array(cfg["r_c1"], np.float32), np.array(cfg["r_c2"], np.float32)
        r_c1[2], r_c2[2] = np.float32(2e-5), np.float32(-1e-5)
        cfg.update(r_c1=r_c1, r_c2=r_c2, cost=dict(cfg["cost"], steering_coeff=0.3 + 0.1 * i, throttle_coeff=0.2))
    st = np.array(cfg["start_state"], np.float32)
    st[4] += np.float32(0.05 * i)
    st[6] += np.float32(0.01 * i)
    cost = dict(cfg["cost"], desired_speed=6.0 + 0.5 * i, l1_cost=(i == 1))
    cfg.update(theta=np.asarray(cfg["theta"], np.float32) * np.float32(1.0 + 0.02 * i), start_state=st, cost=cost,
               nu=(0.275 + 0.01 * i, 0.3 - 0.01 * i), gamma=0.15 + 0.01 * i, u_lo=(-0.99 + 0.02 * i, -0.99), u_hi=(0.99, 0.65 - 0.03 * i))
    kw = dict(eps=noise_for(cfg, 100 + i)) if i % 2 == 0 else dict(seed=700 + i)
    return cfg, U0, kw


@functools.lru_cache(maxsize=None)
def _mixed_fleet(net, iters):
    """The five instances and every one of them solved ALONE with "valu_lds" and with "lds16" (computed once, not changed)."""
    insts = [_instance(i, list(net), K, T, iters) for i, (K, T) in enumerate(zip(KS, TS))]
    alone = {}
    for v in ("valu_lds", "lds16"):
        alone[v] = []
        for cfg, U0, kw in insts:
            sol = _solver(cfg, v, U0, **kw)
            try:
                sol.compute_control(cfg["start_state"])
                alone[v].append(_results(sol))
            finally:
                sol.close()
    return insts, alone


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("net", NETS, ids=_id)
def test_a_fleet_of_five_has_every_handles_own_bits(net, iters):
    insts, alone = _mixed_fleet(tuple(net), iters)
    sols = [_solver(cfg, V, U0, **kw) for cfg, U0, kw in insts]
    try:
        capi.compute_control_batch(sols, [cfg["start_state"] for cfg, _, _ in insts])
        infos = [s.debug_launch_info() for s in sols]
        assert infos == [(5, 0)] * 5, infos
        for i, s in enumerate(sols):
            got = _results(s)
            assert got["variant"] == fleet_name(net), got["variant"]
            for v in ("valu_lds", "lds16"):
                assert alone[v][i]["variant"] != got["variant"]
                _same_bits(got, alone[v][i], "%s iters=%d instance %d vs %s alone" % (_id(net), iters, i, v))
            assert np.all(np.isfinite(got["costs"]))
        print("FLEET16 bits net=%s iters=%d: 5 instances K=%s T=%s in launches of %s, each equal to valu_lds and lds16 alone" % (
            _id(net), iters, KS, TS, infos[0]))
    finally:
        _close(sols)


# ------------------------------------------------------------------------------------------------------------------ 2
SMALL = (6, 32, 32, 4)


@functools.lru_cache(maxsize=None)
def _many(n=65, K=64, T=17):
    """n instances on one oval (affine transform, no control cost): distinct states, seeds and cost parameters; each solved alone
    with "lds16"."""
    base = S.make_config(K, T, layers=list(SMALL), track="oval")
    U0 = warm_U(base)
    cfgs = []
    for i in range(n):
        st = np.array(base["start_state"], np.float32)
        st[0] += np.float32(0.3 * i)
        st[4] += np.float32(0.02 * i)
        cfgs.append(dict(base, start_state=st, cost=dict(base["cost"], desired_speed=5.0 + 0.1 * i)))
    alone = []
    for i, cfg in enumerate(cfgs):
        sol = _solver(cfg, "lds16", U0, seed=2000 + i)
        try:
            sol.compute_control(cfg["start_state"])
            alone.append(_results(sol))
        finally:
            sol.close()
    assert len({a["costs"].tobytes() for a in alone}) == n, "the instances are distinct"
    return cfgs, U0, alone


@pytest.mark.parametrize("n,shared", [(2, True), (64, True), (65, False)])
def test_fleet_sizes(n, shared):
    cfgs, U0, alone = _many()
    sols = [_solver(cfgs[i], V, U0, seed=2000 + i) for i in range(n)]
    try:
        capi.compute_control_batch(sols, [cfgs[i]["start_state"] for i in range(n)])
        infos = {s.debug_launch_info() for s in sols}
        print("FLEET16 sizes n=%d: launch info %s" % (n, infos))
        assert infos == {(n if shared else 1, 0)}
        for i, s in enumerate(sols):
            _same_bits(_results(s), alone[i], "n=%d instance %d" % (n, i))
    finally:
        _close(sols)


def test_one_handle_through_the_batch_call_and_alone():
    cfgs, U0, alone = _many()
    for how in ("batch", "single"):
        sol = _solver(cfgs[3], V, U0, seed=2003)
        try:
            if how == "batch":
                capi.compute_control_batch([sol], [cfgs[3]["start_state"]])
            else:
                sol.compute_control(cfgs[3]["start_state"])
            assert sol.debug_launch_info() == (1, 0)
            got = _results(sol)
            assert got["variant"] == fleet_name(SMALL)
            _same_bits(got, alone[3], how)
            # ... and mppi_rollout_only: the costs of the next draws, as "lds16" alone has them
            twin = _solver(cfgs[3], "lds16", U0, seed=2003)
            try:
                twin.compute_control(cfgs[3]["start_state"])
                np.testing.assert_array_equal(sol.rollout_only(cfgs[3]["start_state"]).view(U32),
                                              twin.rollout_only(cfgs[3]["start_state"]).view(U32))
            finally:
                twin.close()
        finally:
            sol.close()


# ------------------------------------------------------------------------------------------------------------------ 3
FALLBACKS = ["auto", "another_list", "another_num_iters", "K_8192", "projective", "stage_timing"]


@pytest.mark.parametrize("what", FALLBACKS)
def test_sets_that_fall_back_to_handle_by_handle_solves(what):
    """Three handles, the middle one out of line: no launch is shared (instances = 1 on every handle) and every handle has the
    bits of its own solve."""
    net, K, T = [6, 16, 24, 4], 192, 17
    cfgs = [S.make_config(K, T, layers=list(net), track="oval") for _ in range(3)]
    for i, cfg in enumerate(cfgs):
        st = np.array(cfg["start_state"], np.float32)
        st[4] += np.float32(0.1 * i)
        cfg["start_state"] = st
    variants = [V, V, V]
    if what == "auto":
        variants[1] = "auto"
    elif what == "another_list":
        cfgs[1] = S.make_config(K, T, layers=[6, 16, 25, 4], track="oval")
    elif what == "another_num_iters":
        cfgs[1] = dict(cfgs[1], num_iters=2)
    elif what == "K_8192":
        cfgs[1] = S.make_config(8192, T, layers=list(net), track="oval")
    elif what == "projective":
        r_c1 = np.array(cfgs[1]["r_c1"], np.float32)
        r_c1[2] = np.float32(2e-5)
        cfgs[1] = dict(cfgs[1], r_c1=r_c1)

    def make():
        sols = [_solver(cfg, v, warm_U(cfg), seed=40 + i) for i, (cfg, v) in enumerate(zip(cfgs, variants))]
        if what == "stage_timing":
            sols[1].enable_stage_timing(1)
        return sols
    fleet, solo = make(), make()
    try:
        capi.compute_control_batch(fleet, [cfg["start_state"] for cfg in cfgs])
        for s, cfg in zip(solo, cfgs):
            s.compute_control(cfg["start_state"])
        infos = [s.debug_launch_info() for s in fleet]
        print("FLEET16 fallback %s: launch info %s" % (what, infos))
        assert infos == [(1, 0)] * 3
        for i, (a, b) in enumerate(zip(fleet, solo)):
            _same_bits(_results(a), _results(b), "%s handle %d" % (what, i))
        if what not in ("auto", "K_8192"):   # (the control: without the odd one out the other two do share)
            capi.compute_control_batch([fleet[0], fleet[2]], [cfgs[0]["start_state"], cfgs[2]["start_state"]])
            assert fleet[0].debug_launch_info() == (2, 0)
    finally:
        _close(fleet + solo)


def _bare_solver(cfg):
    """A handle with its costmap and cost parameters but WITHOUT network parameters."""
    import ctypes as C
    sol = capi.Solver.__new__(capi.Solver)
    sol.L, sol.cfg, sol.K, sol.T, sol.num_iters, sol.h = capi.lib(), cfg, int(cfg["K"]), int(cfg["T"]), 1, C.c_void_p()
    c = capi.make_config_struct(cfg, 0)
    assert sol.L.mppi_create(C.byref(c), C.byref(sol.h)) == capi.OK
    m = np.ascontiguousarray(cfg["map_rgba"], np.float32)
    fp = lambda a: np.ascontiguousarray(a, np.float32).ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    sol._ck(sol.L.mppi_set_costmap(sol.h, m.shape[1], m.shape[0], fp(m), fp(cfg["r_c1"]), fp(cfg["r_c2"]), fp(cfg["trs"])))
    p = capi.make_cost_struct(cfg["cost"])
    sol._ck(sol.L.mppi_set_cost_params(sol.h, C.byref(p)))
    return sol


def test_a_handle_without_parameters_fails_the_call_and_moves_nobody():
    net, K, T = [6, 16, 24, 4], 192, 17
    cfg = S.make_config(K, T, layers=list(net), track="oval")
    U0, st = warm_U(cfg), cfg["start_state"]
    fleet = [_solver(cfg, V, U0, seed=60 + i) for i in range(2)]
    twins = [_solver(cfg, V, U0, seed=60 + i) for i in range(2)]
    bare = _bare_solver(cfg)
    try:
        bare.set_rollout_variant(V)
        with pytest.raises(capi.MppiError) as e:
            capi.compute_control_batch(fleet + [bare], [st] * 3)
        print("FLEET16 unready handle: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_STATE and "mppi_set_nn_params" in str(e.value)
        assert [s.debug_launch_info() for s in fleet] == [(0, 0)] * 2, "nothing was enqueued for the other handles"
        capi.compute_control_batch(fleet, [st] * 2)
        capi.compute_control_batch(twins, [st] * 2)
        for i in range(2):
            assert fleet[i].debug_launch_info() == (2, 0)
            _same_bits(_results(fleet[i]), _results(twins[i]), "after the failed call, handle %d" % i)
    finally:
        _close(fleet + twins + [bare])


# ------------------------------------------------------------------------------------------------------------------ 4
def _stream_state(sol):
    return sol.get_control_seq(), sol.get_control_hist(), sol.generate_noise()


def test_generator_streams_stay_in_step():
    """Ticks of the fleet against the same ticks driven handle by handle on twins forced to "lds16": the nominal sequence, the
    control history and the generator's NEXT draws are bit-equal per handle -- after 4 shared ticks, after one handle left, solved
    alone and rejoined, and after two different fleets of three alternated on the device."""
    net, T = [6, 32, 32, 4], 17
    Ks = (64, 192, 128, 64, 256, 192)
    cfgs = []
    for i, K in enumerate(Ks):
        cfg = S.make_config(K, T, layers=list(net), track="oval", opt_stride=1)
        st = np.array(cfg["start_state"], np.float32)
        st[4] += np.float32(0.1 * i)
        cfg["start_state"] = st
        cfgs.append(cfg)
    states = [cfg["start_state"] for cfg in cfgs]
    fleet = [_solver(cfg, V, warm_U(cfg), seed=300 + i) for i, cfg in enumerate(cfgs)]
    twins = [_solver(cfg, "lds16", warm_U(cfg), seed=300 + i) for i, cfg in enumerate(cfgs)]

    def twin_ticks(idx, n):
        for i in idx:
            for _ in range(n):
                twins[i].compute_control(states[i])
                twins[i].slide_control_seq(1)

    def check(tag):
        # (generate_noise draws: both sides draw, so they stay comparable afterwards)
        for i, (a, b) in enumerate(zip(fleet, twins)):
            for x, y, what in zip(_stream_state(a), _stream_state(b), ("U", "hist", "next draws")):
                np.testing.assert_array_equal(x.view(U32), y.view(U32), err_msg="%s: handle %d %s" % (tag, i, what))
    try:
        capi.control_ticks_batch(fleet, states, 4, 1)
        assert {s.debug_launch_info() for s in fleet} == {(6, 0)}
        twin_ticks(range(6), 4)
        check("4 ticks")
        assert not np.array_equal(fleet[0].get_control_seq(), warm_U(cfgs[0]))
        # one handle leaves, solves alone, rejoins
        fleet[2].compute_control(states[2])
        fleet[2].slide_control_seq(1)
        assert fleet[2].debug_launch_info() == (1, 0)
        twin_ticks([2], 1)
        capi.control_ticks_batch(fleet, states, 1, 1)
        assert {s.debug_launch_info() for s in fleet} == {(6, 0)}
        twin_ticks(range(6), 1)
        check("left and rejoined")
        # two different fleets alternate on the device
        A, B = fleet[:3], fleet[3:]
        for _ in range(4):
            capi.compute_control_batch(A, states[:3], blocking=False)
            capi.compute_control_batch(B, states[3:], blocking=False)
            for s in fleet:
                s.synchronize()
                s.slide_control_seq(1)
        assert {s.debug_launch_info() for s in fleet} == {(3, 0)}
        twin_ticks(range(6), 4)
        check("two fleets alternating")
        print("FLEET16 streams: 6 handles K=%s, 9 ticks in fleets of 6 / 1 / 3 + 3: U, hist and the next draws equal to lds16 twins" % (Ks,))
    finally:
        _close(fleet + twins)


# ------------------------------------------------------------------------------------------------------------------ 5
def test_no_gated_form():
    cfg = S.make_config(192, 17, layers=[6, 48, 48, 4], track="oval", opt_stride=1)
    st = cfg["start_state"]
    sols = [_solver(cfg, V, warm_U(cfg), seed=77 + i) for i in range(2)]
    twins = [_solver(cfg, V, warm_U(cfg), seed=77 + i) for i in range(2)]
    try:
        for group in (sols, twins):
            capi.control_ticks_batch(group, [st, st], 1, 1)
        with pytest.raises(capi.MppiError) as e:
            sols[0].arm(0.1)
        print("FLEET16 arm: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_UNSUPPORTED
        with pytest.raises(capi.MppiError) as e:
            capi.arm_batch(sols, 0.1)
        print("FLEET16 arm_batch: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_UNSUPPORTED
        for s in sols:
            assert not s.is_armed() and s.debug_launch_info() == (2, 0), "nothing was enqueued"
        for group in (sols, twins):
            capi.compute_control_batch(group, [st, st])
        for a, b in zip(sols, twins):
            _same_bits(_results(a), _results(b), "after the refused arm")
    finally:
        _close(sols + twins)


def test_refusals_are_those_of_lds16(golden_dir):
    bf_W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    too_big = [6, 128, 128, 128, 128, 4]
    cases = [("bf", S.make_config(256, 20, track="oval", bf_W=bf_W)),
             ("6-129-4", S.make_config(256, 20, layers=[6, 129, 4], track="oval")),
             ("6-4", S.make_config(256, 20, layers=[6, 4], track="oval")),
             (_id(too_big), S.make_config(256, 20, layers=too_big, track="oval"))]
    for tag, cfg in cases:
        sol = capi.Solver(cfg)
        try:
            sol.seed(5, 0)
            before = sol.rollout_variant()
            sol.compute_control(cfg["start_state"])
            first = sol.get_results()
            status = {}
            for v in ("lds16", V):
                with pytest.raises(capi.MppiError) as e:
                    sol.set_rollout_variant(v)
                status[v] = e.value.status
                assert v in str(e.value), str(e.value)
                if v == V:
                    print("FLEET16 refusal %s: status %d, %s" % (tag, e.value.status, e.value))
            assert status[V] == status["lds16"] == capi.ERR_UNSUPPORTED, (tag, status)
            assert sol.rollout_variant() == before
            sol.reset_controls()
            sol.seed(5, 0)
            sol.compute_control(cfg["start_state"])
            _same_bits(sol.get_results(), first, tag, keys=("costs", "w", "U"))
        finally:
            sol.close()
    cfg = S.make_config(256, 20, layers=[6, 32, 32, 4], track="oval")
    sol = capi.Solver(cfg)
    try:
        auto = sol.rollout_variant()
        sol.set_rollout_variant(V)
        assert sol.rollout_variant() == fleet_name([6, 32, 32, 4])
        sol.set_rollout_variant("auto")
        assert sol.rollout_variant() == auto and "fleet" not in auto  # the automatic choice has not changed
    finally:
        sol.close()


def test_the_trace_after_a_fleet_solve_is_the_trace_after_the_handles_own():
    net = [6, 33, 97, 66, 4]
    cfgs = [S.make_config(256, 23, layers=list(net), track="oval") for _ in range(2)]
    cfgs[1]["start_state"] = np.array(cfgs[1]["start_state"], np.float32) + np.array([0, 0, 0, 0, 0.3, 0, 0], np.float32)
    fleet = [_solver(cfg, V, warm_U(cfg), seed=31 + i) for i, cfg in enumerate(cfgs)]
    solo = [_solver(cfg, V, warm_U(cfg), seed=31 + i) for i, cfg in enumerate(cfgs)]
    try:
        capi.compute_control_batch(fleet, [cfg["start_state"] for cfg in cfgs])
        assert fleet[0].debug_launch_info() == (2, 0)
        ks = np.arange(256)
        for a, b, cfg in zip(fleet, solo, cfgs):
            b.compute_control(cfg["start_state"])
            ta, tb = a.trace_rollouts(ks), b.trace_rollouts(ks)
            assert set(ta) == set(tb)
            for key in ta:
                np.testing.assert_array_equal(np.asarray(ta[key]), np.asarray(tb[key]), err_msg=key)
            np.testing.assert_array_equal(ta["costs"].view(U32), a.get_results()["costs"].view(U32))
    finally:
        _close(fleet + solo)


def test_live_updates_follow_the_generic_kernel():
    """Between two fleet solves: mppi_update_model, mppi_set_cost_params, mppi_set_costmap_transform and a variant switch away and
    back -- every solve of every handle equals the same sequence on "valu_lds" alone, bit for bit."""
    net = [6, 33, 97, 66, 4]
    cfgs = [S.make_config(192, 17, layers=list(net), track="oval") for _ in range(2)]
    cfgs[1]["start_state"] = np.array(cfgs[1]["start_state"], np.float32) + np.array([0, 0, 0, 0, 0.3, 0, 0], np.float32)
    states = [cfg["start_state"] for cfg in cfgs]
    U0 = warm_U(cfgs[0])
    eps = [noise_for(cfg, 99 + i) for i, cfg in enumerate(cfgs)]
    _, theta2 = P.synthetic_model(list(net), seed=11)
    cost2 = dict(cfgs[0]["cost"], desired_speed=7.5, speed_coeff=3.0, crash_coeff=8000.0)
    r_c1, r_c2, trs = (np.array(cfgs[0][k], np.float32) for k in ("r_c1", "r_c2", "trs"))
    trs2 = trs.copy()
    trs2[0] += np.float32(0.02)   # some texels of the rollouts' track move
    trs2[1] -= np.float32(0.015)
    fleet = [_solver(cfg, V, U0, eps[i]) for i, cfg in enumerate(cfgs)]
    twins = [_solver(cfg, "valu_lds", U0, eps[i]) for i, cfg in enumerate(cfgs)]
    infos, prev = [], None

    def step(tag):
        nonlocal prev
        for group in (fleet, twins):
            for i, s in enumerate(group):
                s.set_control_seq(U0)
                s.set_noise(eps[i])
        capi.compute_control_batch(fleet, states)
        infos.append(fleet[0].debug_launch_info())
        now = []
        for i, (a, b) in enumerate(zip(fleet, twins)):
            b.compute_control(states[i])
            now.append(_results(a))
            _same_bits(now[-1], _results(b), "%s handle %d" % (tag, i))
        changed = prev is None or not np.array_equal(prev[0]["costs"], now[0]["costs"])
        prev = now
        return changed
    try:
        step("first")
        for s in fleet + twins:
            s.update_model(list(net), _update_data(list(net), np.asarray(theta2, np.float32)))
        assert step("update_model")
        for s in fleet + twins:
            s.set_cost_params(cost2)
        assert step("set_cost_params")
        for s in fleet + twins:
            s.set_costmap_transform(r_c1, r_c2, trs2)
        assert step("set_costmap_transform")
        fleet[1].set_rollout_variant("auto")
        step("one handle on auto")
        fleet[1].set_rollout_variant(V)
        step("and back")
        print("FLEET16 live updates: 6 solves equal to valu_lds, launch info %s" % infos)
        assert infos == [(2, 0)] * 4 + [(1, 0), (2, 0)], infos
    finally:
        _close(fleet + twins)


# ------------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("net", [[6, 16, 24, 4], [6, 33, 97, 66, 4]], ids=_id)
def test_every_rollout_of_one_instance_of_a_fleet(net, monkeypatch):
    """The _hold of tests/test_lds16_gpu.py -- V bit-equal to the mode-1 oracle, every cost within TOL64 of ref64 and TOL_MODE of the
    oracle, no allowance -- on the ramp at K = 1984, T = 60, solved as instance 3 of a fleet of five."""
    def fleet_solve(cfg, variant, U0, eps):
        others = [SC.ramp_config(K, T, layers=list(net)) for K, T in ((192, 17), (64, 60), (4096, 17), (64, 17))]
        sols = [_solver(c, V, SC.ramp_U(c, seed=i), seed=90 + i) for i, c in enumerate(others)]
        sols.insert(3, _solver(cfg, V, U0, eps))
        try:
            capi.compute_control_batch(sols, [s.cfg["start_state"] for s in sols])
            assert sols[3].debug_launch_info() == (5, 0)
            return _results(sols[3])
        finally:
            _close(sols)
    monkeypatch.setattr(L16, "_solve", fleet_solve)
    monkeypatch.setattr(L16, "lds16_name", fleet_name)
    L16._hold("fleet16 instance 3 of 5", net, 1984, 60)


# ------------------------------------------------------------------------------------------------------------------ 7
@pytest.mark.timing
def test_sharing_the_launches_beats_not_sharing_them():
    """16 handles, K = 1920, T = 100, generator noise: the median tick of mppi_control_ticks_batch over 200 ticks after 20 warm
    ones (tools/fleet_time.py), for 6-32-32-4 and 6-64-64-64-64-4 -- (a) "fleet16" is faster than (b) the same handles forced to
    "lds16", handle by handle.  (c) "auto" is printed, not held to anything.
    Measured (MI355X): see DESIGN.md 4.19."""
    spec = importlib.util.spec_from_file_location("fleet_time", os.path.join(ROOT, "tools", "fleet_time.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    rows = ft.table([[6, 32, 32, 4], [6, 64, 64, 64, 64, 4]])
    for row in rows:
        assert row["a_instances"] == 16 and row["b_instances"] == 1 and row["c_instances"] == 1, row
        assert row["a_ms"] < row["b_ms"], row
