"""The "fleet_multi4" rollout form (csrc/rollout_fleet_multi.hip): the workgroup of "multi4_tree_gen" -- four dynamics waves with
every weight in registers, the riders on the side, eps from the stand-alone generator -- with the argument block read from device
memory, so that 2..64 handles of one standard network share ONE generator, ONE rollout and ONE tail launch per iteration of
mppi_compute_control_batch.  The yardstick is existing code: every handle's results are bit for bit those of a twin forced to
"multi4_tree_gen" and solved alone.
  1. bits: a mixed fleet of 5 on each of the three shapes, one and two iterations;
  2. sizes: 2 and 64 share, 65 does not, 1 through the batch call and through mppi_compute_control;
  3. sets that fall back to handle-by-handle solves;
  4. the generator streams stay in step over ticks; a handle leaves and rejoins; two fleets alternate;
  5. refusals, no gated form, a handle without parameters;
  6. the trace and a live model update on a member of a fleet;
  7. the every-rollout bar (tests/test_every_rollout_gpu.py: _hold, the bound of "multi4_tree") on one instance of a shared launch;
  8. (timing) the fleet's tick beats "fleet16"'s on the same handles.
Shapes: T = 17 wraps the 16-step rings, K = 64 is one workgroup, mixed K makes whole workgroups leave early.
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
from tests import test_every_rollout_gpu as ER
from tests.helpers import noise_for, warm_U
from tests.test_fleet16_gpu import _bare_solver
from tests.test_lds44_gpu import _results, _same_bits, _solver, _update_data

pytestmark = pytest.mark.gpu

U32 = np.uint32
V = "fleet_multi4"
SOLO = "multi4_tree_gen"   # the yardstick: existing code
NETS = [[6, 32, 32, 4], [6, 32, 32, 32, 32, 4], [6, 64, 64, 4]]
KS = (192, 64, 128, 192, 64)   # the largest is not alone and not only first: workgroups x = 1, 2 leave early in three instances
T = 17
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _id(net):
    return "-".join(map(str, net))


def fleet_name(net):
    return "mfma16x16x4_h%d_l%d_fleet_multi4_tree_gen" % (net[1], len(net) - 2)


def solo_name(net):
    return "mfma16x16x4_h%d_l%d_multi4_tree_gen" % (net[1], len(net) - 2)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


def _close(sols):
    for s in sols:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 1
def _instance(i, net, K, iters):
    """Instance i of the mixed fleet: its own state, model scale, seed, warm U, cost parameters, nu, gamma and control limits;
    instance 2 on another costmap (the ring), instance 3 with explicit noise.  What the instances share beside the shape: the
    affine costmap transform and no control cost (one pair per launch, csrc/abi_solve.hip: fleet_together)."""
    cfg = S.make_config(K, T, layers=list(net), track="ring" if i == 2 else "oval", num_iters=iters)
    U0 = warm_U(cfg, seed=3 + i)
    st = np.array(cfg["start_state"], np.float32)
    st[4] += np.float32(0.05 * i)
    st[6] += np.float32(0.01 * i)
    cost = dict(cfg["cost"], desired_speed=6.0 + 0.5 * i, speed_coeff=4.25 + 0.25 * i, l1_cost=(i == 1))
    cfg.update(theta=np.asarray(cfg["theta"], np.float32) * np.float32(1.0 + 0.02 * i), start_state=st, cost=cost,
               nu=(0.275 + 0.01 * i, 0.3 - 0.01 * i), gamma=0.15 + 0.01 * i, u_lo=(-0.99 + 0.02 * i, -0.99), u_hi=(0.99, 0.65 - 0.03 * i))
    kw = dict(eps=noise_for(cfg, 100 + i)) if i == 3 else dict(seed=700 + i)
    return cfg, U0, kw


@functools.lru_cache(maxsize=None)
def _mixed_fleet(net, iters):
    """The five instances and every one of them solved ALONE with "multi4_tree_gen" (computed once, not changed)."""
    insts = [_instance(i, list(net), K, iters) for i, K in enumerate(KS)]
    alone = []
    for cfg, U0, kw in insts:
        sol = _solver(cfg, SOLO, U0, **kw)
        try:
            sol.compute_control(cfg["start_state"])
            alone.append(_results(sol))
        finally:
            sol.close()
    return insts, alone


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("net", NETS, ids=_id)
def test_a_mixed_fleet_of_five_has_the_bits_of_the_solo_twins(net, iters):
    insts, alone = _mixed_fleet(tuple(net), iters)
    sols = [_solver(cfg, V, U0, **kw) for cfg, U0, kw in insts]
    try:
        capi.compute_control_batch(sols, [cfg["start_state"] for cfg, _, _ in insts])
        infos = [s.debug_launch_info() for s in sols]
        assert infos == [(5, 0)] * 5, infos
        for i, s in enumerate(sols):
            got = _results(s)
            assert got["variant"] == fleet_name(net), got["variant"]
            assert alone[i]["variant"] == solo_name(net), alone[i]["variant"]
            _same_bits(got, alone[i], "%s iters=%d instance %d vs %s alone" % (_id(net), iters, i, SOLO))
            assert np.all(np.isfinite(got["costs"]))
        assert len({a["costs"].tobytes() for a in alone}) == 5, "the instances are distinct"
        print("FLEET_MULTI4 bits net=%s iters=%d: 5 instances K=%s T=%d in launches of %s, each equal to %s alone" % (
            _id(net), iters, KS, T, infos[0], SOLO))
    finally:
        _close(sols)


# ------------------------------------------------------------------------------------------------------------------ 2
SMALL = (6, 32, 32, 4)


@functools.lru_cache(maxsize=None)
def _many(n=65, K=64):
    """n instances on one oval: distinct states, seeds and cost parameters; each solved alone with "multi4_tree_gen"."""
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
        sol = _solver(cfg, SOLO, U0, seed=2000 + i)
        try:
            sol.compute_control(cfg["start_state"])
            alone.append(_results(sol))
        finally:
            sol.close()
    assert len({a["costs"].tobytes() for a in alone}) == n, "the instances are distinct"
    return cfgs, U0, alone


@pytest.mark.parametrize("n,shared", [(2, True), (64, True), (65, False)])
def test_fleet_sizes(n, shared):
    """2..64 handles share the launch; beyond 64 every handle is solved alone (launch info (1, 0)) with the same bits."""
    cfgs, U0, alone = _many()
    sols = [_solver(cfgs[i], V, U0, seed=2000 + i) for i in range(n)]
    try:
        capi.compute_control_batch(sols, [cfgs[i]["start_state"] for i in range(n)])
        infos = {s.debug_launch_info() for s in sols}
        print("FLEET_MULTI4 sizes n=%d: launch info %s" % (n, infos))
        assert infos == {(n if shared else 1, 0)}
        for i, s in enumerate(sols):
            _same_bits(_results(s), alone[i], "n=%d instance %d" % (n, i))
    finally:
        _close(sols)


def test_one_handle_through_the_batch_call_and_alone():
    """One handle: the fleet kernel with one instance, launch info (1, 0), through either entry."""
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
        finally:
            sol.close()


# ------------------------------------------------------------------------------------------------------------------ 3
FALLBACKS = ["auto", "fleet16", "another_shape", "another_num_iters", "K_8192", "projective", "stage_timing"]


@pytest.mark.parametrize("what", FALLBACKS)
def test_sets_that_fall_back_to_handle_by_handle_solves(what):
    """Three handles, the middle one out of line: no launch is shared (instances = 1 on every handle) and every handle has the
    bits of its own solve -- the "fleet_multi4" ones those of "multi4_tree_gen" twins."""
    net, K = [6, 32, 32, 4], 192
    cfgs = [S.make_config(K, T, layers=list(net), track="oval") for _ in range(3)]
    for i, cfg in enumerate(cfgs):
        st = np.array(cfg["start_state"], np.float32)
        st[4] += np.float32(0.1 * i)
        cfg["start_state"] = st
    variants = [V, V, V]
    if what in ("auto", "fleet16"):
        variants[1] = what
    elif what == "another_shape":
        cfgs[1] = S.make_config(K, T, layers=[6, 32, 32, 32, 32, 4], track="oval")
    elif what == "another_num_iters":
        cfgs[1] = dict(cfgs[1], num_iters=2)
    elif what == "K_8192":
        cfgs[1] = S.make_config(8192, T, layers=list(net), track="oval")
    elif what == "projective":
        r_c1 = np.array(cfgs[1]["r_c1"], np.float32)
        r_c1[2] = np.float32(2e-5)
        cfgs[1] = dict(cfgs[1], r_c1=r_c1)

    def make(twins):
        sols = [_solver(cfg, SOLO if (twins and v == V) else v, warm_U(cfg), seed=40 + i) for i, (cfg, v) in enumerate(zip(cfgs, variants))]
        if what == "stage_timing":
            sols[1].enable_stage_timing(1)
        return sols
    fleet, solo = make(False), make(True)
    try:
        capi.compute_control_batch(fleet, [cfg["start_state"] for cfg in cfgs])
        for s, cfg in zip(solo, cfgs):
            s.compute_control(cfg["start_state"])
        infos = [s.debug_launch_info() for s in fleet]
        print("FLEET_MULTI4 fallback %s: launch info %s" % (what, infos))
        assert infos == [(1, 0)] * 3
        for i, (a, b) in enumerate(zip(fleet, solo)):
            _same_bits(_results(a), _results(b), "%s handle %d" % (what, i))
        # the control: without the odd one out the other two do share
        capi.compute_control_batch([fleet[0], fleet[2]], [cfgs[0]["start_state"], cfgs[2]["start_state"]])
        assert fleet[0].debug_launch_info() == (2, 0) and fleet[2].debug_launch_info() == (2, 0)
        for i in (0, 2):
            solo[i].compute_control(cfgs[i]["start_state"])
            _same_bits(_results(fleet[i]), _results(solo[i]), "%s: the pair that shares, handle %d" % (what, i))
    finally:
        _close(fleet + solo)


# ------------------------------------------------------------------------------------------------------------------ 4
def _stream_state(sol):
    return sol.get_control_seq(), sol.get_control_hist(), sol.generate_noise()


def test_generator_streams_stay_in_step():
    """Ticks of the fleet against the same ticks driven handle by handle on twins forced to "multi4_tree_gen": the nominal
    sequence, the control history and the generator's NEXT draws are bit-equal per handle -- after 4 shared ticks, after one
    handle left, solved alone and rejoined, and after two different fleets of three alternated without a synchronise between."""
    net = [6, 32, 32, 4]
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
    twins = [_solver(cfg, SOLO, warm_U(cfg), seed=300 + i) for i, cfg in enumerate(cfgs)]

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
        print("FLEET_MULTI4 streams: 6 handles K=%s, 9 ticks in fleets of 6 / 1 / 3 + 3: U, hist and the next draws equal to %s twins" % (Ks, SOLO))
    finally:
        _close(fleet + twins)


# ------------------------------------------------------------------------------------------------------------------ 5
def test_refusals(golden_dir):
    """The basis-function model, a shape whose weights do not fit (6-64x4-4) and a list that is no standard shape (6-48-48-4):
    MPPI_ERR_UNSUPPORTED with a reason that names the form; the handle keeps its form and its results.  A K that is no multiple
    of 64 never reaches the form: mppi_create refuses it (MPPI_ERR_INVALID), so no such handle exists -- the plan's own refusal of
    such a K is tests/test_fleet_multi4_cpu.py's."""
    bf_W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    cases = [("bf", S.make_config(256, 20, track="oval", bf_W=bf_W), "network model"),
             ("6-64x4-4", S.make_config(256, 20, layers=[6, 64, 64, 64, 64, 4], track="oval"), "6-32x2-4, 6-32x4-4 and 6-64x2-4"),
             ("6-48-48-4", S.make_config(256, 20, layers=[6, 48, 48, 4], track="oval"), "6-32x2-4, 6-32x4-4 and 6-64x2-4")]
    with pytest.raises(capi.MppiError) as e:
        capi.Solver(S.make_config(208, 20, layers=[6, 32, 32, 4], track="oval"))
    assert e.value.status == capi.ERR_INVALID
    for tag, cfg, reason in cases:
        sol = capi.Solver(cfg)
        try:
            sol.seed(5, 0)
            before = sol.rollout_variant()
            sol.compute_control(cfg["start_state"])
            first = sol.get_results()
            with pytest.raises(capi.MppiError) as e:
                sol.set_rollout_variant(V)
            print("FLEET_MULTI4 refusal %s: status %d, %s" % (tag, e.value.status, e.value))
            assert e.value.status == capi.ERR_UNSUPPORTED, tag
            assert V in str(e.value) and reason in str(e.value), str(e.value)
            assert sol.rollout_variant() == before
            assert sol.debug_launch_info() == (1, 0)
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


def test_no_gated_form():
    cfg = S.make_config(192, T, layers=[6, 32, 32, 4], track="oval", opt_stride=1)
    st = cfg["start_state"]
    sols = [_solver(cfg, V, warm_U(cfg), seed=77 + i) for i in range(2)]
    twins = [_solver(cfg, SOLO, warm_U(cfg), seed=77 + i) for i in range(2)]
    try:
        capi.control_ticks_batch(sols, [st, st], 1, 1)
        for s in twins:
            s.compute_control(st)
            s.slide_control_seq(1)
        with pytest.raises(capi.MppiError) as e:
            sols[0].arm(0.1)
        print("FLEET_MULTI4 arm: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_UNSUPPORTED
        with pytest.raises(capi.MppiError) as e:
            capi.arm_batch(sols, 0.1)
        print("FLEET_MULTI4 arm_batch: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_UNSUPPORTED
        for s in sols:
            assert not s.is_armed() and s.debug_launch_info() == (2, 0), "nothing was enqueued"
        capi.compute_control_batch(sols, [st, st])
        for a, b in zip(sols, twins):
            b.compute_control(st)
            _same_bits(_results(a), _results(b), "after the refused arm")
    finally:
        _close(sols + twins)


def test_a_handle_without_parameters_fails_the_call_and_moves_nobody():
    net, K = [6, 32, 32, 4], 192
    cfg = S.make_config(K, T, layers=list(net), track="oval")
    U0, st = warm_U(cfg), cfg["start_state"]
    fleet = [_solver(cfg, V, U0, seed=60 + i) for i in range(2)]
    twins = [_solver(cfg, SOLO, U0, seed=60 + i) for i in range(2)]
    bare = _bare_solver(cfg)
    try:
        bare.set_rollout_variant(V)
        with pytest.raises(capi.MppiError) as e:
            capi.compute_control_batch(fleet + [bare], [st] * 3)
        print("FLEET_MULTI4 unready handle: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_STATE and "mppi_set_nn_params" in str(e.value)
        assert [s.debug_launch_info() for s in fleet] == [(0, 0)] * 2, "nothing was enqueued for the other handles"
        capi.compute_control_batch(fleet, [st] * 2)
        for i in range(2):
            twins[i].compute_control(st)
            assert fleet[i].debug_launch_info() == (2, 0)
            _same_bits(_results(fleet[i]), _results(twins[i]), "after the failed call, handle %d" % i)
    finally:
        _close(fleet + twins + [bare])


# ------------------------------------------------------------------------------------------------------------------ 6
def test_the_trace_and_a_live_update_on_a_member_of_a_fleet():
    """mppi_trace_rollouts after a shared solve gives the records it gives after the twin's solo solve; after mppi_update_model on
    every handle the next shared solve has the twins' bits again, and other costs than before."""
    net, K = [6, 64, 64, 4], 128
    cfgs = [S.make_config(K, 23, layers=list(net), track="oval") for _ in range(2)]
    cfgs[1]["start_state"] = np.array(cfgs[1]["start_state"], np.float32) + np.array([0, 0, 0, 0, 0.3, 0, 0], np.float32)
    states = [cfg["start_state"] for cfg in cfgs]
    U0 = warm_U(cfgs[0])
    eps = [noise_for(cfg, 99 + i) for i, cfg in enumerate(cfgs)]
    _, theta2 = P.synthetic_model(list(net), seed=11)
    fleet = [_solver(cfg, V, U0, eps[i]) for i, cfg in enumerate(cfgs)]
    solo = [_solver(cfg, SOLO, U0, eps[i]) for i, cfg in enumerate(cfgs)]
    ks = np.arange(K)

    def step(tag):
        for group in (fleet, solo):
            for i, s in enumerate(group):
                s.set_control_seq(U0)
                s.set_noise(eps[i])
        capi.compute_control_batch(fleet, states)
        assert fleet[0].debug_launch_info() == (2, 0)
        out = []
        for i, (a, b) in enumerate(zip(fleet, solo)):
            b.compute_control(states[i])
            out.append(_results(a))
            _same_bits(out[-1], _results(b), "%s handle %d" % (tag, i))
            ta, tb = a.trace_rollouts(ks), b.trace_rollouts(ks)
            assert set(ta) == set(tb)
            for key in ta:
                np.testing.assert_array_equal(np.asarray(ta[key]), np.asarray(tb[key]), err_msg="%s handle %d trace %s" % (tag, i, key))
        return out
    try:
        first = step("first")
        for s in fleet + solo:
            s.update_model(list(net), _update_data(list(net), np.asarray(theta2, np.float32)))
        second = step("update_model")
        assert not np.array_equal(first[0]["costs"], second[0]["costs"])
        print("FLEET_MULTI4 trace / update_model: 2 shared solves of 2 handles, results and %d traced rollouts each equal to %s twins" % (K, SOLO))
    finally:
        _close(fleet + solo)


# ------------------------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("net", [ER.SHIPPED, ER.N64X2])
def test_every_rollout_of_one_instance_of_a_shared_launch(net):
    """The bar tests/test_every_rollout_gpu.py holds "multi4_tree" to -- V bit-equal to the mode-4 oracle, every cost within TOL64
    of ref64 and TOL_MODE of the oracle, no allowance -- on the ramp at K = 1984, T = 100, solved as instance 3 of a fleet of five."""
    K, T_ = 1984, 100
    cfg, U0, eps = ER._problem(net, K, T_)
    layers = ER.NET_LAYERS[net]
    others = [SC.ramp_config(k, t, layers=layers) for k, t in ((192, 17), (64, 60), (4096, 17), (64, 17))]
    sols = [_solver(c, V, SC.ramp_U(c, seed=i), seed=90 + i) for i, c in enumerate(others)]
    sols.insert(3, _solver(cfg, V, U0, eps))
    try:
        capi.compute_control_batch(sols, [s.cfg["start_state"] for s in sols])
        assert sols[3].debug_launch_info() == (5, 0)
        got = _results(sols[3])
    finally:
        _close(sols)
    h, n = ER.NET_HN[net]
    ER._hold("fleet_multi4 instance 3 of 5", net, K, T_, got, fleet_name([6] + [h] * n + [4]))


# ------------------------------------------------------------------------------------------------------------------ 8
@pytest.mark.timing
def test_the_fleets_tick_beats_fleet16s():
    """16 handles of 6-32-32-4, K = 1920, T = 100, generator noise: the median tick of mppi_control_ticks_batch over 200 ticks
    after 20 warm ones (tools/fleet_time.py) -- (d) "fleet_multi4" is faster than (a) "fleet16" on the same handles, both arms in
    one process.  Measured (MI355X): see DESIGN.md 4.22."""
    spec = importlib.util.spec_from_file_location("fleet_time", os.path.join(ROOT, "tools", "fleet_time.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    rows = ft.table([[6, 32, 32, 4]], n=16, K=1920, T=100, ticks=200, warm=20, ways="da")
    for row in rows:
        assert row["d_instances"] == 16 and row["a_instances"] == 16, row
        assert row["d_ms"] < row["a_ms"], row
