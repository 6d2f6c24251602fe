"""The "fleet_bf" rollout form (csrc/rollout_fleet_bf.hip): the workgroups of the basis-function model's own kernels
(csrc/bf_group.hpp: one, two or three waves per 64 rollouts) with the argument block read from device memory and eps from the
stand-alone generator, so that 2..64 handles of the model share ONE generator, ONE rollout and ONE tail launch per iteration of
mppi_compute_control_batch.  "fleet_bf": the wave count is the plan's choice (tests/test_fleet_bf_cpu.py); "fleet_bf_w1" / "_w2" /
"_w3": that count forced.  The yardstick is existing code: every handle's results are bit for bit those of a twin forced to
"bf3" and solved alone -- the new kernel is never compared to itself.
  1. bits: a mixed fleet of 5 under each of the four names, one and two iterations;
  2. sizes: 2 and 64 share, 65 does not, 1 through the batch call and through mppi_compute_control;
  3. sets that fall back to handle-by-handle solves;
  4. the generator streams stay in step over ticks; a handle leaves and rejoins; two fleets alternate;
  5. refusals, no gated form, a handle without parameters;
  6. the trace and mppi_set_bf_params between two ticks on a member of a fleet;
  7. the every-rollout bar (tests/test_every_rollout_gpu.py: _hold, the bound of "bf3") on one instance of a shared launch, once
     per wave count;
  8. (timing) the fleet's tick against the same handles in "auto".
Shapes: T = 17 wraps the 16-step rings of the two- and three-wave bodies, K = 64 is one workgroup, mixed K makes whole workgroups
leave early.  Each case prints what it measured."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import synthetic as S
from tests import scenes as SC
from tests import test_every_rollout_gpu as ER
from tests.helpers import noise_for, warm_U
from tests.test_fleet16_gpu import _bare_solver
from tests.test_lds44_gpu import _results, _same_bits, _solver

pytestmark = pytest.mark.gpu

U32 = np.uint32
V = "fleet_bf"
NAMES = {"fleet_bf": "basis_funcs25_fleet", "fleet_bf_w1": "basis_funcs25_fleet_w1", "fleet_bf_w2": "basis_funcs25_fleet_w2",
         "fleet_bf_w3": "basis_funcs25_fleet_w3"}
SOLO = "bf3"   # the yardstick: existing code
SOLO_NAME = "basis_funcs25_valu_3w"
KS = (192, 64, 128, 192, 64)   # the largest is not alone and not only first: workgroups x = 1, 2 leave early in three instances
T = 17
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


def _W():
    return np.asarray(ER._bf_W(), np.float32)   # tests/golden/models/basis_function_09_12_2018.npz


def _bf_config(K, T_=T, **over):
    return S.make_config(K, T_, bf_W=_W(), **dict(dict(track="oval"), **over))


def _close(sols):
    for s in sols:
        s.close()


def _set_W(sol, W):
    W = capi._f32(W, (4, 25))
    sol._ck(sol.L.mppi_set_bf_params(sol.h, capi._fp(W), W.size))


# ------------------------------------------------------------------------------------------------------------------ 1
def _instance(i, K, iters):
    """Instance i of the mixed fleet: its own state, W scale, seed, warm U, cost parameters, nu, gamma and control limits;
    instance 2 on another costmap (the ring), instance 3 with explicit noise.  What the instances share: the affine costmap
    transform and no control cost (one pair per launch, csrc/abi_solve.hip: fleet_together)."""
    cfg = _bf_config(K, track="ring" if i == 2 else "oval", num_iters=iters)
    U0 = warm_U(cfg, seed=3 + i)
    st = np.array(cfg["start_state"], np.float32)
    st[4] += np.float32(0.05 * i)
    st[6] += np.float32(0.01 * i)
    cost = dict(cfg["cost"], desired_speed=6.0 + 0.5 * i, speed_coeff=4.25 + 0.25 * i, l1_cost=(i == 1))
    cfg.update(bf_W=_W() * np.float32(1.0 + 0.02 * i), start_state=st, cost=cost,
               nu=(0.275 + 0.01 * i, 0.3 - 0.01 * i), gamma=0.15 + 0.01 * i, u_lo=(-0.99 + 0.02 * i, -0.99), u_hi=(0.99, 0.65 - 0.03 * i))
    kw = dict(eps=noise_for(cfg, 100 + i)) if i == 3 else dict(seed=700 + i)
    return cfg, U0, kw


@functools.lru_cache(maxsize=None)
def _mixed_fleet(iters):
    """The five instances and every one of them solved ALONE with "bf3" (computed once, not changed)."""
    insts = [_instance(i, K, iters) for i, K in enumerate(KS)]
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
@pytest.mark.parametrize("name", list(NAMES))
def test_a_mixed_fleet_of_five_has_the_bits_of_the_solo_twins(name, iters):
    insts, alone = _mixed_fleet(iters)
    sols = [_solver(cfg, name, U0, **kw) for cfg, U0, kw in insts]
    try:
        capi.compute_control_batch(sols, [cfg["start_state"] for cfg, _, _ in insts])
        infos = [s.debug_launch_info() for s in sols]
        assert infos == [(5, 0)] * 5, infos
        for i, s in enumerate(sols):
            got = _results(s)
            assert got["variant"] == NAMES[name], got["variant"]
            assert alone[i]["variant"] == SOLO_NAME, alone[i]["variant"]
            _same_bits(got, alone[i], "%s iters=%d instance %d vs %s alone" % (name, iters, i, SOLO))
            assert np.all(np.isfinite(got["costs"]))
        assert len({a["costs"].tobytes() for a in alone}) == 5, "the instances are distinct"
        print("FLEET_BF bits %s iters=%d: 5 instances K=%s T=%d in launches of %s, each equal to %s alone" % (
            name, iters, KS, T, infos[0], SOLO))
    finally:
        _close(sols)


# ------------------------------------------------------------------------------------------------------------------ 2
@functools.lru_cache(maxsize=None)
def _many(n=65, K=64):
    """n instances on one oval: distinct states, seeds and cost parameters; each solved alone with "bf3"."""
    base = _bf_config(K)
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
        print("FLEET_BF sizes n=%d: launch info %s" % (n, infos))
        assert infos == {(n if shared else 1, 0)}
        for i, s in enumerate(sols):
            _same_bits(_results(s), alone[i], "n=%d instance %d" % (n, i))
    finally:
        _close(sols)


@pytest.mark.parametrize("name", list(NAMES))
def test_one_handle_through_the_batch_call_and_alone(name):
    """One handle: the fleet kernel with one instance, launch info (1, 0), through either entry."""
    cfgs, U0, alone = _many()
    for how in ("batch", "single"):
        sol = _solver(cfgs[3], name, U0, seed=2003)
        try:
            if how == "batch":
                capi.compute_control_batch([sol], [cfgs[3]["start_state"]])
            else:
                sol.compute_control(cfgs[3]["start_state"])
            assert sol.debug_launch_info() == (1, 0)
            got = _results(sol)
            assert got["variant"] == NAMES[name]
            _same_bits(got, alone[3], "%s %s" % (name, how))
        finally:
            sol.close()


# ------------------------------------------------------------------------------------------------------------------ 3
FALLBACKS = ["auto", "bf_row", "network_fleet16", "another_wave_count", "another_num_iters", "control_cost", "projective", "stage_timing"]


@pytest.mark.parametrize("what", FALLBACKS)
def test_sets_that_fall_back_to_handle_by_handle_solves(what):
    """Three handles, the middle one out of line in exactly one thing: no launch is shared (instances = 1 on every handle) and
    every handle has the bits of its own solve -- the "fleet_bf" ones those of "bf3" twins."""
    K = 192
    cfgs = [_bf_config(K) for _ in range(3)]
    for i, cfg in enumerate(cfgs):
        st = np.array(cfg["start_state"], np.float32)
        st[4] += np.float32(0.1 * i)
        cfg["start_state"] = st
    variants = [V, V, V]
    if what in ("auto", "bf_row"):
        variants[1] = what
    elif what == "network_fleet16":
        cfgs[1] = S.make_config(K, T, layers=[6, 32, 32, 4], track="oval")
        variants[1] = "fleet16"
    elif what == "another_wave_count":
        variants = ["fleet_bf_w2", "fleet_bf_w3", "fleet_bf_w2"]
    elif what == "another_num_iters":
        cfgs[1] = dict(cfgs[1], num_iters=2)
    elif what == "control_cost":
        cfgs[1] = dict(cfgs[1], cost=dict(cfgs[1]["cost"], steering_coeff=0.5))
    elif what == "projective":
        r_c1 = np.array(cfgs[1]["r_c1"], np.float32)
        r_c1[2] = np.float32(2e-5)
        cfgs[1] = dict(cfgs[1], r_c1=r_c1)

    def make(twins):
        sols = [_solver(cfg, SOLO if (twins and v in NAMES) else v, warm_U(cfg), seed=40 + i) for i, (cfg, v) in enumerate(zip(cfgs, variants))]
        if what == "stage_timing":
            sols[1].enable_stage_timing(1)
        return sols
    fleet, solo = make(False), make(True)
    try:
        capi.compute_control_batch(fleet, [cfg["start_state"] for cfg in cfgs])
        for s, cfg in zip(solo, cfgs):
            s.compute_control(cfg["start_state"])
        infos = [s.debug_launch_info() for s in fleet]
        print("FLEET_BF fallback %s: launch info %s" % (what, infos))
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
    """Ticks of the fleet against the same ticks driven handle by handle on twins forced to "bf3" (whose control wave draws with
    the in-kernel generator): the nominal sequence, the control history and the generator's NEXT draws are bit-equal per handle --
    after 3 shared ticks, after one handle left, solved alone and rejoined, and after two different fleets of three alternated
    without a synchronise between."""
    Ks = (64, 192, 128, 64, 256, 192)
    cfgs = []
    for i, K in enumerate(Ks):
        cfg = _bf_config(K, opt_stride=1)
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
        capi.control_ticks_batch(fleet, states, 3, 1)
        assert {s.debug_launch_info() for s in fleet} == {(6, 0)}
        twin_ticks(range(6), 3)
        check("3 ticks")
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
        print("FLEET_BF streams: 6 handles K=%s, 8 ticks in fleets of 6 / 1 / 3 + 3: U, hist and the next draws equal to %s twins" % (Ks, SOLO))
    finally:
        _close(fleet + twins)


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("name", list(NAMES))
def test_a_network_handle_is_refused_and_left_as_it_was(name):
    """MPPI_ERR_UNSUPPORTED, "fleet_bf is a form of the basis-function model"; the handle keeps its form and its results."""
    cfg = S.make_config(256, 20, layers=[6, 32, 32, 4], track="oval")
    sol = capi.Solver(cfg)
    try:
        sol.seed(5, 0)
        before = sol.rollout_variant()
        sol.compute_control(cfg["start_state"])
        first = sol.get_results()
        with pytest.raises(capi.MppiError) as e:
            sol.set_rollout_variant(name)
        print("FLEET_BF refusal %s: status %d, %s" % (name, e.value.status, e.value))
        assert e.value.status == capi.ERR_UNSUPPORTED
        assert "fleet_bf is a form of the basis-function model" in str(e.value), str(e.value)
        assert sol.rollout_variant() == before
        assert sol.debug_launch_info() == (1, 0)
        sol.reset_controls()
        sol.seed(5, 0)
        sol.compute_control(cfg["start_state"])
        _same_bits(sol.get_results(), first, name, keys=("costs", "w", "U"))
    finally:
        sol.close()


def test_the_automatic_choice_has_not_changed():
    cfg = _bf_config(256, 20)
    sol = capi.Solver(cfg)
    try:
        auto = sol.rollout_variant()
        for name, reported in NAMES.items():
            sol.set_rollout_variant(name)
            assert sol.rollout_variant() == reported
        sol.set_rollout_variant("auto")
        assert sol.rollout_variant() == auto and "fleet" not in auto
        with pytest.raises(capi.MppiError) as e:
            sol.set_rollout_variant("fleet_bf_w4")
        assert e.value.status == capi.ERR_INVALID and sol.rollout_variant() == auto
    finally:
        sol.close()


def test_no_gated_form():
    cfg = _bf_config(192, opt_stride=1)
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
        print("FLEET_BF arm: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_UNSUPPORTED
        with pytest.raises(capi.MppiError) as e:
            capi.arm_batch(sols, 0.1)
        print("FLEET_BF arm_batch: status %d, %s" % (e.value.status, e.value))
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
    cfg = _bf_config(192)
    U0, st = warm_U(cfg), cfg["start_state"]
    fleet = [_solver(cfg, V, U0, seed=60 + i) for i in range(2)]
    twins = [_solver(cfg, SOLO, U0, seed=60 + i) for i in range(2)]
    bare = _bare_solver(cfg)   # costmap and cost parameters, no W
    try:
        bare.set_rollout_variant(V)
        assert bare.rollout_variant() == NAMES[V]
        with pytest.raises(capi.MppiError) as e:
            capi.compute_control_batch(fleet + [bare], [st] * 3)
        print("FLEET_BF unready handle: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_STATE
        assert [s.debug_launch_info() for s in fleet] == [(0, 0)] * 2, "nothing was enqueued for the other handles"
        capi.compute_control_batch(fleet, [st] * 2)
        for i in range(2):
            twins[i].compute_control(st)
            assert fleet[i].debug_launch_info() == (2, 0)
            _same_bits(_results(fleet[i]), _results(twins[i]), "after the failed call, handle %d" % i)
    finally:
        _close(fleet + twins + [bare])


# ------------------------------------------------------------------------------------------------------------------ 6
def test_the_trace_and_new_parameters_on_a_member_of_a_fleet():
    """mppi_trace_rollouts after a shared solve gives the records it gives after the twin's solo solve; after mppi_set_bf_params on
    every handle between two ticks the next shared solve has the twins' bits again, and other costs than before."""
    K = 128
    cfgs = [_bf_config(K, 23) for _ in range(2)]
    cfgs[1]["start_state"] = np.array(cfgs[1]["start_state"], np.float32) + np.array([0, 0, 0, 0, 0.3, 0, 0], np.float32)
    states = [cfg["start_state"] for cfg in cfgs]
    U0 = warm_U(cfgs[0])
    eps = [noise_for(cfg, 99 + i) for i, cfg in enumerate(cfgs)]
    W2 = _W() * np.float32(1.05)
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
            _set_W(s, W2)
        second = step("set_bf_params")
        assert not np.array_equal(first[0]["costs"], second[0]["costs"])
        print("FLEET_BF trace / set_bf_params: 2 shared solves of 2 handles, results and %d traced rollouts each equal to %s twins" % (K, SOLO))
    finally:
        _close(fleet + solo)


# ------------------------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("name", ["fleet_bf_w1", "fleet_bf_w2", "fleet_bf_w3"])
def test_every_rollout_of_one_instance_of_a_shared_launch(name):
    """The bar tests/test_every_rollout_gpu.py holds "bf3" to -- V bit-equal to the mode-1 oracle, every cost within TOL64 of ref64
    and TOL_MODE of the oracle, no allowance -- on the ramp at K = 1984, T = 100, solved as instance 3 of a fleet of five."""
    K, T_ = 1984, 100
    cfg, U0, eps = ER._problem("bf", K, T_)
    others = [SC.ramp_config(k, t, bf_W=ER._bf_W()) for k, t in ((192, 17), (64, 60), (4096, 17), (64, 17))]
    sols = [_solver(c, name, SC.ramp_U(c, seed=i), seed=90 + i) for i, c in enumerate(others)]
    sols.insert(3, _solver(cfg, name, U0, eps))
    try:
        capi.compute_control_batch(sols, [s.cfg["start_state"] for s in sols])
        assert sols[3].debug_launch_info() == (5, 0)
        got = _results(sols[3])
    finally:
        _close(sols)
    ER._hold("%s instance 3 of 5" % name, "bf", K, T_, got, NAMES[name])


# ------------------------------------------------------------------------------------------------------------------ 8
@pytest.mark.timing
def test_the_fleets_tick_beats_the_same_handles_in_auto():
    """16 handles of the basis-function model, K = 2560, T = 100, generator noise: the median tick of mppi_control_ticks_batch
    over 200 ticks after 20 warm ones (tools/fleet_time.py --model bf) -- (f) "fleet_bf", three launches per tick, is faster than
    (c) the same handles in "auto", solved handle by handle; (F) "fleet_bf" a second time gives the A/A spread of the run, which
    the lead has to exceed.  All arms in one process.  Measured (MI355X): see DESIGN.md 4.23."""
    spec = importlib.util.spec_from_file_location("fleet_time", os.path.join(ROOT, "tools", "fleet_time.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    row = ft.table_bf(n=16, K=2560, T=100, ticks=200, warm=20, ways="fcF")[0]
    spread = abs(row["f_ms"] - row["F_ms"])
    print("FLEET_BF timing: fleet_bf %.4f ms, again %.4f ms (A/A spread %.4f), auto %.4f ms" % (row["f_ms"], row["F_ms"], spread, row["c_ms"]))
    assert row["f_instances"] == 16 and row["F_instances"] == 16 and row["c_instances"] == 1, row
    assert max(row["f_ms"], row["F_ms"]) + spread < row["c_ms"], row
