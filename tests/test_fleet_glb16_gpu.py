"""The "fleet_glb16" rollout form (csrc/rollout_glb16.hip: rollout_fleet_glb16_kernel): the wavefront, the image and the bits of
"glb16" with the argument block AND the layer list read from device memory, so that 2..64 handles of ANY layer lists
mppi_create accepts -- and any caps on their resident blocks -- share ONE generator, ONE rollout and ONE tail launch per
iteration of mppi_compute_control_batch.  Whatever the set, every handle's results are bit for bit those of its own solve.
  1. a mixed fleet of five in the 16-tile instance against every handle alone with "valu_lds" and with "glb16";
  2. the same in the 8-tile instance (one member streams by default);
  3. the seam inside a shared launch: a cap per member; both members of a pair at every cap of seam_caps against "lds16";
  4. the every-rollout bar on one member of a shared launch, once per tile instance;
  5. sizes: 2 and 64 share, 65 does not, 1 through the batch call equals the handle alone;
  6. sets that fall back to handle-by-handle solves;
  7. a handle without parameters; the generator streams stay in step over ticks;
  8. refusals, mppi_arm, the trace, live updates;
  9. (timing) sharing the launches beats the same handles solved one by one in "glb16".
The new kernel is never compared with itself.  Each case prints what it measured."""
import functools
import importlib.util
import os

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import params as P
from autorally_amd import synthetic as S
from tests import scenes as SC
from tests import test_fleet16_gpu as F16
from tests import test_glb16_gpu as G16
from tests.helpers import noise_for, warm_U
from tests.test_glb16_pack import resident_blocks, stream_blocks
from tests.test_lds44_gpu import _results, _same_bits, _solver, _update_data

pytestmark = pytest.mark.gpu

U32 = np.uint32
V = "fleet_glb16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W128X4 = [6, 128, 128, 128, 128, 4]
# (list, K, T) of the members.  16 tiles: a member wider than 128 stands neither first nor alone, the largest K is not first, 64 and
# 1984 leave absent waves in the last workgroup, 6-256-256-4 streams by default.  8 tiles: no member wider than 128, 6-128x4-4 has
# an image beyond the LDS and streams by default
FLEETS = {
    16: (([6, 33, 97, 66, 4], 64, 17), ([6, 197, 67, 4], 1984, 2), ([6, 16, 256, 4], 64, 17), ([6, 129, 4], 1984, 60), ([6, 256, 256, 4], 64, 17)),
    8: (([6, 5, 7, 4], 192, 17), ([6, 32, 32, 4], 64, 2), ([6, 33, 97, 66, 4], 1984, 17), (W128X4, 64, 17), ([6, 64, 64, 64, 64, 4], 64, 17)),
}


def _id(net):
    return "-".join(map(str, net))


def fleet_glb_name(net):
    return "mfma16x16x4_fleet_glb_l%d_w%d" % (len(net) - 2, max(net[1:-1]))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


def _close(sols):
    for s in sols:
        s.close()


def _alone(cfg, variant, U0, kw):
    sol = _solver(cfg, variant, U0, **kw)
    try:
        sol.compute_control(cfg["start_state"])
        return _results(sol)
    finally:
        sol.close()


# --------------------------------------------------------------------------------------------------------------- 1, 2
@functools.lru_cache(maxsize=None)
def _mixed_fleet(tiles, iters):
    """The five instances (tests/test_fleet16_gpu.py: _instance -- own scene, state, weights, cost parameters, nu, gamma, limits;
    explicit noise on the even members, a seed on the odd ones) and every one of them solved ALONE with "valu_lds" and with
    "glb16" (computed once, not changed)."""
    insts = [F16._instance(i, list(net), K, T, iters) for i, (net, K, T) in enumerate(FLEETS[tiles])]
    alone = {v: [_alone(cfg, v, U0, kw) for cfg, U0, kw in insts] for v in ("valu_lds", "glb16")}
    return insts, alone


def _solve_mixed(tiles, iters, variants):
    insts, alone = _mixed_fleet(tiles, iters)
    sols = [_solver(cfg, v, U0, **kw) for (cfg, U0, kw), v in zip(insts, variants)]
    try:
        capi.compute_control_batch(sols, [cfg["start_state"] for cfg, _, _ in insts])
        infos = [s.debug_launch_info() for s in sols]
        assert infos == [(5, 0)] * 5, infos
        for i, s in enumerate(sols):
            net = FLEETS[tiles][i][0]
            got = _results(s)
            assert got["variant"] == fleet_glb_name(net), got["variant"]
            for v in ("valu_lds", "glb16"):
                assert alone[v][i]["variant"] != got["variant"]
                _same_bits(got, alone[v][i], "%d tiles iters=%d member %d (%s, %s) vs %s alone" % (tiles, iters, i, _id(net), variants[i], v))
            assert np.all(np.isfinite(got["costs"]))
        return infos
    finally:
        _close(sols)


@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("tiles", [16, 8])
def test_a_mixed_fleet_of_five_has_every_handles_own_bits(tiles, iters):
    assert (max(max(net[1:-1]) for net, _, _ in FLEETS[tiles]) > 128) == (tiles == 16)
    streams = [_id(net) for net, _, _ in FLEETS[tiles] if resident_blocks(net) < stream_blocks(net)]
    assert streams, "a member of this fleet streams by default"
    infos = _solve_mixed(tiles, iters, [V] * 5)
    print("FLEET_GLB16 bits %d tiles iters=%d: lists %s K=%s T=%s in launches of %s (%s streamed by default), each equal to valu_lds and glb16 alone" % (
        tiles, iters, [_id(m[0]) for m in FLEETS[tiles]], [m[1] for m in FLEETS[tiles]], [m[2] for m in FLEETS[tiles]], infos[0], streams))


# ------------------------------------------------------------------------------------------------------------------ 3
def test_a_cap_per_member_gives_the_same_bits():
    variants = [V + "_r0", V + "_r1", V + "_r3", V, V + "_r17"]
    _solve_mixed(8, 1, variants)
    print("FLEET_GLB16 caps: the 8-tile fleet with %s equal to valu_lds and glb16 alone" % variants)


def test_the_seam_at_every_kind_of_block_inside_a_shared_launch():
    """Two 6-48-48-4 handles, K = 64, T = 17 on the oval, both at "fleet_glb16_r<N>" for every N of tests/test_glb16_gpu.py's
    seam_caps: each equals its own solve in "lds16"."""
    net = [6, 48, 48, 4]
    cfgs = [S.make_config(64, 17, layers=list(net), track="oval") for _ in range(2)]
    cfgs[1]["start_state"] = np.array(cfgs[1]["start_state"], np.float32) + np.array([0, 0, 0, 0, 0.3, 0, 0], np.float32)
    cfgs[1]["theta"] = np.asarray(cfgs[1]["theta"], np.float32) * np.float32(1.03)
    U0 = warm_U(cfgs[0])
    eps = [noise_for(cfg, 77 + i) for i, cfg in enumerate(cfgs)]
    lds16 = [_alone(cfg, "lds16", U0, dict(eps=eps[i])) for i, cfg in enumerate(cfgs)]
    assert lds16[0]["costs"].tobytes() != lds16[1]["costs"].tobytes()
    caps = G16.seam_caps(net)
    assert resident_blocks(net) == stream_blocks(net) == caps[-1], "this list is fully resident without a cap"
    sols = [_solver(cfg, V, U0, eps[i]) for i, cfg in enumerate(cfgs)]
    try:
        for n in caps:
            for i, s in enumerate(sols):
                s.set_rollout_variant("%s_r%d" % (V, n))
                s.set_control_seq(U0)
                s.set_noise(eps[i])
            capi.compute_control_batch(sols, [cfg["start_state"] for cfg in cfgs])
            for i, s in enumerate(sols):
                assert s.debug_launch_info() == (2, 0)
                got = _results(s)
                assert got["variant"] == fleet_glb_name(net) != lds16[i]["variant"]
                _same_bits(got, lds16[i], "%s fleet_glb16_r%d member %d vs lds16" % (_id(net), n, i))
        print("FLEET_GLB16 seam net=%s: %d caps %s, both members of a shared launch equal to lds16" % (_id(net), len(caps), caps))
    finally:
        _close(sols)


# ------------------------------------------------------------------------------------------------------------------ 4
class _Member:
    """What tests/test_glb16_gpu.py's _hold solves: member `at` of a fleet; compute_control solves the whole fleet in one call."""

    def __init__(self, sols, at):
        self._sols, self._at = sols, at

    def compute_control(self, state):
        states = [s.cfg["start_state"] for s in self._sols]
        states[self._at] = state
        capi.compute_control_batch(self._sols, states)
        assert self._sols[self._at].debug_launch_info() == (len(self._sols), 0)

    def close(self):
        _close(self._sols)

    def __getattr__(self, name):
        return getattr(self._sols[self._at], name)


@pytest.mark.parametrize("net,K,T,beside", [([6, 197, 67, 4], 1984, 2, [6, 32, 32, 4]), ([6, 256, 256, 4], 64, 17, [6, 129, 4])], ids=["197-67_beside_32-32", "256-256_beside_129"])
def test_every_rollout_of_one_member_of_a_shared_launch(net, K, T, beside, monkeypatch):
    """The _hold of tests/test_glb16_gpu.py -- V bit-equal to the mode-1 oracle, EVERY cost within TOL64 of ref64 and TOL_MODE of
    the oracle, distinct costs, no crash flag, no allowance -- on the ramp through its _references, solved as the second member of
    a shared launch beside a neighbour of another list.  Both launches are the 16-tile instance (each has a member wider than
    128); in the first the neighbour is an 8-tile list riding in it."""
    def member(cfg, variant, U0, eps=None, seed=None, hist=None):
        other = SC.ramp_config(192, 17, layers=list(beside))
        sols = [_solver(other, variant, SC.ramp_U(other, seed=5), seed=91), _solver(cfg, variant, U0, eps, hist=hist)]
        return _Member(sols, 1)
    monkeypatch.setattr(G16, "_solver", member)
    monkeypatch.setattr(G16, "glb16_name", fleet_glb_name)
    G16._hold("fleet_glb16 member 1 of 2 beside %s" % _id(beside), net, K, T, variant=V)


def test_every_rollout_of_a_member_of_an_8_tile_launch(monkeypatch):
    """The same bar in the 8-tile instance: 6-128x4-4 (K = 64, T = 17; it streams by default) beside a 6-32-32-4 neighbour."""
    def member(cfg, variant, U0, eps=None, seed=None, hist=None):
        other = SC.ramp_config(192, 17, layers=[6, 32, 32, 4])
        sols = [_solver(other, variant, SC.ramp_U(other, seed=5), seed=91), _solver(cfg, variant, U0, eps, hist=hist)]
        return _Member(sols, 1)
    monkeypatch.setattr(G16, "_solver", member)
    monkeypatch.setattr(G16, "glb16_name", fleet_glb_name)
    G16._hold("fleet_glb16 member 1 of 2, 8 tiles", W128X4, 64, 17, variant=V)


# ------------------------------------------------------------------------------------------------------------------ 5
PAIR = ([6, 32, 32, 4], [6, 129, 4])


@functools.lru_cache(maxsize=None)
def _many(n=65, K=64, T=17):
    """n instances on one oval (affine transform, no control cost), alternating 6-32-32-4 and 6-129-4: distinct states, seeds and
    cost parameters; each solved alone with "glb16"."""
    bases = [S.make_config(K, T, layers=list(net), track="oval") for net in PAIR]
    U0 = warm_U(bases[0])
    cfgs = []
    for i in range(n):
        base = bases[i % 2]
        st = np.array(base["start_state"], np.float32)
        st[0] += np.float32(0.3 * i)
        st[4] += np.float32(0.02 * i)
        cfgs.append(dict(base, start_state=st, cost=dict(base["cost"], desired_speed=5.0 + 0.1 * i)))
    alone = [_alone(cfg, "glb16", U0, dict(seed=2000 + i)) for i, cfg in enumerate(cfgs)]
    assert len({a["costs"].tobytes() for a in alone}) == n, "the instances are distinct"
    return cfgs, U0, alone


@pytest.mark.parametrize("n,shared", [(2, True), (64, True), (65, False)])
def test_fleet_sizes(n, shared):
    cfgs, U0, alone = _many()
    sols = [_solver(cfgs[i], V, U0, seed=2000 + i) for i in range(n)]
    try:
        capi.compute_control_batch(sols, [cfgs[i]["start_state"] for i in range(n)])
        infos = {s.debug_launch_info() for s in sols}
        print("FLEET_GLB16 sizes n=%d: launch info %s" % (n, infos))
        assert infos == {(n if shared else 1, 0)}
        for i, s in enumerate(sols):
            got = _results(s)
            assert got["variant"] == fleet_glb_name(PAIR[i % 2])
            _same_bits(got, alone[i], "n=%d instance %d" % (n, i))
    finally:
        _close(sols)


def test_one_handle_through_the_batch_call_and_alone():
    cfgs, U0, alone = _many()
    for at in (2, 3):  # a 6-32-32-4 and a 6-129-4 handle
        for how in ("batch", "single"):
            sol = _solver(cfgs[at], V, U0, seed=2000 + at)
            try:
                if how == "batch":
                    capi.compute_control_batch([sol], [cfgs[at]["start_state"]])
                else:
                    sol.compute_control(cfgs[at]["start_state"])
                assert sol.debug_launch_info() == (1, 0)
                got = _results(sol)
                assert got["variant"] == fleet_glb_name(PAIR[at % 2])
                _same_bits(got, alone[at], "%s handle %d" % (how, at))
                # ... and mppi_rollout_only: the costs of the next draws, as "glb16" alone has them
                twin = _solver(cfgs[at], "glb16", U0, seed=2000 + at)
                try:
                    twin.compute_control(cfgs[at]["start_state"])
                    np.testing.assert_array_equal(sol.rollout_only(cfgs[at]["start_state"]).view(U32),
                                                  twin.rollout_only(cfgs[at]["start_state"]).view(U32))
                finally:
                    twin.close()
            finally:
                sol.close()


# ------------------------------------------------------------------------------------------------------------------ 6
FALLBACKS = ["glb16", "fleet16", "another_num_iters", "another_cost_flags", "K_4160", "stage_timing"]


@pytest.mark.parametrize("what", FALLBACKS)
def test_sets_that_fall_back_to_handle_by_handle_solves(what):
    """Three handles of three lists, the middle one out of line in ONE thing: no launch is shared (instances = 1 on every handle)
    and every handle has the bits of its own solve -- twins in the same forms solved one by one, and the fleet members' twins in
    "glb16".  Without the odd one out the other two do share."""
    nets, K, T = ([6, 129, 4], [6, 33, 97, 66, 4], [6, 16, 24, 4]), 192, 17
    cfgs = [S.make_config(K, T, layers=list(net), track="oval") for net in nets]
    for i, cfg in enumerate(cfgs):
        st = np.array(cfg["start_state"], np.float32)
        st[4] += np.float32(0.1 * i)
        cfg["start_state"] = st
    variants = [V, V, V]
    if what in ("glb16", "fleet16"):
        variants[1] = what
    elif what == "another_num_iters":
        cfgs[1] = dict(cfgs[1], num_iters=2)
    elif what == "K_4160":
        cfgs[1] = dict(S.make_config(4160, T, layers=list(nets[1]), track="oval"), start_state=cfgs[1]["start_state"])
    elif what == "another_cost_flags":
        r_c1 = np.array(cfgs[1]["r_c1"], np.float32)
        r_c1[2] = np.float32(2e-5)
        cfgs[1] = dict(cfgs[1], r_c1=r_c1)

    def make(vs):
        sols = [_solver(cfg, v, warm_U(cfg), seed=40 + i) for i, (cfg, v) in enumerate(zip(cfgs, vs))]
        if what == "stage_timing":
            sols[1].enable_stage_timing(1)
        return sols
    fleet, solo, glb = make(variants), make(variants), make(["glb16"] * 3)
    try:
        capi.compute_control_batch(fleet, [cfg["start_state"] for cfg in cfgs])
        for group in (solo, glb):
            for s, cfg in zip(group, cfgs):
                s.compute_control(cfg["start_state"])
        infos = [s.debug_launch_info() for s in fleet]
        print("FLEET_GLB16 fallback %s: launch info %s" % (what, infos))
        assert infos == [(1, 0)] * 3
        for i, (a, b, c) in enumerate(zip(fleet, solo, glb)):
            _same_bits(_results(a), _results(b), "%s handle %d" % (what, i))
            _same_bits(_results(a), _results(c), "%s handle %d vs glb16" % (what, i))
        capi.compute_control_batch([fleet[0], fleet[2]], [cfgs[0]["start_state"], cfgs[2]["start_state"]])
        assert fleet[0].debug_launch_info() == fleet[2].debug_launch_info() == (2, 0)
    finally:
        _close(fleet + solo + glb)


# ------------------------------------------------------------------------------------------------------------------ 7
def test_a_handle_without_parameters_fails_the_call_and_moves_nobody():
    nets, K, T = ([6, 16, 24, 4], [6, 129, 4]), 192, 17
    cfgs = [S.make_config(K, T, layers=list(net), track="oval") for net in nets]
    U0, st = warm_U(cfgs[0]), cfgs[0]["start_state"]
    fleet = [_solver(cfg, V, U0, seed=60 + i) for i, cfg in enumerate(cfgs)]
    twins = [_solver(cfg, "glb16", U0, seed=60 + i) for i, cfg in enumerate(cfgs)]
    bare = F16._bare_solver(cfgs[1])
    try:
        bare.set_rollout_variant(V)
        with pytest.raises(capi.MppiError) as e:
            capi.compute_control_batch(fleet + [bare], [st] * 3)
        print("FLEET_GLB16 unready handle: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_STATE and "mppi_set_nn_params" in str(e.value)
        assert [s.debug_launch_info() for s in fleet] == [(0, 0)] * 2, "nothing was enqueued for the other handles"
        capi.compute_control_batch(fleet, [st] * 2)
        for i in range(2):
            twins[i].compute_control(st)
            assert fleet[i].debug_launch_info() == (2, 0)
            _same_bits(_results(fleet[i]), _results(twins[i]), "after the failed call, handle %d" % i)
    finally:
        _close(fleet + twins + [bare])


def test_generator_streams_stay_in_step():
    """Ticks of a mixed fleet against the same ticks driven handle by handle on twins forced to "glb16": the nominal sequence, the
    control history and the generator's NEXT draws are bit-equal per handle -- after 4 shared ticks, after one handle left, solved
    alone and rejoined, and after two different fleets of three alternated on the device."""
    T = 17
    nets = ([6, 32, 32, 4], [6, 129, 4], [6, 33, 97, 66, 4], [6, 16, 256, 4], [6, 5, 7, 4], [6, 64, 64, 64, 64, 4])
    Ks = (64, 192, 128, 64, 256, 192)
    cfgs = []
    for i, (net, K) in enumerate(zip(nets, Ks)):
        cfg = S.make_config(K, T, layers=list(net), track="oval", opt_stride=1)
        st = np.array(cfg["start_state"], np.float32)
        st[4] += np.float32(0.1 * i)
        cfg["start_state"] = st
        cfgs.append(cfg)
    states = [cfg["start_state"] for cfg in cfgs]
    fleet = [_solver(cfg, V, warm_U(cfg), seed=300 + i) for i, cfg in enumerate(cfgs)]
    twins = [_solver(cfg, "glb16", warm_U(cfg), seed=300 + i) for i, cfg in enumerate(cfgs)]

    def twin_ticks(idx, n):
        for i in idx:
            for _ in range(n):
                twins[i].compute_control(states[i])
                twins[i].slide_control_seq(1)

    def check(tag):
        # (generate_noise draws: both sides draw, so they stay comparable afterwards)
        for i, (a, b) in enumerate(zip(fleet, twins)):
            for x, y, what in zip(F16._stream_state(a), F16._stream_state(b), ("U", "hist", "next draws")):
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
        # two different fleets alternate on the device: the first an 8-tile launch beside a wide member, the second a 16-tile one
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
        print("FLEET_GLB16 streams: 6 handles of 6 lists K=%s, 9 ticks in fleets of 6 / 1 / 3 + 3: U, hist and the next draws equal to glb16 twins" % (Ks,))
    finally:
        _close(fleet + twins)


# ------------------------------------------------------------------------------------------------------------------ 8
def test_refusals_leave_the_handle_as_it_was(golden_dir):
    bf_W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    cases = [("bf", S.make_config(256, 20, track="oval", bf_W=bf_W), V, capi.ERR_UNSUPPORTED, V),
             ("6-4", S.make_config(256, 20, layers=[6, 4], track="oval"), V, capi.ERR_UNSUPPORTED, V),
             ("6-4", S.make_config(256, 20, layers=[6, 4], track="oval"), V + "_r0", capi.ERR_UNSUPPORTED, V)]
    wide = S.make_config(256, 20, layers=[6, 129, 4], track="oval")
    cases += [("malformed", wide, V + tail, capi.ERR_INVALID, "unknown variant")
              for tail in ("_", "_r", "_rx", "x", "_r-1", "_r1x", "_r 1", "r1", "_R1", "_r+1")]
    for tag, cfg, name, status, text in cases:
        sol = capi.Solver(cfg)
        try:
            sol.seed(5, 0)
            before = sol.rollout_variant()
            sol.compute_control(cfg["start_state"])
            first = sol.get_results()
            glb16_status = None
            if status == capi.ERR_UNSUPPORTED:  # the refusals are those of "glb16"
                with pytest.raises(capi.MppiError) as e:
                    sol.set_rollout_variant(name.replace(V, "glb16"))
                glb16_status = e.value.status
                assert glb16_status == status
            with pytest.raises(capi.MppiError) as e:
                sol.set_rollout_variant(name)
            print("FLEET_GLB16 refusal %s %r: status %d, %s" % (tag, name, e.value.status, e.value))
            assert e.value.status == status, (tag, name, e.value.status)
            assert text in str(e.value), str(e.value)
            assert sol.rollout_variant() == before
            sol.reset_controls()
            sol.seed(5, 0)
            sol.compute_control(cfg["start_state"])
            _same_bits(sol.get_results(), first, tag, keys=("costs", "w", "U"))
        finally:
            sol.close()
    for net in ([6, 129, 4], [6, 200, 256, 4], G16.DEEP8, [6, 32, 32, 4]):
        sol = capi.Solver(S.make_config(256, 20, layers=net, track="oval"))
        try:
            auto = sol.rollout_variant()
            for name in (V, V + "_r0", V + "_r000012", V + "_r999999999"):
                sol.set_rollout_variant(name)
                assert sol.rollout_variant() == fleet_glb_name(net)
            sol.set_rollout_variant("auto")
            assert sol.rollout_variant() == auto and "fleet" not in auto  # the automatic choice has not changed
        finally:
            sol.close()


def test_no_gated_form_and_the_next_solve_is_an_ordinary_one():
    nets = ([6, 48, 48, 4], [6, 129, 4])
    cfgs = [S.make_config(192, 17, layers=list(net), track="oval", opt_stride=1) for net in nets]
    states = [cfg["start_state"] for cfg in cfgs]
    sols = [_solver(cfg, V, warm_U(cfg), seed=77 + i) for i, cfg in enumerate(cfgs)]
    twins = [_solver(cfg, "glb16", warm_U(cfg), seed=77 + i) for i, cfg in enumerate(cfgs)]
    try:
        capi.control_ticks_batch(sols, states, 1, 1)
        capi.control_ticks_batch(twins, states, 1, 1)
        with pytest.raises(capi.MppiError) as e:
            sols[0].arm(0.1)
        print("FLEET_GLB16 arm: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_UNSUPPORTED
        with pytest.raises(capi.MppiError) as e:
            capi.arm_batch(sols, 0.1)
        print("FLEET_GLB16 arm_batch: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_UNSUPPORTED
        for s in sols:
            assert not s.is_armed() and s.debug_launch_info() == (2, 0), "nothing was enqueued"
        capi.compute_control_batch(sols, states)
        for a, b, st in zip(sols, twins, states):
            b.compute_control(st)
            assert a.debug_launch_info() == (2, 0)
            _same_bits(_results(a), _results(b), "after the refused arm")
    finally:
        _close(sols + twins)


def test_the_trace_after_a_shared_solve_has_the_costs_of_the_solve():
    nets = ([6, 33, 97, 66, 4], [6, 200, 256, 4])
    cfgs = [S.make_config(256, 23, layers=list(net), track="oval") for net in nets]
    cfgs[1]["start_state"] = np.array(cfgs[1]["start_state"], np.float32) + np.array([0, 0, 0, 0, 0.3, 0, 0], np.float32)
    fleet = [_solver(cfg, V, warm_U(cfg), seed=31 + i) for i, cfg in enumerate(cfgs)]
    solo = [_solver(cfg, "glb16", warm_U(cfg), seed=31 + i) for i, cfg in enumerate(cfgs)]
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
    """Between the ticks of a shared launch: mppi_update_model on one member, mppi_set_control_limits on the other, a variant
    switch away and back -- every solve of every handle equals the same sequence on "valu_lds" alone, bit for bit."""
    nets = ([6, 33, 97, 66, 4], [6, 129, 4])
    cfgs = [S.make_config(192, 17, layers=list(net), track="oval") for net in nets]
    cfgs[1]["start_state"] = np.array(cfgs[1]["start_state"], np.float32) + np.array([0, 0, 0, 0, 0.3, 0, 0], np.float32)
    states = [cfg["start_state"] for cfg in cfgs]
    U0 = warm_U(cfgs[0])
    eps = [noise_for(cfg, 99 + i) for i, cfg in enumerate(cfgs)]
    _, theta2 = P.synthetic_model(list(nets[1]), seed=11)
    fleet = [_solver(cfg, V, U0, eps[i]) for i, cfg in enumerate(cfgs)]
    twins = [_solver(cfg, "valu_lds", U0, eps[i]) for i, cfg in enumerate(cfgs)]
    infos, prev = [], None

    def step(tag, who):
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
        changed = prev is None or not np.array_equal(prev[who]["costs"], now[who]["costs"])
        prev = now
        return changed
    try:
        step("first", 0)
        for s in (fleet[1], twins[1]):
            s.update_model(list(nets[1]), _update_data(list(nets[1]), np.asarray(theta2, np.float32)))
        assert step("update_model on member 1", 1)
        for s in (fleet[0], twins[0]):
            s.set_control_limits((-0.4, -0.5), (0.45, 0.3))
        assert step("set_control_limits on member 0", 0)
        fleet[1].set_rollout_variant("auto")
        step("one handle on auto", 1)
        fleet[1].set_rollout_variant(V + "_r2")
        step("and back, under a cap", 1)
        print("FLEET_GLB16 live updates: 5 solves equal to valu_lds, launch info %s" % infos)
        assert infos == [(2, 0)] * 3 + [(1, 0), (2, 0)], infos
    finally:
        _close(fleet + twins)


# ------------------------------------------------------------------------------------------------------------------ 9
@pytest.mark.timing
def test_sharing_the_launches_beats_glb16_handle_by_handle():
    """16 handles cycling through four lists, K = 1920, T = 100, generator noise: the median tick of mppi_control_ticks_batch over
    200 ticks after 20 warm ones (tools/fleet_time.py --mixed) -- (a) "fleet_glb16" is below (b) the same handles forced to
    "glb16", handle by handle, by more than the A/A spread of the run (a against A: "fleet_glb16" a second time).  ("auto" is
    "valu_lds" on two of these lists, 0.4 s per tick at four handles: not run here.)  Measured (MI355X): see DESIGN.md 4.24."""
    spec = importlib.util.spec_from_file_location("fleet_time", os.path.join(ROOT, "tools", "fleet_time.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    row, = ft.mixed_table([[6, 32, 32, 4], [6, 64, 64, 64, 64, 4], [6, 129, 4], [6, 256, 256, 4]], ns=(16,), ways="abA")
    assert row["a_instances"] == row["A_instances"] == 16 and row["b_instances"] == 1, row
    spread = abs(row["a_ms"] - row["A_ms"])
    assert max(row["a_ms"], row["A_ms"]) + spread < row["b_ms"], row
