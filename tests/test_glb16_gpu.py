"""The "glb16" rollout form (csrc/rollout_glb16.hip): every layer list mppi_create accepts for the network model -- hidden widths
up to 256, an image of any size -- on "lds16"'s wavefront (16 rollouts, v_mfma_f32_16x16x4_f32, the reference's order), the head of
the image and the first R blocks of its stream resident in LDS, the other blocks read from the image in global memory.  The form
is EXACT: its arithmetic is the oracle's mode 1, its bits are those of "valu_lds" and of "lds16", for every R ("glb16_r<N>").
  1. every rollout of every layer list against ref64 and the mode-1 oracle on the flip-free ramp (tests/scenes.py);
  2. bit-identity with "valu_lds": ring, oval and ramp, explicit noise and the generator, two iterations;
  3. the seam between resident and streamed blocks at every kind of block, against "lds16", "glb16" and "glb16_r0";
  4. a -inf yaw rate on ragged lists (a padded neuron's activation is SET to 0);
  5. launch shapes: K = 16 384 and a K from the device's CU count for each workgroup size; U behind the streaming tail;
  6. live updates follow "valu_lds" bit for bit; 7. refusals, names, mppi_arm, a batch of two, the trace, "auto";
  8. not slower than "valu_lds".
Each case prints what it measured.

The references of 1. are computed on the host and the mode-1 oracle is held to ref64 there BEFORE the GPU result is looked at
(_references): with the synthetic weights of tests/scenes.py (gentle_model) every (list, shape) below passes that check, so no
(list, scene, seed) had to be replaced."""
import functools
import os
from unittest import mock

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import params as P
from autorally_amd import synthetic as S
from oracle import oracle as O
from tests import branch_cases as BC
from tests import edge_cases as EC
from tests import ref64 as R
from tests import scenes as SC
from tests.helpers import noise_for, oracle_mode_for, rel_err, warm_U
from tests.scenes import TOL64, TOL_MODE
from tests.test_glb16_pack import AHEAD, glb16_packer, lds_bytes, resident_blocks, stream_blocks, workgroup_threads  # noqa: F401 (a fixture)
from tests.test_lds16_pack import _tiles
from tests.test_lds44_gpu import _cus, _results, _same_bits, _solve, _solver, _update_data

pytestmark = pytest.mark.gpu

U32 = np.uint32
V = "glb16"
DEEP8 = [6, 20, 70, 9, 130, 33, 65, 4]
W128X4 = [6, 128, 128, 128, 128, 4]
# nine tiles (an odd last tile in the 16-tile instance); a narrow layer behind the widest; ragged 13 and 16 tiles; the largest
# two-layer list; 13 and 5 tiles; one tile in front of 16; eight entries; the 8-tile instance with an image beyond the LDS; a fully
# resident list
NETS = [[6, 129, 4], [6, 256, 7, 4], [6, 200, 256, 4], [6, 256, 256, 4], [6, 197, 67, 4], [6, 16, 256, 4], DEEP8, W128X4, [6, 33, 97, 66, 4]]
SHAPES = [(64, 17), (1984, 2), (1984, 60)]  # 1984 = 31 x 64: a workgroup with absent waves at 512 threads
EXTRA_LISTS = {"129": [6, 129, 4], "200-256": [6, 200, 256, 4]}  # names for tests/edge_cases.py, while this file runs


def _id(net):
    return "-".join(map(str, net))


def glb16_name(net):
    return "mfma16x16x4_glb_l%d_w%d" % (len(net) - 2, max(net[1:-1]))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    with mock.patch.dict(BC.NET_LAYERS, EXTRA_LISTS):
        yield


# ------------------------------------------------------------------------------------------------------------------ 1
@functools.lru_cache(maxsize=None)
def _references(net, K, T, with_ref64=True):
    """(cfg, U0, eps, the mode-1 oracle's costs and V, ref64's costs) on the ramp, the oracle held to ref64 on the host."""
    cfg = SC.ramp_config(K, T, layers=list(net))
    U0 = SC.ramp_U(cfg, seed=K % 31 + T)
    eps = noise_for(cfg, 1000 + T)
    costs_o, V_o, crash_o = O.Oracle(cfg, fma_mode=1, nthreads=16).rollouts(cfg["start_state"], U0, eps[0])
    assert not np.any(crash_o)
    costs_r = None
    if with_ref64:
        costs_r, _, crash_r = R.Ref64(cfg).rollouts(cfg["start_state"], U0, eps[0])
        assert not np.any(crash_r)
        e = rel_err(costs_o, costs_r)
        assert float(e.max()) <= TOL64, ("the mode-1 oracle itself is outside the ref64 bound here", _id(net), K, T, float(e.max()))
    return cfg, U0, eps, costs_o, V_o, costs_r


def _hold(tag, net, K, T, with_ref64=True, variant=V, hist=None):
    """The every-rollout bar of tests/test_lds16_gpu.py: the name, V bit-equal to the mode-1 oracle, EVERY cost within TOL64 of
    ref64 and TOL_MODE of the oracle, on costs that differ from rollout to rollout, no crash flag, no count allowance."""
    cfg, U0, eps, costs_o, V_o, costs_r = _references(tuple(net), K, T, with_ref64)
    sol = _solver(cfg, variant, U0, eps, hist=hist)
    try:
        sol.compute_control(cfg["start_state"])
        got = _results(sol)
    finally:
        sol.close()
    assert got["variant"] == glb16_name(net), got["variant"]
    assert oracle_mode_for(got["variant"]) == 1
    assert len(np.unique(got["costs"])) > K // 2, "the rollouts of this case are not distinct"
    np.testing.assert_array_equal(got["V"].view(U32), V_o.view(U32))
    eo = rel_err(got["costs"], costs_o)
    ko = int(np.argmax(eo))
    line = "GLB16 %s net=%s K=%d T=%d: oracle max %.2e (k=%d), %d of %d costs bit-equal to the oracle, %d distinct" % (
        tag, _id(net), K, T, eo[ko], ko, int(np.sum(got["costs"].view(U32) == costs_o.view(U32))), K, len(np.unique(got["costs"])))
    if with_ref64:
        e64 = rel_err(got["costs"], costs_r)
        k64 = int(np.argmax(e64))
        print(line + "; ref64 max %.2e (k=%d, margin x%.1f)" % (e64[k64], k64, TOL64 / max(e64[k64], 1e-30)))
        assert float(e64[k64]) <= TOL64, ("ref64", k64, float(e64[k64]), int(np.sum(e64 > TOL64)))
    else:
        print(line)
    assert float(eo[ko]) <= TOL_MODE, ("oracle mode 1", ko, float(eo[ko]), int(np.sum(eo > TOL_MODE)))
    return cfg, got


@pytest.mark.parametrize("K,T", SHAPES)
@pytest.mark.parametrize("net", NETS, ids=_id)
def test_every_rollout_of_every_layer_list(net, K, T):
    _hold("every", net, K, T)


# ------------------------------------------------------------------------------------------------------------------ 2
def _scene(track, net, K=256, T=13, **over):
    if track == "ramp":
        cfg = SC.ramp_config(K, T, layers=list(net), **over)
        return cfg, SC.ramp_U(cfg)
    cfg = S.make_config(K, T, layers=list(net), track=track, **over)
    return cfg, warm_U(cfg)


@pytest.mark.parametrize("net", NETS, ids=_id)
def test_bit_identical_to_the_generic_kernel(net):
    """Costs, weights, V, U and the trajectory cost of "glb16" are those of "valu_lds" as uint32: on the ring and the oval
    (crashes, thresholds) and on the ramp, with explicit noise and with the generator's draws, with two iterations.  K = 256,
    T = 13: the generic kernel reads the wide lists' parameters from global memory on every use."""
    for track in ("ring", "oval", "ramp"):
        cfg, U0 = _scene(track, net, num_iters=2)
        eps = noise_for(cfg, 4321)
        for mode, kw in (("explicit", dict(eps=eps)), ("generator", dict(seed=97))):
            got = _solve(cfg, V, U0, **kw)
            assert got["variant"] == glb16_name(net)
            ref = _solve(cfg, "valu_lds", U0, **kw)
            assert ref["variant"] == "valu_lds"
            _same_bits(got, ref, "%s %s %s vs valu_lds" % (_id(net), track, mode))
        print("GLB16 bits net=%s %s iters=2: equal to valu_lds; costs %.4g .. %.4g, %d distinct" % (
            _id(net), track, float(got["costs"].min()), float(got["costs"].max()), len(np.unique(got["costs"]))))
        assert np.all(np.isfinite(got["costs"]))


# ------------------------------------------------------------------------------------------------------------------ 3
def seam_caps(net):
    """Caps N ("glb16_r<N>": blocks below N resident) that put the seam at every kind of block of the stream: 0 .. 3, the first and
    the last block of every layer, the last block of every pair of tiles, every block of an odd last tile, the block behind each
    of those, and all of the stream."""
    mt = _tiles(net)
    caps, b = {0, 1, 2, 3}, 0
    for j in range(1, len(mt)):
        mt_in, mt_out = mt[j - 1], mt[j]
        caps |= {b, b + 1}                                   # the layer's first block
        for p in range(mt_out // 2):
            b += 2 * mt_in
            caps |= {b - 1, b}                               # the last block of a pair
        if mt_out % 2:
            caps |= set(range(b, b + mt_in + 1))             # an odd last tile (the output layer is one)
            b += mt_in
        caps |= {b - 1, b}                                   # the layer's last block
    assert b + AHEAD == stream_blocks(net)
    caps |= {b + AHEAD - 1, b + AHEAD}
    return sorted(c for c in caps if 0 <= c <= stream_blocks(net))


@pytest.mark.parametrize("net", [[6, 48, 48, 4], [6, 33, 97, 66, 4]], ids=_id)
def test_the_seam_at_every_kind_of_block(net):
    """K = 64, T = 17 on the oval: "glb16_r<N>" for every N of seam_caps equals "lds16" and "glb16" bit for bit."""
    cfg, U0 = _scene("oval", net, K=64, T=17)
    eps = noise_for(cfg, 77)
    lds16, full = _solve(cfg, "lds16", U0, eps), _solve(cfg, V, U0, eps)
    assert lds16["variant"] != full["variant"] == glb16_name(net)
    _same_bits(full, lds16, "%s glb16 vs lds16" % _id(net))
    caps = seam_caps(net)
    assert resident_blocks(net) == stream_blocks(net) == caps[-1], "this list is fully resident without a cap"
    for n in caps:
        got = _solve(cfg, "glb16_r%d" % n, U0, eps)
        assert got["variant"] == glb16_name(net)
        _same_bits(got, lds16, "%s glb16_r%d vs lds16" % (_id(net), n))
    print("GLB16 seam net=%s: %d caps %s equal to lds16 and glb16" % (_id(net), len(caps), caps))


def test_the_seam_of_the_widest_list():
    """6-256-256-4: the default R (149 of 274 blocks), R - 1 and R + 1 (clipped to R) against everything streamed."""
    net = [6, 256, 256, 4]
    cfg, U0 = _scene("oval", net, K=64, T=17)
    eps = noise_for(cfg, 78)
    r = resident_blocks(net)
    assert 0 < r < stream_blocks(net)
    ref = _solve(cfg, "glb16_r0", U0, eps)
    for v in (V, "glb16_r%d" % (r - 1), "glb16_r%d" % (r + 1), "glb16_r1", "glb16_r16", "glb16_r17"):
        _same_bits(_solve(cfg, v, U0, eps), ref, "%s %s vs glb16_r0" % (_id(net), v))
    _same_bits(_solve(cfg, "valu_lds", U0, eps), ref, "%s valu_lds vs glb16_r0" % _id(net))
    print("GLB16 seam net=%s: R = %d of %d blocks; R, R - 1, R + 1, 1, 16, 17 equal to glb16_r0 and valu_lds" % (_id(net), r, stream_blocks(net)))


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("K", EC.START_KS)
@pytest.mark.parametrize("name", list(EXTRA_LISTS))
def test_a_minus_inf_yaw_rate_on_ragged_lists(name, K):
    """tests/edge_cases.py's start state "yaw_rate_minus_inf" on 6-129-4 (one neuron in the ninth tile) and 6-200-256-4 (eight in
    the thirteenth): the zero weights of a neuron that does not exist times -inf are NaN; its activation is SET to 0.  The bar
    is edge_cases.hold_start_state's: the mode-1 oracle's costs, V bit-equal, U behind ref64's tail stages."""
    cfg, U0, eps, state = EC.start_state_problem(name, K, "yaw_rate_minus_inf")
    for variant in (V, "glb16_r1"):
        sol = _solver(cfg, variant, U0, eps, hist=EC.START_HIST)
        try:
            sol.compute_control(state)
            got = _results(sol)
        finally:
            sol.close()
        EC.hold_start_state(variant, name, K, "yaw_rate_minus_inf", got, glb16_name(EXTRA_LISTS[name]))


# ------------------------------------------------------------------------------------------------------------------ 5
def _launch_cases():
    """(net, K, T) -> the workgroup the rule picks: K = 16 384 on the widest and on a small list (256 threads, every workgroup
    resident); 128 rollouts per CU on an image beyond the LDS (512 threads, one workgroup per CU); one 64-block more than two
    256-thread workgroups per CU hold on a small list (512 threads as the largest, a second round, absent waves)."""
    cus = _cus()
    return [([6, 256, 256, 4], 16384, 5), ([6, 129, 4], 16384, 17), (W128X4, 128 * cus, 5), ([6, 129, 4], 128 * cus + 64, 17)], cus


@pytest.mark.parametrize("case", range(4))
def test_launch_shapes(case, glb16_packer):  # noqa: F811
    """V bit-equal to the mode-1 oracle and every cost within TOL_MODE of it; K > 4096: U behind the streaming tail within 2e-6
    of ref64's weighting, reduction and smoothing fed with the solve's own costs and V (tests/test_edge_rollouts_gpu.py's bar)."""
    cases, cus = _launch_cases()
    net, K, T = cases[case]
    threads = [workgroup_threads(n, k, cus) for n, k, _ in cases]
    _, (r, nbytes, got_threads) = glb16_packer(net, K=K, cus=cus)
    assert got_threads == threads[case] and (r, nbytes) == (resident_blocks(net), lds_bytes(net)), (got_threads, threads, r, nbytes)
    print("GLB16 launch net=%s K=%d on %d CUs: %d of %d blocks resident, %d bytes of LDS, %d threads per workgroup, %d workgroups (all cases: %s)" % (
        _id(net), K, cus, r, stream_blocks(net), nbytes, threads[case], -(-(K // 16) // (threads[case] // 64)), threads))
    assert {256, 512} <= set(threads), threads
    cfg, got = _hold("launch", net, K, T, with_ref64=False, hist=EC.START_HIST)
    assert K > 4096
    ref = R.Ref64(cfg)
    w, beta, eta, tc = ref.weights(got["costs"])
    dU = float(np.max(np.abs(ref.savgol(ref.weighted_reduction(w, eta, got["V"]), EC.START_HIST) - got["U"])))
    print("GLB16 launch net=%s K=%d: |dU| %.2e against ref64's tail stages (bar 2e-6)" % (_id(net), K, dU))
    assert np.all(np.isfinite(got["U"])) and dU <= 2e-6, dU


# ------------------------------------------------------------------------------------------------------------------ 6
def test_live_updates_follow_the_generic_kernel():
    """A solve after each of mppi_set_nn_params, mppi_update_model, mppi_set_cost_params, mppi_set_costmap_transform and a variant
    switch away and back on 6-129-4: the image follows the model -- every solve equals the same sequence on "valu_lds" bit for bit."""
    net = [6, 129, 4]
    cfg, U0 = _scene("oval", net, K=512, T=43)
    eps = noise_for(cfg, 99)
    _, theta2 = P.synthetic_model(list(net), seed=11)
    _, theta3 = P.synthetic_model(list(net), seed=12)
    cost2 = dict(cfg["cost"], desired_speed=7.5, speed_coeff=3.0, crash_coeff=8000.0)
    r_c1, r_c2, trs = np.array(cfg["r_c1"], np.float32), np.array(cfg["r_c2"], np.float32), np.array(cfg["trs"], np.float32)
    trs2 = trs.copy()
    trs2[0] += np.float32(0.004)
    trs2[1] -= np.float32(0.003)
    trace = {}
    for variant in (V, "valu_lds"):
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
            sol.set_cost_params(cost2)
            solve()
            sol.set_costmap_transform(r_c1, r_c2, trs2)
            solve()
            sol.set_rollout_variant("auto")
            solve()
            sol.set_rollout_variant(variant)
            solve()
        finally:
            sol.close()
        trace[variant] = out
    names = [o["variant"] for o in trace[V]]
    assert names[:5] == [glb16_name(net)] * 5 and names[6] == glb16_name(net) and names[5] == "valu_lds", names
    for i, (a, b) in enumerate(zip(trace[V], trace["valu_lds"])):
        _same_bits(a, b, "%s after update %d" % (_id(net), i))
    for i in range(1, 5):  # every update changed the solve
        assert not np.array_equal(trace[V][i]["costs"], trace[V][i - 1]["costs"]), i
    print("GLB16 live updates net=%s: 7 solves equal to valu_lds, names %s" % (_id(net), names))


# ------------------------------------------------------------------------------------------------------------------ 7
def test_refusals_leave_the_handle_as_it_was(golden_dir):
    bf_W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    cases = [("bf", S.make_config(256, 20, track="oval", bf_W=bf_W), V, capi.ERR_UNSUPPORTED, "glb16"),
             ("6-4", S.make_config(256, 20, layers=[6, 4], track="oval"), V, capi.ERR_UNSUPPORTED, "glb16"),
             ("6-4", S.make_config(256, 20, layers=[6, 4], track="oval"), "glb16_r0", capi.ERR_UNSUPPORTED, "glb16")]
    wide = S.make_config(256, 20, layers=[6, 129, 4], track="oval")
    cases += [("malformed", wide, name, capi.ERR_INVALID, "unknown variant")
              for name in ("glb16_", "glb16_r", "glb16_rx", "glb16x", "glb16_r-1", "glb16_r1x", "glb16_r 1", "glb16r1", "glb16_R1", "glb16_r+1")]
    for tag, cfg, name, status, text in cases:
        sol = capi.Solver(cfg)
        try:
            sol.seed(5, 0)
            before = sol.rollout_variant()
            sol.compute_control(cfg["start_state"])
            first = sol.get_results()
            with pytest.raises(capi.MppiError) as e:
                sol.set_rollout_variant(name)
            print("GLB16 refusal %s %r: status %d, %s" % (tag, name, e.value.status, e.value))
            assert e.value.status == status, (tag, name, e.value.status)
            assert text in str(e.value), str(e.value)
            assert sol.rollout_variant() == before
            sol.reset_controls()
            sol.seed(5, 0)
            sol.compute_control(cfg["start_state"])
            _same_bits(sol.get_results(), first, tag, keys=("costs", "w", "U"))
        finally:
            sol.close()
    for net in ([6, 129, 4], [6, 200, 256, 4], DEEP8):
        sol = capi.Solver(S.make_config(256, 20, layers=net, track="oval"))
        try:
            assert sol.rollout_variant() == "valu_lds"
            for name in (V, "glb16_r0", "glb16_r000012", "glb16_r999999999"):
                sol.set_rollout_variant(name)
                assert sol.rollout_variant() == glb16_name(net)
            sol.set_rollout_variant("auto")
            assert sol.rollout_variant() == "valu_lds"  # the automatic choice has not changed
            assert sol.form_candidates() == ["valu_lds"]
        finally:
            sol.close()


def test_no_gated_form_and_the_next_solve_is_an_unarmed_one():
    net = [6, 129, 4]
    cfg = S.make_config(512, 30, layers=net, track="oval", opt_stride=1)
    sols = [capi.Solver(cfg) for _ in range(2)]
    try:
        for sol in sols:
            sol.set_rollout_variant(V)
            sol.seed(77, 0)
            sol.compute_control(cfg["start_state"])
            sol.slide_control_seq(1)
        with pytest.raises(capi.MppiError) as e:
            sols[0].arm(0.1)
        print("GLB16 arm: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_UNSUPPORTED
        assert not sols[0].is_armed() and sols[0].debug_launch_info() == (1, 0), "nothing was enqueued"
        res = []
        for sol in sols:
            sol.compute_control(cfg["start_state"])
            res.append(_results(sol))
        _same_bits(res[0], res[1], "after the refused arm")
        assert res[0]["variant"] == glb16_name(net)
    finally:
        for sol in sols:
            sol.close()


def test_a_batch_of_two_handles_equals_their_single_solves():
    """No batched kernel: mppi_compute_control_batch solves the handles one by one, each in a launch of its own."""
    net, K, T = [6, 129, 4], 1920, 33
    cfgs = [S.make_config(K, T, layers=list(net), track="oval", opt_stride=1, instance=i) for i in range(2)]
    solo = [_solve(cfg, V, warm_U(cfg), seed=500 + i) for i, cfg in enumerate(cfgs)]
    sols = [_solver(cfg, V, warm_U(cfg), seed=500 + i) for i, cfg in enumerate(cfgs)]
    try:
        capi.compute_control_batch(sols, [cfg["start_state"] for cfg in cfgs])
        infos = [s.debug_launch_info() for s in sols]
        print("GLB16 batch net=%s: launch info %s" % (_id(net), infos))
        assert infos == [(1, 0), (1, 0)]
        for i, s in enumerate(sols):
            got = _results(s)
            assert got["variant"] == glb16_name(net)
            _same_bits(got, solo[i], "instance %d" % i)
    finally:
        for s in sols:
            s.close()


def test_the_trace_of_a_solve_has_its_costs():
    net = [6, 200, 256, 4]
    cfg = S.make_config(256, 23, layers=list(net), track="oval")
    sol = _solver(cfg, V, warm_U(cfg), seed=31)
    try:
        sol.compute_control(cfg["start_state"])
        got = sol.get_results()
        tr = sol.trace_rollouts(np.arange(cfg["K"]))
        same = int(np.sum(tr["costs"].view(U32) == got["costs"].view(U32)))
        print("GLB16 trace net=%s: %d of %d traced costs bit-equal to the solve's, %d rollouts crash" % (
            _id(net), same, cfg["K"], int(np.sum(tr["first_crash"] >= 0))))
        np.testing.assert_array_equal(tr["costs"].view(U32), got["costs"].view(U32))
        assert sol.rollout_variant() == glb16_name(net)
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("net", [[6, 256, 256, 4], W128X4], ids=_id)
def test_not_slower_than_the_generic_kernel(net):
    """K = 1984, T = 60: the median rollout stage (the kernel's own dispatch time, every 2nd solve timed) of 6 timed solves per
    form, the forms alternating in blocks inside one process.  The generic kernel takes tenths of a second per solve on these
    lists (it reads the parameters from global memory on every use), hence the few samples.  The comparison with "lds16" is a
    row of tools/glb16_table.py, not an assertion."""
    cfg = S.make_config(1984, 60, layers=list(net), track="oval")
    st = cfg["start_state"]
    sols = {}
    try:
        for v in (V, "valu_lds"):
            sols[v] = capi.Solver(cfg)
            sols[v].set_rollout_variant(v)
            for _ in range(3):  # code objects loaded, every buffer touched
                sols[v].compute_control(st)
        samples = {v: [] for v in sols}
        for block in range(2):
            for v, sol in sols.items():
                for _ in range(3):
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
        print("GLB16 speed net=%s K=1984 T=60: glb16 %.1f us, valu_lds %.1f us, ratio %.2f (6 samples each)" % (
            _id(net), med[V], med["valu_lds"], med["valu_lds"] / med[V]))
        assert med[V] <= med["valu_lds"], med
    finally:
        for sol in sols.values():
            sol.close()
