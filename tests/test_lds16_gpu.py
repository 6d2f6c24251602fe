"""The "lds16" rollout form (csrc/rollout_lds16.hip): any layer list with hidden widths up to 128 whose image fits the LDS, one
wavefront per 16 rollouts on v_mfma_f32_16x16x4_f32 with the A operands read from an LDS image, every layer in the reference's
order.  The form is EXACT: its arithmetic is the oracle's mode 1 and its bits are those of "valu_lds".
  1. every rollout of every layer list against ref64 and the mode-1 oracle on the flip-free ramp (tests/scenes.py);
  2. bit-identity with "valu_lds" (and "mfma" on the table shapes): ring, oval and ramp, explicit noise and the generator, two iterations;
  3. the throughput regime: K = 16 384 and a K from the device's CU count for each workgroup size the launcher's rule has;
  4. live updates (parameters, model, cost parameters, costmap transform, a variant switch) follow "valu_lds" bit for bit;
  5. refusals; no gated form (mppi_arm); a batch of two handles; the trace of an lds16 solve;
  6. not slower than "valu_lds".
Each case prints what it measured."""
import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import params as P
from autorally_amd import synthetic as S
from oracle import oracle as O
from tests import ref64 as R
from tests import scenes as SC
from tests.helpers import noise_for, oracle_mode_for, rel_err, warm_U
from tests.scenes import TOL64, TOL_MODE
from tests.test_lds16_pack import LDS_LIMIT, image_quads, packer, workgroup_threads  # noqa: F401 (packer: a fixture)
from tests.test_lds44_gpu import _cus, _results, _same_bits, _solve, _solver, _update_data

pytestmark = pytest.mark.gpu

U32 = np.uint32
V = "lds16"
TABLE = [[6, 32, 32, 4], [6, 64, 64, 4]]
NETS = [[6, 5, 7, 4], [6, 17, 4], [6, 24, 4], [6, 16, 24, 4], [6, 48, 48, 4], [6, 32, 32, 32, 4], [6, 65, 4], [6, 33, 97, 66, 4],
        [6, 96, 96, 4], [6, 128, 128, 4], [6, 128, 128, 128, 4], [6, 16, 16, 16, 16, 16, 16, 4]] + TABLE
SHAPES = [(64, 17), (1984, 2), (1984, 60)]  # 1984 = 31 x 64: a workgroup with absent waves at 512 and 1024 threads


def _id(net):
    return "-".join(map(str, net))


def lds16_name(net):
    return "mfma16x16x4_lds_l%d_w%d" % (len(net) - 2, max(net[1:-1]))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


# ------------------------------------------------------------------------------------------------------------------ 1
def _hold(tag, net, K, T, with_ref64=True):
    """The every-rollout bar of tests/test_every_rollout_gpu.py: the name, V bit-equal to the mode-1 oracle, EVERY cost within
    TOL64 of ref64 and TOL_MODE of the oracle, on costs that differ from rollout to rollout, no crash flag, no count allowance."""
    cfg = SC.ramp_config(K, T, layers=list(net))
    U0 = SC.ramp_U(cfg, seed=K % 31 + T)
    eps = noise_for(cfg, 1000 + T)
    got = _solve(cfg, V, U0, eps)
    assert got["variant"] == lds16_name(net), got["variant"]
    assert oracle_mode_for(got["variant"]) == 1
    costs_o, V_o, crash_o = O.Oracle(cfg, fma_mode=1, nthreads=16).rollouts(cfg["start_state"], U0, eps[0])
    assert not np.any(crash_o)
    assert len(np.unique(got["costs"])) > K // 2, "the rollouts of this case are not distinct"
    np.testing.assert_array_equal(got["V"].view(U32), V_o.view(U32))
    eo = rel_err(got["costs"], costs_o)
    ko = int(np.argmax(eo))
    line = "LDS16 %s net=%s K=%d T=%d: oracle max %.2e (k=%d), %d of %d costs bit-equal to the oracle, %d distinct" % (
        tag, _id(net), K, T, eo[ko], ko, int(np.sum(got["costs"].view(U32) == costs_o.view(U32))), K, len(np.unique(got["costs"])))
    if with_ref64:
        costs_r, _, crash_r = R.Ref64(cfg).rollouts(cfg["start_state"], U0, eps[0])
        assert not np.any(crash_r)
        e64 = rel_err(got["costs"], costs_r)
        k64 = int(np.argmax(e64))
        print(line + "; ref64 max %.2e (k=%d, margin x%.1f)" % (e64[k64], k64, TOL64 / max(e64[k64], 1e-30)))
        assert float(e64[k64]) <= TOL64, ("ref64", k64, float(e64[k64]), int(np.sum(e64 > TOL64)))
    else:
        print(line)
    assert float(eo[ko]) <= TOL_MODE, ("oracle mode 1", ko, float(eo[ko]), int(np.sum(eo > TOL_MODE)))


@pytest.mark.parametrize("K,T", SHAPES)
@pytest.mark.parametrize("net", NETS, ids=_id)
def test_every_rollout_of_every_layer_list(net, K, T):
    _hold("every", net, K, T)


def test_every_rollout_of_a_long_horizon():
    _hold("long", [6, 16, 24, 4], 1984, 300)


# ------------------------------------------------------------------------------------------------------------------ 2
def _scene(track, net, **over):
    if track == "ramp":
        cfg = SC.ramp_config(512, 43, layers=list(net), **over)
        return cfg, SC.ramp_U(cfg)
    cfg = S.make_config(512, 43, layers=list(net), track=track, **over)
    return cfg, warm_U(cfg)


@pytest.mark.parametrize("net", NETS, ids=_id)
def test_bit_identical_to_the_generic_kernel(net):
    """Costs, weights, V, U and the trajectory cost of "lds16" are those of "valu_lds" as uint32: on the ring and the oval
    (crashes, thresholds) and on the ramp, with explicit noise and with the generator's draws, with two iterations; on the table
    shapes also against the exact MFMA form, whose weights stay in registers."""
    others = ["valu_lds"] + (["mfma"] if list(net) in TABLE else [])
    for track in ("ring", "oval", "ramp"):
        cfg, U0 = _scene(track, net, num_iters=2)
        eps = noise_for(cfg, 4321)
        for mode, kw in (("explicit", dict(eps=eps)), ("generator", dict(seed=97))):
            got = _solve(cfg, V, U0, **kw)
            assert got["variant"] == lds16_name(net)
            for v in others:
                ref = _solve(cfg, v, U0, **kw)
                assert ref["variant"] != got["variant"]
                _same_bits(got, ref, "%s %s %s vs %s" % (_id(net), track, mode, v))
        print("LDS16 bits net=%s %s iters=2: equal to %s; costs %.4g .. %.4g, %d distinct" % (
            _id(net), track, others, float(got["costs"].min()), float(got["costs"].max()), len(np.unique(got["costs"]))))
        assert np.all(np.isfinite(got["costs"]))


# ------------------------------------------------------------------------------------------------------------------ 3
def _throughput_cases():
    """(net, K) -> the workgroup the rule picks there: K = 16 384 on a small and on the largest image, and a K from the CU count
    for 512 threads (the largest image: one workgroup per CU) and for 1024 (a 64-wide list whose image leaves one per CU)."""
    cus = _cus()
    return [([6, 48, 48, 4], 16384), ([6, 128, 128, 128, 4], 16384), ([6, 128, 128, 128, 4], 128 * cus),
            ([6, 64, 64, 64, 64, 64, 64, 4], 256 * cus)], cus


@pytest.mark.parametrize("case", range(4))
def test_throughput_regime(case, packer):  # noqa: F811
    """The streaming tail (K > 4096), several waves per SIMD or several rounds, every workgroup size of the rule: V bit-equal to
    the mode-1 oracle and every cost within TOL_MODE of it."""
    cases, cus = _throughput_cases()
    net, K = cases[case]
    threads = [workgroup_threads(n, k, cus) for n, k in cases]
    # the library's own rule (lds16_block_threads, what the launcher calls with the handle's CU count) on this device's CUs
    assert packer(net, launch=(K, cus))[3] == threads[case], (packer(net, launch=(K, cus)), threads[case])
    print("LDS16 throughput net=%s K=%d on %d CUs: image %d bytes, %d threads per workgroup, %d workgroups (all cases: %s)" % (
        _id(net), K, cus, image_quads(net) * 16, threads[case], -(-(K // 16) // (threads[case] // 64)), threads))
    assert {256, 512, 1024} <= set(threads), threads
    _hold("throughput", net, K, 17, with_ref64=False)


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("net", [[6, 16, 24, 4], [6, 33, 97, 66, 4], [6, 64, 64, 4]], ids=_id)
def test_live_updates_follow_the_generic_kernel(net):
    """A solve after each of mppi_set_nn_params, mppi_update_model, mppi_set_cost_params, mppi_set_costmap_transform and a variant
    switch away and back: the LDS image follows the model -- every solve equals the same sequence on "valu_lds" bit for bit."""
    cfg, U0 = _scene("oval", net)
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
    assert names[:5] == [lds16_name(net)] * 5 and names[6] == lds16_name(net) and names[5] != lds16_name(net), names
    for i, (a, b) in enumerate(zip(trace[V], trace["valu_lds"])):
        _same_bits(a, b, "%s after update %d" % (_id(net), i))
    for i in range(1, 5):  # every update changed the solve
        assert not np.array_equal(trace[V][i]["costs"], trace[V][i - 1]["costs"]), i
    print("LDS16 live updates net=%s: 7 solves equal to valu_lds, names %s" % (_id(net), names))


# ------------------------------------------------------------------------------------------------------------------ 5
def test_refusals_leave_the_handle_as_it_was(golden_dir):
    import os
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
            with pytest.raises(capi.MppiError) as e:
                sol.set_rollout_variant(V)
            print("LDS16 refusal %s: status %d, %s" % (tag, e.value.status, e.value))
            assert e.value.status == capi.ERR_UNSUPPORTED, (tag, e.value.status)
            assert "lds16" in str(e.value), str(e.value)
            if tag == _id(too_big):  # needed and available bytes
                need = image_quads(too_big) * 16
                assert need > LDS_LIMIT and "%d bytes" % need in str(e.value) and "%d" % LDS_LIMIT in str(e.value), str(e.value)
            assert sol.rollout_variant() == before
            sol.reset_controls()
            sol.seed(5, 0)
            sol.compute_control(cfg["start_state"])
            _same_bits(sol.get_results(), first, tag, keys=("costs", "w", "U"))
        finally:
            sol.close()
    cfg = S.make_config(256, 20, layers=[6, 100, 72, 4], track="oval")
    sol = capi.Solver(cfg)
    try:
        assert sol.rollout_variant() == "valu_lds"
        sol.set_rollout_variant(V)
        assert sol.rollout_variant() == lds16_name([6, 100, 72, 4])
        sol.set_rollout_variant("auto")
        assert sol.rollout_variant() == "valu_lds"  # the automatic choice has not changed
        assert sol.form_candidates() == ["valu_lds"]
    finally:
        sol.close()


def test_no_gated_form_and_the_next_solve_is_an_unarmed_one():
    cfg = S.make_config(512, 30, layers=[6, 48, 48, 4], track="oval", opt_stride=1)
    sols = [capi.Solver(cfg) for _ in range(2)]
    try:
        for sol in sols:
            sol.set_rollout_variant(V)
            sol.seed(77, 0)
            sol.compute_control(cfg["start_state"])
            sol.slide_control_seq(1)
        with pytest.raises(capi.MppiError) as e:
            sols[0].arm(0.1)
        print("LDS16 arm: status %d, %s" % (e.value.status, e.value))
        assert e.value.status == capi.ERR_UNSUPPORTED
        assert not sols[0].is_armed() and sols[0].debug_launch_info() == (1, 0), "nothing was enqueued"
        res = []
        for sol in sols:
            sol.compute_control(cfg["start_state"])
            res.append(_results(sol))
        _same_bits(res[0], res[1], "after the refused arm")
        assert res[0]["variant"] == lds16_name([6, 48, 48, 4])
    finally:
        for sol in sols:
            sol.close()


def test_a_batch_of_two_handles_equals_their_single_solves():
    """No batched kernel: mppi_compute_control_batch solves the handles one by one, each in a launch of its own."""
    net, K, T = [6, 48, 48, 4], 1920, 33
    cfgs = [S.make_config(K, T, layers=list(net), track="oval", opt_stride=1, instance=i) for i in range(2)]
    solo = [_solve(cfg, V, warm_U(cfg), seed=500 + i) for i, cfg in enumerate(cfgs)]
    sols = [_solver(cfg, V, warm_U(cfg), seed=500 + i) for i, cfg in enumerate(cfgs)]
    try:
        capi.compute_control_batch(sols, [cfg["start_state"] for cfg in cfgs])
        infos = [s.debug_launch_info() for s in sols]
        print("LDS16 batch net=%s: launch info %s" % (_id(net), infos))
        assert infos == [(1, 0), (1, 0)]
        for i, s in enumerate(sols):
            got = _results(s)
            assert got["variant"] == lds16_name(net)
            _same_bits(got, solo[i], "instance %d" % i)
    finally:
        for s in sols:
            s.close()


@pytest.mark.parametrize("net", [[6, 33, 97, 66, 4], [6, 48, 48, 4]], ids=_id)
def test_the_trace_of_a_solve_has_its_costs(net):
    cfg = S.make_config(512, 43, layers=list(net), track="oval")
    sol = _solver(cfg, V, warm_U(cfg), seed=31)
    try:
        sol.compute_control(cfg["start_state"])
        got = sol.get_results()
        ks = np.arange(cfg["K"])
        tr = sol.trace_rollouts(ks)
        same = int(np.sum(tr["costs"].view(U32) == got["costs"].view(U32)))
        print("LDS16 trace net=%s: %d of %d traced costs bit-equal to the solve's, %d rollouts crash" % (
            _id(net), same, cfg["K"], int(np.sum(tr["first_crash"] >= 0))))
        np.testing.assert_array_equal(tr["costs"].view(U32), got["costs"].view(U32))
        assert sol.rollout_variant() == lds16_name(net)
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("net", [[6, 32, 32, 32, 4], [6, 128, 128, 128, 4]], ids=_id)
def test_not_slower_than_the_generic_kernel(net):
    """K = 1984, T = 60: the median rollout stage (the kernel's own dispatch time, sampled every 8th solve; every 2nd on the wide list) of 20 timed solves per
    form, the forms alternating in blocks inside one process.  The bar is "not slower" than the generic kernel -- for 6-128-128-128-4
    that is its instance that reads the parameters from global memory (they do not fit the LDS beside its tiles): a low bar."""
    cfg = S.make_config(1984, 60, layers=list(net), track="oval")
    st = cfg["start_state"]
    # the generic kernel takes 0.1 s per solve of the wide list (measured): there every 2nd solve is timed, after 10 warm-up solves
    slow = max(net) > 64
    every, warm = (2, 10) if slow else (8, 30)
    sols = {}
    try:
        for v in (V, "valu_lds"):
            sols[v] = capi.Solver(cfg)
            sols[v].set_rollout_variant(v)
            for _ in range(warm):  # clocks up, code objects loaded
                sols[v].compute_control(st)
        samples = {v: [] for v in sols}
        for block in range(2):
            for v, sol in sols.items():
                for _ in range(10):
                    sol.enable_stage_timing(every)
                    sol.reset_stage_times()
                    for _ in range(every):
                        sol.compute_control(st)
                        sol.slide_control_seq(1)
                    t = sol.get_stage_times()
                    sol.enable_stage_timing(0)
                    assert t["n_solves"] == 1, t
                    samples[v].append(1e3 * t["rollout_ms"])
        med = {v: float(np.median(x)) for v, x in samples.items()}
        print("LDS16 speed net=%s K=1984 T=60: lds16 %.1f us, valu_lds %.1f us, ratio %.2f (20 samples each)" % (
            _id(net), med[V], med["valu_lds"], med["valu_lds"] / med[V]))
        assert med[V] <= med["valu_lds"], med
    finally:
        for sol in sols.values():
            sol.close()
