"""The "lds44" rollout form (csrc/rollout_lds44.hip): any layer list with hidden widths up to 64 on v_mfma_f32_4x4x1, the
weights of every layer read from LDS, every layer -- the output layer too -- one k-ascending chain.  The form is EXACT: its
arithmetic is the oracle's mode 1 and its bits are those of "valu_lds", the generic kernel it stands in for.
  1. every rollout of every layer list against ref64 and the mode-1 oracle on the flip-free ramp (tests/scenes.py);
  2. bit-identity with "valu_lds" (and "valu", "mfma" on the table shapes): ring, oval and ramp, explicit noise and the in-kernel
     generator, two iterations;
  3. at and beyond the resident capacity, with the largest image (one workgroup per CU) and a small one;
  4. live updates (model, cost parameters, costmap transform, a variant switch) follow "valu_lds" bit for bit;
  5. solve-ahead: armed loop, disarm, chained ticks, a two-handle batch, armed and not;
  6. refusals; 7. the hand-over hook of every role; 8. not slower than "valu_lds".
Each case prints what it measured."""
import functools

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

pytestmark = pytest.mark.gpu

U32 = np.uint32
TABLE = [[6, 32, 32, 4], [6, 32, 32, 32, 32, 4], [6, 64, 64, 4], [6, 64, 64, 64, 64, 4]]  # the shapes the other fast forms serve
NETS = [[6, 32, 32, 32, 4], [6, 64, 64, 64, 4], [6, 48, 48, 4], [6, 16, 24, 4], [6, 40, 4], [6, 64, 32, 16, 4], [6, 5, 7, 4],
        [6, 24, 4], [6, 20, 36, 52, 4], [6, 32, 32, 32, 32, 32, 32, 4], [6, 64, 64, 64, 64, 64, 64, 4]] + TABLE
SHAPES = [(64, 17), (1984, 100), (1984, 2), (1984, 300)]
LARGEST, SMALL = (6, 64, 64, 64, 64, 64, 64, 4), (6, 16, 24, 4)


def _id(net):
    return "-".join(map(str, net))


def lds44_name(net):
    return "mfma4x4x1_lds_l%d_w%d" % (len(net) - 2, max(net[1:-1]))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


@functools.lru_cache(maxsize=None)
def _cus():
    """The device's CU count, asked in a child process (torch brings a HIP runtime of its own)."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    n = int(out.stdout.split()[-1])
    assert 32 <= n <= 1024, n
    return n


def _solver(cfg, variant, U0, eps=None, seed=None, hist=None):
    sol = capi.Solver(cfg)
    if variant != "auto":
        sol.set_rollout_variant(variant)
    sol.set_control_seq(U0)
    sol.set_control_hist(np.zeros(4, np.float32) if hist is None else hist)
    if eps is not None:
        sol.set_noise(eps)
    else:
        sol.seed(seed, 0)
    return sol


def _results(sol):
    got = sol.get_results()
    got["V"] = sol.get_applied_controls()
    got["variant"] = sol.rollout_variant()
    return got


def _solve(cfg, variant, U0, eps=None, seed=None):
    sol = _solver(cfg, variant, U0, eps, seed)
    try:
        sol.compute_control(cfg["start_state"])
        return _results(sol)
    finally:
        sol.close()


def _same_bits(a, b, what, keys=("costs", "w", "V", "U")):
    for key in keys:
        np.testing.assert_array_equal(a[key].view(U32), b[key].view(U32), err_msg="%s: %s" % (what, key))
    assert np.float32(a["traj_cost"]).view(U32) == np.float32(b["traj_cost"]).view(U32), (what, a["traj_cost"], b["traj_cost"])


# ------------------------------------------------------------------------------------------------------------------ 1, 3
def _hold(tag, net, K, T):
    """The every-rollout bar of tests/test_every_rollout_gpu.py: the name, V bit-equal to the mode-1 oracle, EVERY cost within
    TOL64 of ref64 and TOL_MODE of the oracle, on costs that differ from rollout to rollout, no crash flag, no count allowance."""
    cfg = SC.ramp_config(K, T, layers=list(net))
    U0 = SC.ramp_U(cfg, seed=K % 31 + T)
    eps = noise_for(cfg, 1000 + T)
    got = _solve(cfg, "lds44", U0, eps)
    assert got["variant"] == lds44_name(net), got["variant"]
    assert oracle_mode_for(got["variant"]) == 1
    costs_o, V_o, crash_o = O.Oracle(cfg, fma_mode=1, nthreads=16).rollouts(cfg["start_state"], U0, eps[0])
    costs_r, _, crash_r = R.Ref64(cfg).rollouts(cfg["start_state"], U0, eps[0])
    assert not np.any(crash_o) and not np.any(crash_r)
    assert len(np.unique(got["costs"])) > K // 2, "the rollouts of this case are not distinct"
    np.testing.assert_array_equal(got["V"].view(U32), V_o.view(U32))
    e64, eo = rel_err(got["costs"], costs_r), rel_err(got["costs"], costs_o)
    k64, ko = int(np.argmax(e64)), int(np.argmax(eo))
    print("LDS44 %s net=%s K=%d T=%d: ref64 max %.2e (k=%d, margin x%.1f)  oracle max %.2e (k=%d), %d of %d costs bit-equal to "
          "the oracle, %d distinct" % (tag, _id(net), K, T, e64[k64], k64, TOL64 / max(e64[k64], 1e-30), eo[ko], ko,
                                       int(np.sum(got["costs"].view(U32) == costs_o.view(U32))), K, len(np.unique(got["costs"]))))
    assert float(e64[k64]) <= TOL64, ("ref64", k64, float(e64[k64]), int(np.sum(e64 > TOL64)))
    assert float(eo[ko]) <= TOL_MODE, ("oracle mode 1", ko, float(eo[ko]), int(np.sum(eo > TOL_MODE)))


@pytest.mark.parametrize("K,T", SHAPES)
@pytest.mark.parametrize("net", NETS, ids=_id)
def test_every_rollout_of_every_layer_list(net, K, T):
    _hold("every", net, K, T)


@pytest.mark.parametrize("net", [LARGEST, SMALL], ids=_id)
def test_every_rollout_at_and_beyond_the_resident_capacity(net):
    """Two groups per CU and one 64-block more; the largest image leaves room for one workgroup per CU: several rounds."""
    cap = 2 * _cus() * 16
    for K in (cap, cap + 64):
        _hold("capacity", net, K, 17)


# ------------------------------------------------------------------------------------------------------------------ 2
def _scene(track, net, **over):
    if track == "ramp":
        cfg = SC.ramp_config(512, 43, layers=list(net), **over)
        return cfg, SC.ramp_U(cfg)
    cfg = S.make_config(512, 43, layers=list(net), track=track, **over)
    return cfg, warm_U(cfg)


@pytest.mark.parametrize("net", NETS, ids=_id)
def test_bit_identical_to_the_generic_kernel(net):
    """Costs, weights, V, U and the trajectory cost of "lds44" are those of "valu_lds" as uint32: on the ring and the oval
    (crashes, thresholds) and on the ramp, with explicit noise and with the in-kernel noise wave against the stand-alone
    generator, with two iterations; on the table shapes also against "valu" and the exact MFMA form."""
    others = ["valu_lds"] + (["valu", "mfma"] if list(net) in TABLE else [])
    for track in ("ring", "oval", "ramp"):
        for iters in ((1, 2) if track == "oval" else (1,)):
            cfg, U0 = _scene(track, net, num_iters=iters)
            eps = noise_for(cfg, 4321)
            for mode, kw in (("explicit", dict(eps=eps)), ("generator", dict(seed=97))):
                got = _solve(cfg, "lds44", U0, **kw)
                assert got["variant"] == lds44_name(net)
                for v in others:
                    ref = _solve(cfg, v, U0, **kw)
                    assert ref["variant"] != got["variant"]
                    _same_bits(got, ref, "%s %s iters=%d %s vs %s" % (_id(net), track, iters, mode, v))
            print("LDS44 bits net=%s %s iters=%d: equal to %s; costs %.4g .. %.4g, %d distinct" % (
                _id(net), track, iters, others, float(got["costs"].min()), float(got["costs"].max()), len(np.unique(got["costs"]))))
            assert np.all(np.isfinite(got["costs"]))


# ------------------------------------------------------------------------------------------------------------------ 4
def _update_data(layers, theta):
    """[W1|b1|W2|b2|..] -> updateModel's [W1|W2|..|b1|b2|..]"""
    Ws, bs, off = [], [], 0
    for nin, nout in zip(layers[:-1], layers[1:]):
        Ws.append(theta[off:off + nin * nout])
        bs.append(theta[off + nin * nout:off + nin * nout + nout])
        off += nin * nout + nout
    return np.concatenate(Ws + bs).astype(np.float32)


@pytest.mark.parametrize("net", [[6, 16, 24, 4], [6, 64, 32, 16, 4], [6, 64, 64, 4]], ids=_id)
def test_live_updates_follow_the_generic_kernel(net):
    """A solve after each of mppi_update_model, mppi_set_cost_params, mppi_set_costmap_transform and a variant switch away
    and back: the LDS image follows the model -- every solve equals the same sequence on "valu_lds" bit for bit."""
    cfg, U0 = _scene("oval", net)
    eps = noise_for(cfg, 99)
    _, theta2 = P.synthetic_model(list(net), seed=11)
    cost2 = dict(cfg["cost"], desired_speed=7.5, speed_coeff=3.0, crash_coeff=8000.0)
    r_c1, r_c2, trs = np.array(cfg["r_c1"], np.float32), np.array(cfg["r_c2"], np.float32), np.array(cfg["trs"], np.float32)
    trs2 = trs.copy()
    trs2[0] += np.float32(0.004)
    trs2[1] -= np.float32(0.003)
    trace = {}
    for variant in ("lds44", "valu_lds"):
        sol = _solver(cfg, variant, U0, eps)
        out = []

        def solve():
            sol.set_control_seq(U0)
            sol.set_noise(eps)
            sol.compute_control(cfg["start_state"])
            out.append(_results(sol))
        try:
            solve()
            sol.update_model(list(net), _update_data(list(net), theta2))
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
    names = [o["variant"] for o in trace["lds44"]]
    assert names[:4] == [lds44_name(net)] * 4 and names[5] == lds44_name(net) and names[4] != lds44_name(net), names
    for i, (a, b) in enumerate(zip(trace["lds44"], trace["valu_lds"])):
        _same_bits(a, b, "%s after update %d" % (_id(net), i))
    for i in range(1, 4):  # every update changed the solve
        assert not np.array_equal(trace["lds44"][i]["costs"], trace["lds44"][i - 1]["costs"]), i


# ------------------------------------------------------------------------------------------------------------------ 5
def _tick_loop(cfg, variant, armed, n=12):
    """n ticks with a new state every tick (the nominal trajectory's next state); armed: mppi_arm before every compute."""
    sol = capi.Solver(cfg)
    sol.set_rollout_variant(variant)
    sol.seed(77, 0)
    state = np.array(cfg["start_state"], np.float32)
    out = []
    try:
        for _ in range(n):
            if armed:
                sol.arm(0.1)
                assert sol.is_armed()
            sol.compute_control(state)
            assert not sol.is_armed()
            out.append(sol.get_results())
            sol.slide_control_seq(cfg["opt_stride"])
            state = sol.nominal_traj(state)[0][1].copy()
        if armed:  # armed, called off, solved as if it never was
            sol.arm(0.1)
            assert sol.is_armed()
            sol.disarm()
            assert not sol.is_armed()
        sol.compute_control(state)
        out.append(sol.get_results())
    finally:
        sol.close()
    return out


@pytest.mark.parametrize("net,K,T", [([6, 32, 32, 32, 4], 1920, 50), ([6, 16, 24, 4], 512, 30), ([6, 64, 64, 64, 64, 64, 64, 4], 1024, 24)],
                         ids=lambda v: _id(v) if isinstance(v, list) else str(v))
def test_armed_loop_equals_the_unarmed_loop(net, K, T):
    cfg = S.make_config(K, T, layers=list(net), track="oval", opt_stride=1)
    a, b = _tick_loop(cfg, "lds44", True), _tick_loop(cfg, "lds44", False)
    for i, (x, y) in enumerate(zip(a, b)):
        _same_bits(x, y, "%s tick %d" % (_id(net), i), keys=("costs", "w", "U"))
    assert not np.array_equal(a[0]["U"], a[5]["U"])


@pytest.mark.parametrize("net,K,T,opt", [([6, 32, 32, 32, 4], 1920, 50, 1), ([6, 48, 48, 4], 256, 40, 2)],
                         ids=lambda v: _id(v) if isinstance(v, list) else str(v))
def test_chained_control_ticks_equal_the_unchained_loop(net, K, T, opt):
    cfg = S.make_config(K, T, layers=list(net), track="oval", opt_stride=opt)
    st = cfg["start_state"]
    sols = [capi.Solver(cfg) for _ in range(3)]
    try:
        for sol in sols:
            sol.set_rollout_variant("lds44")
            sol.seed(77, 0)
        sols[1].debug_set_chained_ticks(0)
        n = 12
        sols[0].control_ticks(st, n, opt)   # chained: every solve but the first armed one tick ahead
        assert not sols[0].is_armed()
        sols[1].control_ticks(st, n, opt)   # every solve launched when its turn comes
        for _ in range(n):
            sols[2].compute_control(st)
            sols[2].slide_control_seq(opt)
        res = []
        for sol in sols:
            assert sol.rollout_variant() == lds44_name(net)
            res.append((sol.get_control_seq(), sol.get_control_hist()))
            sol.compute_control(st)
            res[-1] += (sol.get_results(),)
        for U, hist, r in res[1:]:
            np.testing.assert_array_equal(res[0][0].view(U32), U.view(U32))
            np.testing.assert_array_equal(res[0][1].view(U32), hist.view(U32))
            _same_bits(res[0][2], r, "after the ticks", keys=("costs", "w", "U"))
        assert np.all(np.isfinite(res[0][2]["U"]))
    finally:
        for sol in sols:
            sol.close()


@pytest.mark.parametrize("armed", [False, True])
def test_a_batch_of_two_handles_keeps_each_handle_its_own_bits(armed):
    """Two handles with two DIFFERENT layer lists do not share a launch (two handles of one list do: tests/test_batch_wide_gpu.py):
    this batch falls back to n asynchronous solves and mppi_arm_batch arms each handle on its own."""
    nets, Ks, T = ([6, 32, 32, 32, 4], [6, 16, 24, 4]), (1920, 512), 33
    cfgs = [S.make_config(K, T, layers=list(net), track="oval", opt_stride=1, instance=i) for i, (net, K) in enumerate(zip(nets, Ks))]
    solo = []
    for i, cfg in enumerate(cfgs):
        solo.append(_solve(cfg, "lds44", warm_U(cfg), seed=500 + i))
    sols = [_solver(cfg, "lds44", warm_U(cfg), seed=500 + i) for i, cfg in enumerate(cfgs)]
    try:
        if armed:
            capi.arm_batch(sols, 0.1)
            assert all(s.is_armed() for s in sols)
        capi.compute_control_batch(sols, [cfg["start_state"] for cfg in cfgs])
        assert not any(s.is_armed() for s in sols)
        for i, s in enumerate(sols):
            got = _results(s)
            assert got["variant"] == lds44_name(nets[i])
            _same_bits(got, solo[i], "instance %d armed=%s" % (i, armed))
    finally:
        for s in sols:
            s.close()


# ------------------------------------------------------------------------------------------------------------------ 6
def test_refusals_leave_the_handle_as_it_was(golden_dir):
    import os
    bf_W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    cases = [("bf", S.make_config(256, 20, track="oval", bf_W=bf_W)),
             ("6-96-96-4", S.make_config(256, 20, layers=[6, 96, 96, 4], track="oval")),
             ("6-4", S.make_config(256, 20, layers=[6, 4], track="oval"))]
    for tag, cfg in cases:
        sol = capi.Solver(cfg)
        try:
            sol.seed(5, 0)
            before = sol.rollout_variant()
            sol.compute_control(cfg["start_state"])
            first = sol.get_results()
            with pytest.raises(capi.MppiError) as e:
                sol.set_rollout_variant("lds44")
            assert e.value.status == capi.ERR_UNSUPPORTED, (tag, e.value.status)
            assert "lds44" in str(e.value), str(e.value)
            assert sol.rollout_variant() == before
            sol.reset_controls()
            sol.seed(5, 0)
            sol.compute_control(cfg["start_state"])
            _same_bits(sol.get_results(), first, tag, keys=("costs", "w", "U"))
        finally:
            sol.close()
    cfg = S.make_config(256, 20, layers=[6, 16, 24, 4], track="oval")
    sol = capi.Solver(cfg)
    try:
        assert sol.rollout_variant() == "valu_lds"
        sol.set_rollout_variant("lds44")
        assert sol.rollout_variant() == lds44_name([6, 16, 24, 4])
        sol.set_rollout_variant("auto")
        assert sol.rollout_variant() == "valu_lds"  # the automatic choice has not changed
        assert sol.form_candidates() == ["valu_lds"]
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------------------------ 7
@pytest.mark.parametrize("wave", [1, 5, 6, 7, 8])
def test_a_starved_wave_fails_the_solve_loudly(wave):
    """Roles: 1 .. 4 dynamics waves, then pose, cost, control, noise wave (mppi_debug_inject_handover_fault): the wave's poll
    budget runs out, the solve ends in MPPI_ERR_HIP, never in finite costs; the next solve after (0, 0) is correct."""
    cfg = S.make_config(256, 40, layers=[6, 20, 36, 52, 4], track="oval")
    sol = capi.Solver(cfg)
    try:
        sol.set_rollout_variant("lds44")
        sol.compute_control(cfg["start_state"])
        good = sol.get_results()
        assert np.all(np.isfinite(good["costs"]))
        sol.debug_inject_handover_fault(wave, 32)
        with pytest.raises(capi.MppiError) as e:
            sol.compute_control(cfg["start_state"])
        assert e.value.status == capi.ERR_HIP
        sol.debug_inject_handover_fault(0, 0)
        sol.reset_controls()
        sol.seed(cfg.get("seed", 1234), 0)
        sol.compute_control(cfg["start_state"])
        again = sol.get_results()
        np.testing.assert_array_equal(again["costs"].view(U32), good["costs"].view(U32))
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------------------------ 8
@pytest.mark.parametrize("net", [[6, 32, 32, 32, 4], [6, 64, 64, 64, 4], [6, 16, 24, 4]], ids=_id)
def test_not_slower_than_the_generic_kernel(net):
    """K = 1920, T = 100: the median rollout stage (the kernel's own dispatch time, sampled every 8th solve) of 50 timed solves
    per form, the forms alternating in blocks inside one process.  The bar is "not slower" than the untouched generic kernel."""
    cfg = S.make_config(1920, 100, layers=list(net), track="oval")
    st = cfg["start_state"]
    sols = {}
    try:
        for v in ("lds44", "valu_lds"):
            sols[v] = capi.Solver(cfg)
            sols[v].set_rollout_variant(v)
            for _ in range(30):  # clocks up, code objects loaded
                sols[v].compute_control(st)
        samples = {v: [] for v in sols}
        for block in range(5):
            for v, sol in sols.items():
                for _ in range(10):
                    sol.enable_stage_timing(8)
                    sol.reset_stage_times()
                    for _ in range(8):
                        sol.compute_control(st)
                        sol.slide_control_seq(1)
                    t = sol.get_stage_times()
                    sol.enable_stage_timing(0)
                    assert t["n_solves"] == 1, t
                    samples[v].append(1e3 * t["rollout_ms"])
        med = {v: float(np.median(x)) for v, x in samples.items()}
        print("LDS44 speed net=%s K=1920 T=100: lds44 %.1f us, valu_lds %.1f us, ratio %.2f (50 samples each)" % (
            _id(net), med["lds44"], med["valu_lds"], med["valu_lds"] / med["lds44"]))
        assert med["lds44"] <= med["valu_lds"], med
    finally:
        for sol in sols.values():
            sol.close()
