"""The "row32" / "row32_tree" rollout forms (csrc/rollout_row32.hip, row_group.hpp): the row form -- the network on the vector ALU,
a rollout on a 16-lane DPP row, every weight in registers -- for every layer list of one to four hidden layers up to 32 wide, a
narrower layer padded with zero neurons.  "row32" keeps the reference's order in every layer: the oracle's mode 1, the bits of
"valu_lds" and "lds44" (one to three hidden layers); "row32_tree" sums the output layer as row_out_tree's butterfly: mode 2 (one
to four).
  1. every rollout of every list against ref64 and the oracle in the form's mode, at the smallest shapes at which the group can go
     wrong: K = 64 / 192 (4 / 12 groups, every wave and row used) x T = 2 (one step), 5 (one chunk of four), 6 (a chunk and a short
     one), 17 (the 16-slot ring wraps), 43 (several wraps, a short last chunk); once at the reference's K = 1920, T = 100;
  2. bits against existing code, never against itself: "valu_lds" and "lds44" twins; on 6-32-32-4 "row_exact" and "row_tree"; the
     tree form's controls within 1e-4 of the mode-1 oracle;
  3. over chained ticks; 4. solve-ahead and the pair; 5. live updates; 6. refusals; 7. one timing test (-m timing only).
Each case prints what it measured."""
import os

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
ONE = [[6, 32, 4], [6, 9, 4]]
TWO = [[6, 32, 32, 4], [6, 16, 24, 4]]
THREE = [[6, 32, 32, 32, 4], [6, 5, 7, 9, 4]]
FOUR = [[6, 32, 32, 32, 32, 4], [6, 20, 32, 8, 32, 4], [6, 32, 32, 32, 17, 4]]   # tree only
EXACT_NETS = ONE + TWO + THREE
CASES = [("row32", n) for n in EXACT_NETS] + [("row32_tree", n) for n in EXACT_NETS + FOUR]
TS = (2, 5, 6, 17, 43)


def _id(v):
    return "-".join(map(str, v)) if isinstance(v, (list, tuple)) else str(v)


def row32_name(form, net):
    return "valu_row8w%s_l%d_w%d" % ("_tree" if form == "row32_tree" else "", len(net) - 2, max(net[1:-1]))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


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


def _padded(cfg):
    """The problem with its LAST hidden layer zero-padded to 32 neurons (rows and biases of the layer, columns of the output
    layer): what the tree form computes, and the only width at which the oracle's mode 2 takes the butterfly."""
    layers, theta = list(cfg["layers"]), np.asarray(cfg["theta"], np.float32)
    n = layers[-2]
    if n == 32:
        return cfg
    off = sum((a + 1) * b for a, b in zip(layers[:-3], layers[1:-2]))
    nin = layers[-3]
    W = np.zeros((32, nin), np.float32)
    b = np.zeros(32, np.float32)
    W[:n] = theta[off:off + n * nin].reshape(n, nin)
    b[:n] = theta[off + n * nin:off + n * nin + n]
    off += n * nin + n
    Wo = np.zeros((4, 32), np.float32)
    Wo[:, :n] = theta[off:off + 4 * n].reshape(4, n)
    bo = theta[off + 4 * n:off + 4 * n + 4]
    assert off + 4 * n + 4 == theta.size
    theta2 = np.concatenate([theta[:off - n * nin - n], W.ravel(), b, Wo.ravel(), bo]).astype(np.float32)
    return dict(cfg, layers=layers[:-2] + [32, 4], theta=theta2)


# ------------------------------------------------------------------------------------------------------------------ 1
def _hold(form, net, K, T):
    """The every-rollout bar of tests/test_lds44_gpu.py: the name, V bit-equal to the oracle, EVERY cost within TOL64 of ref64
    and TOL_MODE of the oracle in the form's mode, on costs that differ from rollout to rollout, no crash flag, no allowance."""
    cfg = SC.ramp_config(K, T, layers=list(net))
    U0 = SC.ramp_U(cfg, seed=K % 31 + T)
    eps = noise_for(cfg, 1000 + T)
    got = _solve(cfg, form, U0, eps)
    assert got["variant"] == row32_name(form, net), got["variant"]
    mode = oracle_mode_for(got["variant"])
    assert mode == (2 if form == "row32_tree" else 1)
    costs_o, V_o, crash_o = O.Oracle(_padded(cfg) if mode == 2 else cfg, fma_mode=mode, nthreads=16).rollouts(cfg["start_state"], U0, eps[0])
    costs_r, _, crash_r = R.Ref64(cfg).rollouts(cfg["start_state"], U0, eps[0])
    assert not np.any(crash_o) and not np.any(crash_r)
    assert len(np.unique(got["costs"])) > K // 2, "the rollouts of this case are not distinct"
    np.testing.assert_array_equal(got["V"].view(U32), V_o.view(U32))
    e64, eo = rel_err(got["costs"], costs_r), rel_err(got["costs"], costs_o)
    k64, ko = int(np.argmax(e64)), int(np.argmax(eo))
    print("ROW32 %s net=%s K=%d T=%d: ref64 max %.2e (k=%d, margin x%.1f)  oracle mode %d max %.2e (k=%d), %d of %d costs bit-equal "
          "to the oracle, %d distinct" % (form, _id(net), K, T, e64[k64], k64, TOL64 / max(e64[k64], 1e-30), mode, eo[ko], ko,
                                          int(np.sum(got["costs"].view(U32) == costs_o.view(U32))), K, len(np.unique(got["costs"]))))
    assert float(e64[k64]) <= TOL64, ("ref64", k64, float(e64[k64]), int(np.sum(e64 > TOL64)))
    assert float(eo[ko]) <= TOL_MODE, ("oracle mode %d" % mode, ko, float(eo[ko]), int(np.sum(eo > TOL_MODE)))


@pytest.mark.parametrize("K", [64, 192])
@pytest.mark.parametrize("form,net", CASES, ids=_id)
def test_every_rollout_of_every_layer_list(form, net, K):
    for T in TS:
        _hold(form, net, K, T)


def test_every_rollout_at_the_reference_shape():
    _hold("row32_tree", [6, 32, 32, 32, 32, 4], 1920, 100)


# ------------------------------------------------------------------------------------------------------------------ 2
def _scene(track, net, K=512, T=43, **over):
    if track == "ramp":
        cfg = SC.ramp_config(K, T, layers=list(net), **over)
        return cfg, SC.ramp_U(cfg)
    cfg = S.make_config(K, T, layers=list(net), track=track, **over)
    return cfg, warm_U(cfg)


@pytest.mark.parametrize("net", EXACT_NETS, ids=_id)
def test_row32_has_the_bits_of_the_generic_kernel_and_of_lds44(net):
    """Costs, weights, V, U and the trajectory cost of "row32" are those of "valu_lds" and of "lds44" as uint32: on the ring and the
    oval (crashes, thresholds) and on the ramp, with explicit noise and with the in-kernel noise wave (against the stand-alone
    generator of "valu_lds"), one iteration and two; on 6-32-32-4 also those of "row_exact"."""
    others = ["valu_lds", "lds44"] + (["row_exact"] if list(net) == [6, 32, 32, 4] else [])
    for track in ("ring", "oval", "ramp"):
        for iters in (1, 2):
            cfg, U0 = _scene(track, net, num_iters=iters)
            eps = noise_for(cfg, 4321)
            for mode, kw in (("explicit", dict(eps=eps)), ("generator", dict(seed=97))):
                got = _solve(cfg, "row32", U0, **kw)
                assert got["variant"] == row32_name("row32", net)
                for v in others:
                    ref = _solve(cfg, v, U0, **kw)
                    assert ref["variant"] != got["variant"]
                    _same_bits(got, ref, "%s %s iters=%d %s vs %s" % (_id(net), track, iters, mode, v))
            print("ROW32 bits net=%s %s iters=%d: equal to %s; costs %.4g .. %.4g, %d distinct" % (
                _id(net), track, iters, others, float(got["costs"].min()), float(got["costs"].max()), len(np.unique(got["costs"]))))
            assert np.all(np.isfinite(got["costs"]))


def test_row32_tree_has_the_bits_of_row_tree_on_6_32_32_4():
    net = [6, 32, 32, 4]
    for track in ("ring", "oval", "ramp"):
        for iters in (1, 2):
            cfg, U0 = _scene(track, net, num_iters=iters)
            eps = noise_for(cfg, 4321)
            for mode, kw in (("explicit", dict(eps=eps)), ("generator", dict(seed=97))):
                got, ref = _solve(cfg, "row32_tree", U0, **kw), _solve(cfg, "row_tree", U0, **kw)
                assert got["variant"] == row32_name("row32_tree", net) and ref["variant"] == "valu_row8w_tree_h32_l2"
                _same_bits(got, ref, "%s iters=%d %s vs row_tree" % (track, iters, mode))


@pytest.mark.parametrize("net", [[6, 9, 4], [6, 32, 32, 32, 4], [6, 32, 32, 32, 32, 4], [6, 32, 32, 32, 17, 4]], ids=_id)
def test_row32_tree_controls_within_the_nominal_tolerance(net):
    """The bar of tests/test_parity_gpu.py: the tree form's U within 1e-4 of the oracle in the REFERENCE's order (mode 1), on
    identical noise, on the ramp."""
    cfg, U0 = _scene("ramp", net)
    eps = noise_for(cfg, 77)
    got = _solve(cfg, "row32_tree", U0, eps)
    ref = O.Oracle(cfg, fma_mode=1, nthreads=16).compute_control(cfg["start_state"], U0, np.zeros(4, np.float32), eps)
    du = float(np.max(np.abs(got["U"] - ref["U"])))
    print("ROW32 tree nominal net=%s: |dU|inf = %.3e" % (_id(net), du))
    assert du <= 1e-4, du


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("net", [[6, 32, 32, 32, 4], [6, 9, 4]], ids=_id)
def test_control_ticks_follow_the_generic_kernel(net):
    """Three mppi_control_ticks of four ticks with slide 1 on the generator: U, the history and the generator's stream (the solve
    after them) are those of a "valu_lds" twin."""
    cfg = S.make_config(192, 17, layers=list(net), track="oval", opt_stride=1)
    st = cfg["start_state"]
    res = {}
    for v in ("valu_lds", "row32"):
        sol = capi.Solver(cfg)
        try:
            sol.set_rollout_variant(v)
            sol.seed(77, 0)
            snaps = []
            for _ in range(3):
                sol.control_ticks(st, 4, 1)
                assert not sol.is_armed()
                snaps.append((sol.get_control_seq(), sol.get_control_hist()))
            sol.compute_control(st)
            res[v] = (snaps, sol.get_results(), sol.rollout_variant())
        finally:
            sol.close()
    assert res["row32"][2] == row32_name("row32", net) and res["valu_lds"][2] == "valu_lds"
    for (Ua, ha), (Ub, hb) in zip(res["row32"][0], res["valu_lds"][0]):
        np.testing.assert_array_equal(Ua.view(U32), Ub.view(U32))
        np.testing.assert_array_equal(ha.view(U32), hb.view(U32))
    _same_bits(res["row32"][1], res["valu_lds"][1], "after the ticks", keys=("costs", "w", "U"))
    assert not np.array_equal(res["row32"][0][0][0], res["row32"][0][2][0])


# ------------------------------------------------------------------------------------------------------------------ 4
def _tick_loop(cfg, variant, armed, n=6):
    """n ticks with a new state every tick (the nominal trajectory's next state); armed: mppi_arm before every compute."""
    sol = capi.Solver(cfg)
    sol.set_rollout_variant(variant)
    sol.seed(77, 0)
    state = np.array(cfg["start_state"], np.float32)
    out = []
    try:
        for _ in range(n):
            if armed:
                sol.arm(0.1)  # raises unless MPPI_OK
                assert sol.is_armed()
                assert sol.debug_launch_info() == (1, 1)
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


@pytest.mark.parametrize("form,net", [("row32", [6, 9, 4]), ("row32", [6, 32, 32, 32, 4]), ("row32_tree", [6, 16, 24, 4]),
                                      ("row32_tree", [6, 32, 32, 32, 32, 4])], ids=_id)
def test_armed_loop_equals_the_unarmed_loop(form, net):
    cfg = S.make_config(192, 22, layers=list(net), track="oval", opt_stride=1)
    b, a = _tick_loop(cfg, form, False), _tick_loop(cfg, form, True)
    for i, (x, y) in enumerate(zip(a, b)):
        _same_bits(x, y, "%s tick %d" % (_id(net), i), keys=("costs", "w", "U"))
    assert not np.array_equal(a[0]["U"], a[5]["U"])


@pytest.mark.parametrize("form,net", [("row32", [6, 32, 32, 32, 4]), ("row32_tree", [6, 20, 32, 8, 32, 4])], ids=_id)
def test_chained_control_ticks_equal_the_unchained_loop(form, net):
    cfg = S.make_config(192, 22, layers=list(net), track="oval", opt_stride=1)
    st = cfg["start_state"]
    sols = [capi.Solver(cfg) for _ in range(3)]
    try:
        for sol in sols:
            sol.set_rollout_variant(form)
            sol.seed(77, 0)
        sols[1].debug_set_chained_ticks(0)
        n = 6
        sols[0].control_ticks(st, n, 1)   # chained: every solve but the first armed one tick ahead
        assert not sols[0].is_armed()
        sols[1].control_ticks(st, n, 1)   # every solve launched when its turn comes
        for _ in range(n):
            sols[2].compute_control(st)
            sols[2].slide_control_seq(1)
        res = []
        for sol in sols:
            assert sol.rollout_variant() == row32_name(form, net)
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
@pytest.mark.parametrize("form,nets", [("row32", ([6, 32, 32, 32, 4], [6, 32, 32, 32, 4])), ("row32_tree", ([6, 32, 32, 32, 32, 4], [6, 32, 32, 32, 32, 4])),
                                       ("row32_tree", ([6, 9, 4], [6, 9, 4])), ("row32", ([6, 16, 24, 4], [6, 16, 24, 4])),
                                       ("row32_tree", ([6, 32, 32, 32, 4], [6, 5, 7, 9, 4]))], ids=_id)
def test_a_pair_keeps_each_handle_its_own_bits(form, nets, armed):
    """Two handles of ONE layer list share a launch (2 instances; gated when armed with mppi_arm_batch); two DIFFERENT lists solve
    per handle.  Either way every handle has the bits of its single solve.  (Two K: the smaller instance's groups return early.)"""
    Ks, T = (192, 64), 21
    same = list(nets[0]) == list(nets[1])
    cfgs = [S.make_config(K, T, layers=list(net), track="oval", opt_stride=1, instance=i) for i, (net, K) in enumerate(zip(nets, Ks))]
    solo = [_solve(cfg, form, warm_U(cfg), seed=500 + i) for i, cfg in enumerate(cfgs)]   # first: an armed kernel holds its CUs
    sols = [_solver(cfg, form, warm_U(cfg), seed=500 + i) for i, cfg in enumerate(cfgs)]
    try:
        want = (2, 1 if armed else 0) if same else (1, 1 if armed else 0)
        if armed:
            capi.arm_batch(sols, 0.1)
            assert all(s.is_armed() for s in sols)
            assert [s.debug_launch_info() for s in sols] == [want, want]
        capi.compute_control_batch(sols, [cfg["start_state"] for cfg in cfgs])
        assert not any(s.is_armed() for s in sols)
        assert [s.debug_launch_info() for s in sols] == [want, want]
        for i, s in enumerate(sols):
            got = _results(s)
            assert got["variant"] == row32_name(form, nets[i])
            _same_bits(got, solo[i], "instance %d armed=%s" % (i, armed))
    finally:
        for s in sols:
            s.close()


# ------------------------------------------------------------------------------------------------------------------ 5
def _update_data(layers, theta):
    """[W1|b1|W2|b2|..] -> updateModel's [W1|W2|..|b1|b2|..]"""
    Ws, bs, off = [], [], 0
    for nin, nout in zip(layers[:-1], layers[1:]):
        Ws.append(theta[off:off + nin * nout])
        bs.append(theta[off + nin * nout:off + nin * nout + nout])
        off += nin * nout + nout
    return np.concatenate(Ws + bs).astype(np.float32)


@pytest.mark.parametrize("net", [[6, 20, 32, 8, 32, 4], [6, 9, 4]], ids=_id)
def test_live_updates_follow_a_twin_created_with_the_new_values(net):
    """After each of mppi_update_model, mppi_set_control_limits, mppi_set_cost_params and a switch to "auto" and back, a solve on
    the "row32_tree" handle equals the solve of a fresh "row32_tree" handle created with those values (the register image follows
    the model)."""
    cfg, U0 = _scene("oval", net, K=192, T=21)
    eps = noise_for(cfg, 99)
    _, theta2 = P.synthetic_model(list(net), seed=11)
    theta2 = np.asarray(theta2, np.float32)
    lo2, hi2 = (-0.5, -0.4), (0.6, 0.5)
    cost2 = dict(cfg["cost"], desired_speed=7.5, speed_coeff=3.0, crash_coeff=8000.0)
    steps = [dict(), dict(theta=theta2), dict(theta=theta2, u_lo=lo2, u_hi=hi2), dict(theta=theta2, u_lo=lo2, u_hi=hi2, cost=cost2)]
    twins = [_solve(dict(cfg, **kw), "row32_tree", U0, eps) for kw in steps]
    sol = _solver(cfg, "row32_tree", U0, eps)
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
        sol.set_control_limits(lo2, hi2)
        solve()
        sol.set_cost_params(cost2)
        solve()
        sol.set_rollout_variant("auto")
        solve()
        sol.set_rollout_variant("row32_tree")
        solve()
    finally:
        sol.close()
    name = row32_name("row32_tree", net)
    names = [o["variant"] for o in out]
    assert names[:4] == [name] * 4 and names[4] == "valu_lds" and names[5] == name, names
    for i in range(4):
        _same_bits(out[i], twins[i], "%s after update %d" % (_id(net), i))
    _same_bits(out[5], twins[3], "%s back from auto" % _id(net))
    for i in range(1, 4):  # every update changed the solve
        assert not np.array_equal(out[i]["costs"], out[i - 1]["costs"]), i


# ------------------------------------------------------------------------------------------------------------------ 6
def test_refusals_name_the_limit_and_leave_the_handle_as_it_was(golden_dir):
    bf_W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    five = [6, 8, 8, 8, 8, 8, 4]
    cases = [("bf", S.make_config(64, 8, track="oval", bf_W=bf_W), ("row32", "row32_tree"), "network model"),
             ("width 33", S.make_config(64, 8, layers=[6, 33, 4], track="oval"), ("row32", "row32_tree"), "1..32"),
             ("five layers", S.make_config(64, 8, layers=five, track="oval"), ("row32", "row32_tree"), "one to four hidden"),
             ("row32 with four", S.make_config(64, 8, layers=[6, 32, 32, 32, 32, 4], track="oval"), ("row32",), "at most three hidden layers")]
    for tag, cfg, forms, text in cases:
        sol = capi.Solver(cfg)
        try:
            sol.seed(5, 0)
            before = sol.rollout_variant()
            sol.compute_control(cfg["start_state"])
            first = sol.get_results()
            for form in forms:
                with pytest.raises(capi.MppiError) as e:
                    sol.set_rollout_variant(form)
                assert e.value.status == capi.ERR_UNSUPPORTED, (tag, e.value.status)
                assert form in str(e.value) and text in str(e.value), (tag, str(e.value))
                assert sol.rollout_variant() == before
            assert not any("row32" in c for c in sol.form_candidates())
            sol.reset_controls()
            sol.seed(5, 0)
            sol.compute_control(cfg["start_state"])
            _same_bits(sol.get_results(), first, tag, keys=("costs", "w", "U"))
        finally:
            sol.close()
    # the standard shapes' candidates do not offer the forms either; the automatic choice is what it was
    for net, auto in (([6, 32, 32, 4], "valu_row8w_tree_h32_l2"), ([6, 32, 32, 32, 32, 4], "mfma16x16x4_h32_l4_quad4w"), ([6, 16, 24, 4], "valu_lds")):
        sol = capi.Solver(S.make_config(64, 8, layers=net, track="oval"))
        try:
            assert sol.rollout_variant() == auto
            cands = sol.form_candidates()
            sol.set_rollout_variant("row32_tree")
            assert sol.rollout_variant() == row32_name("row32_tree", net)
            assert sol.form_candidates() == cands and not any("row32" in c for c in cands)
            sol.set_rollout_variant("auto")
            assert sol.rollout_variant() == auto
        finally:
            sol.close()


def test_a_request_before_the_parameters_builds_the_image_when_they_arrive():
    import ctypes as C
    net = [6, 5, 7, 9, 4]
    cfg, U0 = _scene("oval", net, K=64, T=9)
    eps = noise_for(cfg, 3)
    want = _solve(cfg, "row32", U0, eps)
    sol = capi.Solver.__new__(capi.Solver)   # the steps of Solver.__init__, the request in front of the parameters
    sol.L, sol.cfg, sol.K, sol.T, sol.num_iters, sol.h = capi.lib(), cfg, cfg["K"], cfg["T"], 1, C.c_void_p()
    c = capi.make_config_struct(cfg, 0)
    assert sol.L.mppi_create(C.byref(c), C.byref(sol.h)) == capi.OK
    try:
        sol.set_rollout_variant("row32")
        assert sol.rollout_variant() == row32_name("row32", net)
        sol.set_nn_params(cfg["theta"])
        m = capi._f32(cfg["map_rgba"])
        sol._ck(sol.L.mppi_set_costmap(sol.h, m.shape[1], m.shape[0], capi._fp(m), capi._fp(capi._f32(cfg["r_c1"])),
                                       capi._fp(capi._f32(cfg["r_c2"])), capi._fp(capi._f32(cfg["trs"]))))
        sol.set_cost_params(cfg["cost"])
        sol.set_control_seq(U0)
        sol.set_control_hist(np.zeros(4, np.float32))
        sol.set_noise(eps)
        sol.compute_control(cfg["start_state"])
        _same_bits(_results(sol), want, "request first")
    finally:
        sol.close()


# ------------------------------------------------------------------------------------------------------------------ 7
def _medians(cfg, variants, blocks=5):
    """Median rollout stage (the kernel's own dispatch time, sampled every 8th solve) of 10 x blocks timed solves per entry of
    `variants`, the entries alternating in blocks inside one process; an entry may name a form twice (A, A')."""
    st = cfg["start_state"]
    sols = []
    try:
        for v in variants:
            sol = capi.Solver(cfg)
            if v != "auto":
                sol.set_rollout_variant(v)
            for _ in range(30):  # clocks up, code objects loaded
                sol.compute_control(st)
            sols.append(sol)
        samples = [[] for _ in sols]
        for _ in range(blocks):
            for i, sol in enumerate(sols):
                for _ in range(10):
                    sol.enable_stage_timing(8)
                    sol.reset_stage_times()
                    for _ in range(8):
                        sol.compute_control(st)
                        sol.slide_control_seq(1)
                    t = sol.get_stage_times()
                    sol.enable_stage_timing(0)
                    assert t["n_solves"] == 1, t
                    samples[i].append(1e3 * t["rollout_ms"])
        return [float(np.median(x)) for x in samples], [s.rollout_variant() for s in sols]
    finally:
        for sol in sols:
            sol.close()


@pytest.mark.timing
@pytest.mark.parametrize("form,net,incumbent", [("row32_tree", [6, 32, 32, 32, 32, 4], "auto"), ("row32", [6, 32, 32, 32, 4], "lds44")], ids=_id)
def test_faster_than_the_incumbent(form, net, incumbent):
    """K = 1920, T = 100: the new form's median rollout stage, measured twice (A, A'), is below the incumbent's by more than
    |A - A'|."""
    cfg = S.make_config(1920, 100, layers=list(net), track="oval")
    (a, b, a2), names = _medians(cfg, [form, incumbent, form])
    print("ROW32 speed net=%s K=1920 T=100: %s %.1f / %.1f us, %s (%s) %.1f us, ratio %.2f" % (
        _id(net), form, a, a2, incumbent, names[1], b, b / max(a, a2)))
    assert names[0] == names[2] == row32_name(form, net) and names[1] != names[0]
    assert b - max(a, a2) > abs(a - a2), (a, a2, b)
