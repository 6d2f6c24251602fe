"""The batched DDP pass (mppi_compute_feedback_gains_batch -> csrc/ddp_fleet.hip): the feedback gains of a whole fleet in one launch,
one workgroup per controller.  Every case that claims the kernel asserts on_device == 1 (mppi_debug_ddp_info): a silent fall-back to
the host passes cannot pass.
  1. the device's tanhf (csrc/tanhf_scalar.hpp) returns the host's tanhf bit for bit: 2^20 strided bit patterns and the branch edges;
  2. a mixed fleet chosen for the kernel's seams against oracle.ddp_feedback_gains, at the bounds of
     tests/test_ddp.py::test_product_matches_oracle_on_random_problems (feedback 2e-4 of its maximum, feedforward 2e-4 of
     max(1e-3, its maximum), state 1e-4, everything finite);
  3. the same fleet against n single mppi_compute_feedback_gains calls (the host path), the same bounds; the bit-equal fraction is printed;
  4. sizes: 2, 64, 65 and 130 handles (one, one, two and three launches); 1 handle, a set with a basis-function handle, a set with an
     unready handle run on the host with the single call's bits and error;
  5. one bad instance of five; 6. no interference with a fleet16 run's pending or armed solves; 7. determinism;
  8. (timing) batch < host loop at 64 handles.
Each case prints what it measured."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import params as P
from autorally_amd import synthetic as S
from oracle import oracle as O
from tests.helpers import warm_U

pytestmark = pytest.mark.gpu

U32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("feedback", "feedforward", "x", "u")


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


def _close(sols):
    for s in sols:
        s.close()


# ------------------------------------------------------------------------------------------------------------------ 1
def _libm_tanhf(x):
    libm = C.CDLL("libm.so.6")
    libm.tanhf.restype = C.c_float
    libm.tanhf.argtypes = [C.c_float]
    f = libm.tanhf
    return np.array([f(float(v)) for v in x], np.float32)


def _same_tanh_bits(x, what):
    got, ref = capi.device_tanhf(x), _libm_tanhf(x)
    bad = (got.view(U32) != ref.view(U32)) & ~(np.isnan(got) & np.isnan(ref))   # NaN payloads aside
    print("DDPFLEET tanhf %s: %d inputs, %d differ from the host's tanhf" % (what, x.size, int(bad.sum())))
    assert not bad.any(), [(hex(b), hex(g), hex(r)) for b, g, r in zip(x.view(U32)[bad][:5], got.view(U32)[bad][:5], ref.view(U32)[bad][:5])]


def test_device_tanhf_has_the_hosts_bits_on_strided_patterns():
    bits = (np.arange(1 << 20, dtype=np.uint64) * 4099 % (1 << 32)).astype(U32)   # an odd stride: every exponent, varied low bits
    _same_tanh_bits(bits.view(np.float32), "stride 4099")


def test_device_tanhf_has_the_hosts_bits_on_the_branch_edges():
    ln2 = np.log(2.0)
    # |x| at which tanhf / expm1f change path (tanhf_vec.hpp): 2|x| = 2^-25, |x| = 2^-55, 2|x| = ln2/2, 2|x| = 1.5 ln2, 1, 22 and the
    # reduction's k = 22 | 23 and 56 | 57 edges (2|x| = 22.5 ln2, 56.5 ln2); 64 patterns either side, both signs
    edges = np.array([2.0 ** -26, 2.0 ** -55, ln2 / 4, 0.75 * ln2, 1.0, 22.0, 22.5 * ln2 / 2, 56.5 * ln2 / 2, 0.5 * ln2 / 2, 1.5 * ln2 / 2,
                      2.5 * ln2 / 2, 3.5 * ln2 / 2], np.float32)
    pats = (edges.view(U32)[:, None].astype(np.int64) + np.arange(-64, 65)[None, :]).ravel().astype(U32)
    pats = np.concatenate([pats, pats | U32(0x80000000), np.array([0, 0x80000000, 1, 0x80000001, 0x7f800000, 0xff800000, 0x7f7fffff,
                                                                   0x00800000, 0x007fffff], U32)])
    _same_tanh_bits(pats.view(np.float32), "branch edges")


# ------------------------------------------------------------------------------------------------------------------ 2, 3
# layers, T, hz, negate_yaw_der, tightened limits, Qf on, targets: "given" (the nominal trajectory, passed in), "null", "off"
FLEET = [
    ([6, 4], 2, 20, True, False, False, "given"),
    ([6, 24, 4], 3, 50, False, True, True, "null"),
    ([6, 5, 7, 4], 5, 100, True, False, True, "off"),
    ([6, 32, 32, 4], 17, 50, True, True, False, "off"),
    ([6, 64, 64, 4], 40, 20, False, False, True, "null"),
    ([6, 65, 4], 17, 100, True, False, False, "given"),
    ([6, 8, 8, 8, 8, 8, 4], 40, 50, False, True, True, "off"),
    ([6, 128, 129, 4], 5, 20, True, False, True, "null"),
    ([6, 200, 256, 4], 17, 100, False, True, False, "off"),
    ([6, 32, 32, 4], 250, 100, True, False, True, "off"),
    ([6, 64, 64, 64, 64, 4], 3, 50, True, False, False, "null"),
]


def _problem(i, layers, T, hz, negate, tight, qf_on, tmode, base_map):
    """Instance i, drawn as test_product_matches_oracle_on_random_problems draws: start state, control sequence, DDP weights with
    zero entries in Q."""
    rng = np.random.RandomState(7000 + i)
    over = dict(negate_yaw_der=negate, hz=hz)
    if tight:
        over.update(u_lo=(-0.6, -0.3), u_hi=(0.7, 0.4))
    l, th = P.synthetic_model(list(layers), seed=int(rng.randint(100)))
    cfg = dict(base_map, K=64, T=T, layers=l, theta=th, **over)
    x0 = np.array(cfg["start_state"], np.float32).copy()
    x0[4], x0[5], x0[6] = rng.uniform(0.05, 12), rng.uniform(-1, 1), rng.uniform(-1.5, 1.5)
    x0[3], x0[2] = rng.uniform(-0.2, 0.2), rng.uniform(-3, 3)
    U = np.clip(warm_U(cfg, seed=i) * rng.uniform(0.2, 2.0), cfg["u_lo"], cfg["u_hi"]).astype(np.float32)
    Q = (rng.uniform(0, 1, 7) * (rng.rand(7) < 0.8)).astype(np.float32)
    Q[(i + 3) % 7] = 0.0   # a zero entry in every instance
    R = rng.uniform(0.5, 20, 2).astype(np.float32)
    Qf = (rng.uniform(0, 2, 7) * (1.0 if qf_on else 0.0)).astype(np.float32)
    orc = O.Oracle(cfg)
    xs, us = orc.nominal_traj(x0, U)
    if tmode == "off":
        tx = xs + rng.normal(0, 0.1, xs.shape).astype(np.float32)
        ref = orc.ddp_feedback_gains(x0, tx, us, Q, R, Qf)
        targets = (tx, us)
    else:
        ref = orc.ddp_feedback_gains(x0, xs, us, Q, R, Qf)
        targets = (xs, us) if tmode == "given" else None
    return dict(cfg=cfg, x0=x0, U=U, Q=Q, R=R, Qf=Qf, targets=targets, ref=ref)


@functools.lru_cache(maxsize=None)
def _fleet():
    """The mixed fleet's problems with the oracle's results, its solvers, and every handle's host pass (computed once, not changed)."""
    base_map = S.make_config(64, 5, track="oval")
    probs = [_problem(i, *row, base_map) for i, row in enumerate(FLEET)]
    sols = []
    host = []
    for p in probs:
        sol = capi.Solver(p["cfg"])
        sol.set_control_seq(p["U"])
        sol.set_ddp_weights(p["Q"], p["R"], p["Qf"])
        t = p["targets"]
        host.append(sol.compute_feedback_gains(p["x0"], *(t if t is not None else (None, None))))
        assert sol.debug_ddp_info() == 0
        sols.append(sol)
    return probs, sols, host


def _held(got, ref, tag):
    """The bounds of test_product_matches_oracle_on_random_problems; returns the three errors relative to their bounds' scales."""
    assert all(np.all(np.isfinite(got[k])) for k in KEYS) and np.isfinite(got["total_cost"]), tag
    efb = np.max(np.abs(got["feedback"] - ref["feedback"])) / max(np.abs(ref["feedback"]).max(), 1e-6)
    eff = np.max(np.abs(got["feedforward"] - ref["feedforward"])) / max(1e-3, np.abs(ref["feedforward"]).max())
    ex = np.max(np.abs(got["x"] - ref["x"]))
    print("DDPFLEET %s: feedback %.2e (bound 2e-4)  feedforward %.2e (2e-4)  state %.2e (1e-4)" % (tag, efb, eff, ex))
    assert efb <= 2e-4, tag
    assert eff <= 2e-4, tag
    assert ex <= 1e-4, tag
    return efb, eff, ex


def _batch(sols, probs):
    capi.compute_feedback_gains_batch(sols, [p["x0"] for p in probs], [p["targets"] for p in probs])
    return [s.feedback_gains() for s in sols]


def test_mixed_fleet_matches_the_oracle():
    probs, sols, _ = _fleet()
    got = _batch(sols, probs)
    assert [s.debug_ddp_info() for s in sols] == [1] * len(sols)
    for i, (p, g) in enumerate(zip(probs, got)):
        _held(g, p["ref"], "oracle %d %s T=%d" % (i, "-".join(map(str, FLEET[i][0])), FLEET[i][1]))
        assert np.all(g["u"][-1] == 0.0) and np.all(g["feedback"][-1] == 0.0) and np.all(g["feedforward"][-1] == 0.0)


def test_mixed_fleet_matches_the_host_path():
    probs, sols, host = _fleet()
    got = _batch(sols, probs)
    assert [s.debug_ddp_info() for s in sols] == [1] * len(sols)
    same = total = 0
    for i, (h, g) in enumerate(zip(host, got)):
        _held(g, h, "host %d %s T=%d" % (i, "-".join(map(str, FLEET[i][0])), FLEET[i][1]))
        assert abs(g["total_cost"] - h["total_cost"]) <= 2e-4 * max(1.0, abs(h["total_cost"]))
        for k in KEYS:
            same += int(np.sum(g[k].view(U32) == h[k].view(U32)))
            total += g[k].size
    print("DDPFLEET host path: %d of %d output floats bit-equal to the single calls (%.1f %%; sinf / cosf of the heading differ by "
          "design)" % (same, total, 100.0 * same / total))


def test_two_calls_in_a_row_give_the_same_bits():
    probs, sols, _ = _fleet()
    a = _batch(sols, probs)
    b = _batch(sols, probs)
    for ga, gb in zip(a, b):
        for k in KEYS:
            np.testing.assert_array_equal(ga[k].view(U32), gb[k].view(U32))
        assert np.float32(ga["total_cost"]).view(U32) == np.float32(gb["total_cost"]).view(U32)


# ------------------------------------------------------------------------------------------------------------------ 4
@functools.lru_cache(maxsize=None)
def _pool(n=130, T=5):
    """n small handles on one map (6-8-4 and 6-5-7-4 alternate; distinct states, controls and models), each with its host pass."""
    base_map = S.make_config(64, T, track="oval")
    sols, states, host = [], [], []
    for i in range(n):
        layers = [6, 8, 4] if i % 2 == 0 else [6, 5, 7, 4]
        l, th = P.synthetic_model(layers, seed=i % 17)
        cfg = dict(base_map, K=64, T=T, layers=l, theta=th, hz=(20, 50, 100)[i % 3])
        st = np.array(cfg["start_state"], np.float32)
        st[2] += np.float32(0.05 * i)
        st[4] += np.float32(0.03 * i)
        st[5] += np.float32(0.01 * (i % 7))
        sol = capi.Solver(cfg)
        sol.set_control_seq(warm_U(cfg, seed=i))
        host.append(sol.compute_feedback_gains(st))
        sols.append(sol)
        states.append(st)
    return sols, states, host


@pytest.mark.parametrize("n", [2, 64, 65, 130])
def test_fleet_sizes(n):
    sols, states, host = _pool()
    for s in sols[:n]:
        s.compute_feedback_gains(states[0])   # a host pass last: on_device is 0 before the call
    assert [s.debug_ddp_info() for s in sols[:n]] == [0] * n
    capi.compute_feedback_gains_batch(sols[:n], states[:n])
    assert [s.debug_ddp_info() for s in sols[:n]] == [1] * n
    worst = np.zeros(3)
    for i in range(n):
        g, h = sols[i].feedback_gains(), host[i]
        assert all(np.all(np.isfinite(g[k])) for k in KEYS)
        worst = np.maximum(worst, [np.max(np.abs(g["feedback"] - h["feedback"])) / max(np.abs(h["feedback"]).max(), 1e-6),
                                   np.max(np.abs(g["feedforward"] - h["feedforward"])) / max(1e-3, np.abs(h["feedforward"]).max()),
                                   np.max(np.abs(g["x"] - h["x"]))])
    print("DDPFLEET sizes n=%d (%d launches): worst feedback %.2e feedforward %.2e state %.2e against the single calls" % (
        n, (n + 63) // 64, *worst))
    assert worst[0] <= 2e-4 and worst[1] <= 2e-4 and worst[2] <= 1e-4


def _same_as(got, ref, what):
    for k in KEYS:
        np.testing.assert_array_equal(got[k].view(U32), ref[k].view(U32), err_msg="%s: %s" % (what, k))
    assert np.float32(got["total_cost"]).view(U32) == np.float32(ref["total_cost"]).view(U32), what


def test_one_handle_runs_on_the_host_with_the_single_calls_bits():
    sols, states, host = _pool()
    capi.compute_feedback_gains_batch(sols[:2], states[:2])
    assert sols[0].debug_ddp_info() == 1
    capi.compute_feedback_gains_batch(sols[:1], states[:1])
    assert sols[0].debug_ddp_info() == 0
    _same_as(sols[0].feedback_gains(), host[0], "n = 1")


def test_a_basis_function_handle_sends_the_set_to_the_host(golden_dir):
    sols, states, host = _pool()
    W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    cfg = S.make_config(64, 5, track="oval", bf_W=W)
    bf = capi.Solver(cfg)
    try:
        bf.set_control_seq(warm_U(cfg))
        alone = bf.compute_feedback_gains(cfg["start_state"])
        capi.compute_feedback_gains_batch(sols[:2], states[:2])
        assert sols[0].debug_ddp_info() == 1
        fleet = [sols[0], bf, sols[1]]
        capi.compute_feedback_gains_batch(fleet, [states[0], cfg["start_state"], states[1]])
        assert [s.debug_ddp_info() for s in fleet] == [0, 0, 0]
        _same_as(sols[0].feedback_gains(), host[0], "with bf: 0")
        _same_as(bf.feedback_gains(), alone, "with bf: bf")
        _same_as(sols[1].feedback_gains(), host[1], "with bf: 1")
    finally:
        bf.close()


def test_an_unready_handle_sends_the_set_to_the_host_with_the_single_calls_error():
    from tests.test_fleet16_gpu import _bare_solver
    sols, states, host = _pool()
    cfg = S.make_config(64, 5, layers=[6, 8, 4], track="oval")
    bare = _bare_solver(cfg)
    try:
        with pytest.raises(capi.MppiError) as single:
            bare.compute_feedback_gains(cfg["start_state"])
        capi.compute_feedback_gains_batch(sols[:2], states[:2])
        fleet = [sols[0], bare, sols[1]]
        with pytest.raises(capi.MppiError) as batch:
            capi.compute_feedback_gains_batch(fleet, [states[0], cfg["start_state"], states[1]])
        assert batch.value.status == single.value.status == capi.ERR_STATE
        assert "mppi_set_nn_params" in str(batch.value)
        assert [s.debug_ddp_info() for s in (sols[0], sols[1])] == [0, 0]
        _same_as(sols[0].feedback_gains(), host[0], "with an unready handle: 0")
        _same_as(sols[1].feedback_gains(), host[1], "with an unready handle: 1")
        with pytest.raises(capi.MppiError):
            bare.feedback_gains()
    finally:
        bare.close()


# ------------------------------------------------------------------------------------------------------------------ 5
def test_one_bad_instance_fails_alone():
    sols, states, _ = _pool()
    five, st = sols[10:15], [s.copy() for s in states[10:15]]
    four = [five[0], five[1], five[3], five[4]]
    capi.compute_feedback_gains_batch(four, [st[0], st[1], st[3], st[4]])
    assert [s.debug_ddp_info() for s in four] == [1] * 4
    without = [s.feedback_gains() for s in four]
    st[2][4] = np.float32(np.nan)
    with pytest.raises(capi.MppiError) as e:
        capi.compute_feedback_gains_batch(five, st)
    assert e.value.status == capi.ERR_STATE
    assert "factorised" in five[2].L.mppi_last_error(five[2].h).decode()   # the bad handle's own message
    assert [s.debug_ddp_info() for s in five] == [1] * 5
    with pytest.raises(capi.MppiError):
        five[2].feedback_gains()
    for s, w in zip(four, without):
        _same_as(s.feedback_gains(), w, "beside the bad instance")


# ------------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("armed", [False, True], ids=["pending", "one_armed"])
def test_a_batched_pass_leaves_a_fleet16_run_alone(armed):
    """Three ticks of a fleet16 fleet with a batched DDP pass between mppi_compute_control_batch_async and its collection: U and
    the costs of the same run without DDP, bit for bit.  one_armed: a fourth handle (a latency form) is armed and takes part in the pass."""
    net, K, T, n = [6, 32, 32, 4], 192, 17, 3
    base = S.make_config(K, T, layers=net, track="oval")
    U0 = warm_U(base)

    def run(with_ddp):
        fleet, states = [], []
        for i in range(n):
            st = np.array(base["start_state"], np.float32)
            st[0] += np.float32(0.3 * i)
            sol = capi.Solver(dict(base, start_state=st))
            sol.set_rollout_variant("fleet16")
            sol.set_control_seq(U0)
            sol.seed(900 + i, 0)
            fleet.append(sol)
            states.append(st)
        extra = capi.Solver(base)
        extra.set_control_seq(U0)
        extra.seed(77, 0)
        out = []
        try:
            # targets are given: a pass without them replays the nominal trajectory, which collects the handle's pending solve
            tg = []
            for s, st in zip(fleet + [extra], states + [base["start_state"]]):
                tg.append(s.nominal_traj(st))
            if with_ddp:  # the first pass on a device allocates the pass's buffers: not beside a gated launch
                capi.compute_feedback_gains_batch(fleet + [extra], states + [base["start_state"]], tg)
            for tick in range(3):
                if armed:
                    extra.arm(0.05)
                    assert extra.is_armed()
                capi.compute_control_batch(fleet, states, blocking=False)
                if with_ddp:
                    capi.compute_feedback_gains_batch(fleet + [extra], states + [base["start_state"]], tg)
                    assert [s.debug_ddp_info() for s in fleet + [extra]] == [1] * (n + 1)
                    if armed:
                        assert extra.is_armed()
                for s in fleet:
                    s.synchronize()
                    assert s.debug_launch_info() == (n, 0)
                    r = s.get_results()
                    out.append((r["U"].copy(), r["costs"].copy()))
                    s.slide_control_seq(1)
                if armed:  # the armed solve opens with this state (or, had its gate's deadline passed, is solved afresh: the same bits)
                    extra.compute_control(base["start_state"])
                    r = extra.get_results()
                    out.append((r["U"].copy(), r["costs"].copy()))
        finally:
            _close(fleet + [extra])
        return out

    a, b = run(False), run(True)
    assert len(a) == len(b)
    for (Ua, ca), (Ub, cb) in zip(a, b):
        np.testing.assert_array_equal(Ua.view(U32), Ub.view(U32))
        np.testing.assert_array_equal(ca.view(U32), cb.view(U32))
    print("DDPFLEET no interference (%s): %d result sets bit-equal with and without the batched pass" % ("one armed" if armed else "pending", len(a)))


# ------------------------------------------------------------------------------------------------------------------ 8
@pytest.mark.timing
def test_the_batch_beats_the_host_loop_at_64_handles():
    """6-32-32-4 and 6-64-64-64-64-4, T = 100, n = 2, 4, 16, 64: the median of 200 calls of the batch entry against n single calls
    with one host thread and against the pair entry with two (tools/fleet_time.py --ddp).  The bar is the feature's claim alone:
    batch < host loop at n = 64 on both networks.  Measured (MI355X): see DESIGN.md 4.20."""
    spec = importlib.util.spec_from_file_location("fleet_time", os.path.join(ROOT, "tools", "fleet_time.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    rows = ft.ddp_table([[6, 32, 32, 4], [6, 64, 64, 64, 64, 4]])
    for row in rows:
        if row["n"] == 64:
            assert row["on_device"] == 1, row
            assert row["batch_ms"] < row["host1_ms"] and row["batch_ms"] < row["host2_ms"], row
