"""The batched nominal replay (mppi_nominal_traj_batch -> csrc/nominal_fleet.hip): the nominal trajectories of a whole fleet in one
launch, one workgroup per controller.  Every case that claims the kernel asserts on_device == 1 (mppi_debug_nominal_info): a silent
fall-back to the host replays cannot pass.
  1. the mixed fleet of tests/nominal_cases.py against the oracle and against the single calls: control_seq bit for bit, state_seq[0]
     the bits passed in, states within 1e-4 of both (the project's state bound for these problems); distances from float64 printed,
     the device's largest at most 4 x the host call's largest;
  2. exact bits where sin / cos cannot differ (the heading stays 0): state_seq bit for bit the single call's;
  3. determinism; 4. sizes 2, 64, 65, 130 against fleets of two; 5. fall-backs: one handle, a basis-function handle, an unready handle;
     the refusals that need real handles (a handle twice, a NULL output pointer in the set);
  6. pending fleet16 solves are collected; 7. one NaN state of five; 8. ticks of a fleet16 fleet with the device replay;
  9. (timing) batch < 64 single host calls.
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
from tests import nominal_cases as NC
from tests.helpers import warm_U

pytestmark = pytest.mark.gpu

U32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_BOUND = 1e-4   # tests/test_ddp.py::test_product_matches_oracle_on_random_problems, _held of tests/test_ddp_fleet_gpu.py


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


def _close(sols):
    for s in sols:
        s.close()


def _solver(p):
    sol = capi.Solver(p["cfg"])
    sol.set_control_seq(p["U"])
    return sol


def _bits_equal(a, b, what):
    np.testing.assert_array_equal(a.view(U32), b.view(U32), err_msg=what)


def _on_device(sols):
    return [s.debug_nominal_info() for s in sols]


# ------------------------------------------------------------------------------------------------------------------ 1, 3
@functools.lru_cache(maxsize=None)
def _fleet():
    """The mixed fleet: its problems, solvers, every handle's single (host) call, the oracle's replay and the float64 replay
    (computed once, not changed)."""
    probs = NC.problems()
    sols = [_solver(p) for p in probs]
    host = [s.nominal_traj(p["x0"]) for s, p in zip(sols, probs)]
    assert _on_device(sols) == [0] * len(sols)
    orc = [O.Oracle(p["cfg"]).nominal_traj(p["x0"], p["U"]) for p in probs]
    f64 = [NC.replay64(p["cfg"], p["x0"], p["U"]) for p in probs]
    return probs, sols, host, orc, f64


def test_mixed_fleet_matches_the_oracle_and_the_single_calls():
    probs, sols, host, orc, f64 = _fleet()
    got = capi.nominal_traj_batch(sols, [p["x0"] for p in probs])
    assert _on_device(sols) == [1] * len(sols)
    same = total = 0
    dev64 = host64 = 0.0
    for i, (p, g, h, o, r) in enumerate(zip(probs, got, host, orc, f64)):
        t = NC.tag(i)
        assert np.all(np.isfinite(g[0])) and np.all(np.isfinite(g[1])), t
        e_orc, e_host = float(np.max(np.abs(g[0] - o[0]))), float(np.max(np.abs(g[0] - h[0])))
        d64, h64 = float(np.max(np.abs(g[0] - r[0]))), float(np.max(np.abs(h[0] - r[0])))
        eq = int(np.sum(g[0].view(U32) == h[0].view(U32))) + int(np.sum(g[1].view(U32) == h[1].view(U32)))
        print("NOMFLEET %s: states against the oracle %.2e, against the single call %.2e (bound 1e-4); from float64: device %.2e, "
              "host call %.2e; %d of %d output floats bit-equal to the single call" % (t, e_orc, e_host, d64, h64, eq, g[0].size + g[1].size))
        _bits_equal(g[1], h[1], t + ": control_seq")
        _bits_equal(g[1], o[1], t + ": control_seq against the oracle")
        _bits_equal(g[0][0], p["x0"], t + ": state_seq[0]")
        assert e_orc <= STATE_BOUND and e_host <= STATE_BOUND, t
        same, total = same + eq, total + g[0].size + g[1].size
        dev64, host64 = max(dev64, d64), max(host64, h64)
    print("NOMFLEET fleet: %d of %d output floats bit-equal to the single calls (%.1f %%; sinf / cosf of the heading differ by design); "
          "largest distance from float64: device %.2e, host calls %.2e" % (same, total, 100.0 * same / total, dev64, host64))
    # both are fp32 evaluations of one operation sequence, apart by at most an ulp of sin / cos in a few steps; a wrong weight,
    # order, clamp or dt shows up orders of magnitude larger
    assert dev64 <= 4.0 * host64, (dev64, host64)


def test_two_calls_in_a_row_give_the_same_bits():
    probs, sols, _, _, _ = _fleet()
    a = capi.nominal_traj_batch(sols, [p["x0"] for p in probs])
    b = capi.nominal_traj_batch(sols, [p["x0"] for p in probs])
    assert _on_device(sols) == [1] * len(sols)
    for i, (ga, gb) in enumerate(zip(a, b)):
        _bits_equal(ga[0], gb[0], NC.tag(i))
        _bits_equal(ga[1], gb[1], NC.tag(i))


# ------------------------------------------------------------------------------------------------------------------ 2
FLAT = [([6, 32, 32, 4], 50, True, True), ([6, 65, 4], 100, False, False), ([6, 200, 256, 4], 20, True, True),
        ([6, 64, 64, 64, 64, 4], 50, False, False)]


def test_exact_bits_where_the_heading_stays_zero():
    """Output neuron 3 (the yaw-rate derivative) has zero weights and bias, psi = s6 = 0 at the start: the heading stays exactly 0,
    sin / cos are 0 and 1 on both sides, and the device's states are the single call's BIT FOR BIT -- the fmaf order, the bias add,
    tanhf's bits, the clamp and the Euler step."""
    probs = [NC.make_problem(100 + i, layers, 40, hz, negate, tight, NC.base_map(), flat=True)
             for i, (layers, hz, negate, tight) in enumerate(FLAT)]
    sols = [_solver(p) for p in probs]
    try:
        host = [s.nominal_traj(p["x0"]) for s, p in zip(sols, probs)]
        got = capi.nominal_traj_batch(sols, [p["x0"] for p in probs])
        assert _on_device(sols) == [1] * len(sols)
        for i, (p, g, h) in enumerate(zip(probs, got, host)):
            t = "flat %s" % "-".join(map(str, FLAT[i][0]))
            lo, hi = np.asarray(p["cfg"]["u_lo"], np.float32), np.asarray(p["cfg"]["u_hi"], np.float32)
            assert np.any(p["U"] < lo) and np.any(p["U"] > hi), t + ": clamping fires at both limits"
            assert np.all(h[0][:, 2] == 0.0) and np.all(h[0][:, 6] == 0.0), t + ": the heading stays 0"
            assert np.ptp(h[0][:, 4]) > 1e-3 and np.ptp(h[0][:, 0]) > 1e-2, t + ": the car moves"
            diff = int(np.sum(g[0].view(U32) != h[0].view(U32)))
            print("NOMFLEET %s T=40: %d of %d state floats differ from the single call's bits" % (t, diff, g[0].size))
            _bits_equal(g[0], h[0], t + ": state_seq")
            _bits_equal(g[1], h[1], t + ": control_seq")
    finally:
        _close(sols)


# ------------------------------------------------------------------------------------------------------------------ 4, 5, 7
@functools.lru_cache(maxsize=None)
def _pool(n=130, T=5):
    """n small handles on one map (6-8-4 and 6-5-7-4 alternate; distinct states, controls, rates and models), each with its single call."""
    base_map = S.make_config(64, T, track="oval")
    sols, states, host = [], [], []
    for i in range(n):
        layers = [6, 8, 4] if i % 2 == 0 else [6, 5, 7, 4]
        l, th = P.synthetic_model(layers, seed=i % 17)
        cfg = dict(base_map, K=64, T=T, layers=l, theta=th, hz=(20, 50, 100)[i % 3], negate_yaw_der=bool(i % 5))
        st = np.array(cfg["start_state"], np.float32)
        st[2] += np.float32(0.05 * i)
        st[4] += np.float32(0.03 * i)
        st[5] += np.float32(0.01 * (i % 7))
        sol = capi.Solver(cfg)
        sol.set_control_seq(warm_U(cfg, seed=i) * np.float32(1.0 + 0.3 * (i % 9)))
        host.append(sol.nominal_traj(st))
        sols.append(sol)
        states.append(st)
    return sols, states, host


@functools.lru_cache(maxsize=None)
def _pool_in_twos():
    """Every pool handle's result in a fleet of two (handles 2 q and 2 q + 1 together)."""
    sols, states, _ = _pool()
    out = []
    for q in range(0, len(sols), 2):
        out += capi.nominal_traj_batch(sols[q:q + 2], states[q:q + 2])
        assert _on_device(sols[q:q + 2]) == [1, 1]
    return out


@pytest.mark.parametrize("n", [2, 64, 65, 130])
def test_fleet_sizes(n):
    sols, states, host = _pool()
    twos = _pool_in_twos()
    for s, st in zip(sols[:n], states[:n]):
        s.nominal_traj(st)   # a host replay last: on_device is 0 before the call
    assert _on_device(sols[:n]) == [0] * n
    got = capi.nominal_traj_batch(sols[:n], states[:n])
    assert _on_device(sols[:n]) == [1] * n
    worst = 0.0
    for i in range(n):
        _bits_equal(got[i][0], twos[i][0], "n=%d handle %d: state_seq against the fleet of two" % (n, i))
        _bits_equal(got[i][1], twos[i][1], "n=%d handle %d: control_seq against the fleet of two" % (n, i))
        _bits_equal(got[i][1], host[i][1], "n=%d handle %d: control_seq against the single call" % (n, i))
        worst = max(worst, float(np.max(np.abs(got[i][0] - host[i][0]))))
    print("NOMFLEET sizes n=%d (%d launches): every handle has the bits of its fleet of two; worst state %.2e against the single calls" % (
        n, (n + 63) // 64, worst))
    assert worst <= STATE_BOUND


def _raw_batch(sols, states, fill=9.0, null_state_seq=(), null_control_seq=()):
    """The C call on buffers filled with `fill`: (status, [(state_seq, control_seq)]).  null_*: positions whose pointer is NULL."""
    n = len(sols)
    fp = C.POINTER(C.c_float)
    hs = (C.c_void_p * n)(*[s.h for s in sols])
    st = np.ascontiguousarray(np.stack([np.asarray(x, np.float32).reshape(7) for x in states]), np.float32)
    out = [(np.full((s.T, 7), fill, np.float32), np.full((s.T, 2), fill, np.float32)) for s in sols]
    ssp = (fp * n)(*[o[0].ctypes.data_as(fp) for o in out])
    csp = (fp * n)(*[o[1].ctypes.data_as(fp) for o in out])
    for i in null_state_seq:
        ssp[i] = fp()
    for i in null_control_seq:
        csp[i] = fp()
    return sols[0].L.mppi_nominal_traj_batch(hs, st.ctypes.data_as(fp), ssp, csp, n), out


def test_one_handle_runs_on_the_host_with_the_single_calls_bits():
    sols, states, host = _pool()
    capi.nominal_traj_batch(sols[:2], states[:2])
    assert sols[0].debug_nominal_info() == 1
    got = capi.nominal_traj_batch(sols[:1], states[:1])
    assert sols[0].debug_nominal_info() == 0
    _bits_equal(got[0][0], host[0][0], "n = 1: state_seq")
    _bits_equal(got[0][1], host[0][1], "n = 1: control_seq")


def test_a_basis_function_handle_sends_the_set_to_the_host(golden_dir):
    sols, states, host = _pool()
    W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    cfg = S.make_config(64, 5, track="oval", bf_W=W)
    bf = capi.Solver(cfg)
    try:
        bf.set_control_seq(warm_U(cfg))
        alone = bf.nominal_traj(cfg["start_state"])
        capi.nominal_traj_batch(sols[:2], states[:2])
        assert sols[0].debug_nominal_info() == 1
        fleet = [sols[0], bf, sols[1]]
        got = capi.nominal_traj_batch(fleet, [states[0], cfg["start_state"], states[1]])
        assert _on_device(fleet) == [0, 0, 0]
        for g, h, what in zip(got, (host[0], alone, host[1]), ("0", "bf", "1")):
            _bits_equal(g[0], h[0], "with bf: %s state_seq" % what)
            _bits_equal(g[1], h[1], "with bf: %s control_seq" % what)
    finally:
        bf.close()


def test_an_unready_handle_fails_the_call_and_nothing_is_written():
    from tests.test_fleet16_gpu import _bare_solver
    sols, states, _ = _pool()
    cfg = S.make_config(64, 5, layers=[6, 8, 4], track="oval")
    bare = _bare_solver(cfg)
    try:
        with pytest.raises(capi.MppiError) as single:
            bare.nominal_traj(cfg["start_state"])
        capi.nominal_traj_batch(sols[:2], states[:2])
        fleet = [sols[0], sols[1], bare]   # the unready handle LAST: the two before it must not have been written either
        rc, out = _raw_batch(fleet, [states[0], states[1], cfg["start_state"]])
        assert rc == single.value.status == capi.ERR_STATE
        assert "mppi_set_nn_params" in bare.L.mppi_last_error(bare.h).decode()
        assert all(np.all(a == 9.0) and np.all(b == 9.0) for a, b in out)
        assert _on_device(sols[:2]) == [1, 1]   # nothing ran: the last replay of both is still the device's
    finally:
        bare.close()


@pytest.mark.parametrize("what", ["handle_twice", "null_state_seq", "null_control_seq"])
def test_malformed_sets_of_real_handles_are_refused_and_nothing_is_written(what):
    """The refusals that need real handles: the same handle at positions 0 and 2 of three, a NULL state_seqs[1], a NULL
    control_seqs[1] among valid handles -- MPPI_ERR_INVALID, every buffer as it was, nothing run (on_device unchanged)."""
    sols, states, _ = _pool()
    three, st = sols[20:23], states[20:23]
    capi.nominal_traj_batch(three[:2], st[:2])
    three[2].nominal_traj(st[2])
    before = _on_device(three)
    assert before == [1, 1, 0]
    if what == "handle_twice":
        rc, out = _raw_batch([three[0], three[1], three[0]], [st[0], st[1], st[0]])
    elif what == "null_state_seq":
        rc, out = _raw_batch(three, st, null_state_seq=(1,))
    else:
        rc, out = _raw_batch(three, st, null_control_seq=(1,))
    assert rc == capi.ERR_INVALID
    assert all(np.all(a == 9.0) and np.all(b == 9.0) for a, b in out)
    assert _on_device(three) == before


def test_one_nan_state_of_five_stays_alone():
    sols, states, _ = _pool()
    five, st = sols[10:15], [s.copy() for s in states[10:15]]
    four = [five[0], five[1], five[3], five[4]]
    without = capi.nominal_traj_batch(four, [st[0], st[1], st[3], st[4]])
    st[2][4] = np.float32(np.nan)
    alone = five[2].nominal_traj(st[2])
    rc, got = _raw_batch(five, st)
    assert rc == capi.OK
    assert _on_device(five) == [1] * 5
    np.testing.assert_array_equal(np.isfinite(got[2][0]), np.isfinite(alone[0]))
    assert not np.all(np.isfinite(got[2][0])) and np.any(np.isfinite(got[2][0]))
    _bits_equal(got[2][1], alone[1], "the NaN handle's control_seq")
    for g, w in zip([got[0], got[1], got[3], got[4]], without):
        _bits_equal(g[0], w[0], "beside the NaN instance: state_seq")
        _bits_equal(g[1], w[1], "beside the NaN instance: control_seq")


# ------------------------------------------------------------------------------------------------------------------ 6, 8
def _fleet16(n, base, U0, seed0):
    fleet, states = [], []
    for i in range(n):
        st = np.array(base["start_state"], np.float32)
        st[0] += np.float32(0.3 * i)
        sol = capi.Solver(dict(base, start_state=st))
        sol.set_rollout_variant("fleet16")
        sol.set_control_seq(U0)
        sol.seed(seed0 + i, 0)
        fleet.append(sol)
        states.append(st)
    return fleet, states


def test_pending_fleet16_solves_are_collected_and_the_new_controls_replayed():
    net, K, T, n = [6, 32, 32, 4], 192, 17, 3
    base = S.make_config(K, T, layers=net, track="oval")
    U0 = warm_U(base)
    fleet, states = _fleet16(n, base, U0, 900)
    try:
        capi.nominal_traj_batch(fleet, states)   # the first call on a device allocates the replay's buffers
        capi.compute_control_batch(fleet, states, blocking=False)
        assert [s.debug_launch_info() for s in fleet] == [(n, 0)] * n
        first = capi.nominal_traj_batch(fleet, states)   # collects the three pending solves
        assert _on_device(fleet) == [1] * n
        for s in fleet:
            s.synchronize()   # nothing is pending any more
        again = capi.nominal_traj_batch(fleet, states)
        lo, hi = np.asarray(base["u_lo"], np.float32), np.asarray(base["u_hi"], np.float32)
        for i, (s, a, b) in enumerate(zip(fleet, first, again)):
            Unew = s.get_results()["U"]
            assert np.any(Unew != U0), "the solve moved the control sequence"
            _bits_equal(a[1], np.clip(Unew, lo, hi), "handle %d: control_seq is the NEW sequence, clamped" % i)
            _bits_equal(a[0], b[0], "handle %d: state_seq against the replay after an explicit synchronise" % i)
            _bits_equal(a[1], b[1], "handle %d: control_seq against the replay after an explicit synchronise" % i)
        print("NOMFLEET pending: %d pending fleet16 solves collected by the call; the replay is the new sequence's" % n)
    finally:
        _close(fleet)


def test_ticks_of_a_fleet16_fleet_with_the_device_replay():
    """Three ticks: the fleet solves in shared launches and replays on the device; its twins solve and replay handle by handle on the
    host.  The control sequences agree bit for bit every tick (the replay does not touch the solve), the states stay inside the
    bound, and a handle armed on its own stream stays armed across the call."""
    net, K, T, n = [6, 32, 32, 4], 192, 17, 3
    base = S.make_config(K, T, layers=net, track="oval")
    U0 = warm_U(base)
    fleet, states = _fleet16(n, base, U0, 500)
    twins, _ = _fleet16(n, base, U0, 500)
    extra = capi.Solver(base)
    extra.set_control_seq(U0)
    extra.seed(77, 0)
    everyone, all_states = fleet + [extra], states + [np.array(base["start_state"], np.float32)]
    worst = 0.0
    try:
        capi.nominal_traj_batch(everyone, all_states)   # the first call on a device allocates the replay's buffers: not beside a gated launch
        for tick in range(3):
            extra.arm(0.05)
            assert extra.is_armed()
            capi.compute_control_batch(fleet, states)
            got = capi.nominal_traj_batch(everyone, all_states)
            assert _on_device(everyone) == [1] * (n + 1)
            assert extra.is_armed()
            for i, (s, t, st) in enumerate(zip(fleet, twins, states)):
                t.compute_control(st)
                _bits_equal(s.get_results()["U"], t.get_results()["U"], "tick %d handle %d: the control sequence" % (tick, i))
                h = t.nominal_traj(st)
                _bits_equal(got[i][1], h[1], "tick %d handle %d: control_seq" % (tick, i))
                worst = max(worst, float(np.max(np.abs(got[i][0] - h[0]))))
                s.slide_control_seq(1)
                t.slide_control_seq(1)
            extra.compute_control(all_states[-1])   # opens the armed solve
        print("NOMFLEET ticks: 3 ticks x %d handles, control sequences bit-equal to the twins'; worst state %.2e (bound 1e-4)" % (n, worst))
        assert worst <= STATE_BOUND
    finally:
        _close(everyone + twins)


# ------------------------------------------------------------------------------------------------------------------ 9
@pytest.mark.timing
def test_the_batch_beats_64_single_host_calls():
    """6-32-32-4 and 6-64-64-64-64-4, T = 100, n = 64: the median of 200 calls of the batch entry against 64 single calls on one
    host thread (tools/fleet_time.py --nominal).  Measured (MI355X): see DESIGN.md 4.21."""
    spec = importlib.util.spec_from_file_location("fleet_time", os.path.join(ROOT, "tools", "fleet_time.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    rows = [ft.nominal_ms(net, 64, T=100, calls=200) for net in ([6, 32, 32, 4], [6, 64, 64, 64, 64, 4])]
    for row in rows:
        print("NOMFLEET timing n=64 T=100 net=%s: batch %.4f ms, 64 single host calls %.4f ms, ratio %.2f" % (
            row["net"], row["batch_ms"], row["host1_ms"], row["host1_ms"] / row["batch_ms"]))
    for row in rows:
        assert row["on_device"] == 1, row
        assert row["batch_ms"] < row["host1_ms"], row
