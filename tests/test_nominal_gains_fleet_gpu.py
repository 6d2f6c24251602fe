"""The fused closing stages of a fleet's tick (mppi_nominal_and_gains_batch -> csrc/nominal_gains_fleet.hip): per controller the
nominal replay and the DDP pass that tracks it in one workgroup of one launch.  Every case that claims the kernel asserts fused == 1
(mppi_debug_nominal_and_gains_info): a silent fall-back to the two calls cannot pass.
  1. the mixed fleet of tests/nominal_gains_cases.py in one call: state_seqs / control_seqs BIT FOR BIT mppi_nominal_traj_batch's on
     twin handles; feedback, feedforward, x, u and the total cost (what mppi_get_feedback_gains returns; the per-step costs are not
     part of the getter: their k-ascending sum, the total cost, stands for them) BIT FOR BIT mppi_compute_feedback_gains_batch's
     on the twins with the replay's outputs as targets; the same outputs against the oracle and the float64 replay at the bounds of
     tests/test_nominal_fleet_gpu.py (control_seq exact, states 1e-4, the distance from float64 at most 4 x the host call's) and of
     tests/test_ddp_fleet_gpu.py::_held (feedback 2e-4, feedforward 2e-4, state 1e-4);
  2. determinism; 3. sizes 2, 64, 65, 130 against fleets of two; 4. fall-backs: one handle, a basis-function handle, an unready handle;
  5. one NaN state of five; 6. the refusals that need real handles; 7. ticks of a fleet16 fleet closed with the call, one handle
     armed; 8. pending solves are collected; 9. (timing) the call against the two calls at 64 handles.
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
from tests import nominal_cases as NC
from tests import nominal_gains_cases as NG
from tests.helpers import warm_U

pytestmark = pytest.mark.gpu

U32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("feedback", "feedforward", "x", "u")
STATE_BOUND = 1e-4   # tests/test_nominal_fleet_gpu.py


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


def _close(sols):
    for s in sols:
        s.close()


def _bits_equal(a, b, what):
    np.testing.assert_array_equal(a.view(U32), b.view(U32), err_msg=what)


def _same_gains(got, ref, what):
    for k in KEYS:
        _bits_equal(got[k], ref[k], "%s: %s" % (what, k))
    assert np.float32(got["total_cost"]).view(U32) == np.float32(ref["total_cost"]).view(U32), what + ": total cost"


def _same_seqs(got, ref, what):
    _bits_equal(got[0], ref[0], what + ": state_seq")
    _bits_equal(got[1], ref[1], what + ": control_seq")


def _fused(sols):
    return [s.debug_nominal_and_gains_info() for s in sols]


def _two_calls(sols, states):
    """The two existing calls in sequence, the second with the first one's outputs as targets: ([(state_seq, control_seq)], [gains])."""
    seqs = capi.nominal_traj_batch(sols, states)
    capi.compute_feedback_gains_batch(sols, states, seqs)
    return seqs, [s.feedback_gains() for s in sols]


def _held(got, ref, tag):
    """tests/test_ddp_fleet_gpu.py::_held, its bounds (test_product_matches_oracle_on_random_problems)."""
    assert all(np.all(np.isfinite(got[k])) for k in KEYS) and np.isfinite(got["total_cost"]), tag
    efb = np.max(np.abs(got["feedback"] - ref["feedback"])) / max(np.abs(ref["feedback"]).max(), 1e-6)
    eff = np.max(np.abs(got["feedforward"] - ref["feedforward"])) / max(1e-3, np.abs(ref["feedforward"]).max())
    ex = np.max(np.abs(got["x"] - ref["x"]))
    print("NOMGAINS %s: feedback %.2e (bound 2e-4)  feedforward %.2e (2e-4)  state %.2e (1e-4)" % (tag, efb, eff, ex))
    assert efb <= 2e-4, tag
    assert eff <= 2e-4, tag
    assert ex <= 1e-4, tag


# ------------------------------------------------------------------------------------------------------------------ 1, 2
def _solver(p):
    sol = capi.Solver(p["cfg"])
    sol.set_control_seq(p["U"])
    sol.set_ddp_weights(p["Q"], p["R"], p["Qf"])
    return sol


@functools.lru_cache(maxsize=None)
def _fleet():
    """The mixed fleet: its problems, solvers, and the twins' results of the two calls in sequence and of their single host replays
    (computed once, not changed)."""
    probs = NG.problems()
    sols, twins = [_solver(p) for p in probs], [_solver(p) for p in probs]
    states = [p["x0"] for p in probs]
    host = [t.nominal_traj(p["x0"]) for t, p in zip(twins, probs)]
    seqs, gains = _two_calls(twins, states)
    assert [t.debug_nominal_info() for t in twins] == [1] * len(twins) and [t.debug_ddp_info() for t in twins] == [1] * len(twins)
    return probs, sols, states, seqs, gains, host


def test_mixed_fleet_has_the_bits_of_the_two_calls():
    probs, sols, states, seqs, gains, _ = _fleet()
    got = capi.nominal_and_gains_batch(sols, states)
    assert _fused(sols) == [1] * len(sols)
    for i, (s, g, q, w) in enumerate(zip(sols, got, seqs, gains)):
        _same_seqs(g, q, NC.tag(i))
        _same_gains(s.feedback_gains(), w, NC.tag(i))
    print("NOMGAINS fleet: %d handles, sequences and gains bit-equal to mppi_nominal_traj_batch + mppi_compute_feedback_gains_batch" % len(sols))


def test_mixed_fleet_matches_the_oracle_and_float64():
    probs, sols, states, _, _, host = _fleet()
    orc = NG.oracle_results()
    got = capi.nominal_and_gains_batch(sols, states)
    assert _fused(sols) == [1] * len(sols)
    dev64 = host64 = 0.0
    for i, (p, s, g, h, (oxs, ous, oref)) in enumerate(zip(probs, sols, got, host, orc)):
        t = NC.tag(i)
        r = NC.replay64(p["cfg"], p["x0"], p["U"])
        assert np.all(np.isfinite(g[0])) and np.all(np.isfinite(g[1])), t
        e_orc = float(np.max(np.abs(g[0] - oxs)))
        d64, h64 = float(np.max(np.abs(g[0] - r[0]))), float(np.max(np.abs(h[0] - r[0])))
        print("NOMGAINS %s: states against the oracle %.2e (bound 1e-4); from float64: device %.2e, host call %.2e" % (t, e_orc, d64, h64))
        _bits_equal(g[1], ous, t + ": control_seq against the oracle")
        _bits_equal(g[0][0], p["x0"], t + ": state_seq[0]")
        assert e_orc <= STATE_BOUND, t
        dev64, host64 = max(dev64, d64), max(host64, h64)
        gains = s.feedback_gains()
        _held(gains, oref, "oracle " + t)
        assert np.all(gains["u"][-1] == 0.0) and np.all(gains["feedback"][-1] == 0.0) and np.all(gains["feedforward"][-1] == 0.0)
    print("NOMGAINS fleet: largest distance from float64: device %.2e, host calls %.2e" % (dev64, host64))
    assert dev64 <= 4.0 * host64, (dev64, host64)   # tests/test_nominal_fleet_gpu.py's bound and its reason


def test_two_calls_in_a_row_give_the_same_bits():
    probs, sols, states, _, _, _ = _fleet()
    a = capi.nominal_and_gains_batch(sols, states)
    ga = [s.feedback_gains() for s in sols]
    b = capi.nominal_and_gains_batch(sols, states)
    assert _fused(sols) == [1] * len(sols)
    for i, (s, qa, qb, g) in enumerate(zip(sols, a, b, ga)):
        _same_seqs(qa, qb, NC.tag(i))
        _same_gains(s.feedback_gains(), g, NC.tag(i))


# ------------------------------------------------------------------------------------------------------------------ 3, 4, 5, 6
@functools.lru_cache(maxsize=None)
def _pool(n=130, T=5):
    """n small handles on one map (6-8-4 and 6-5-7-4 alternate; distinct states, controls, rates and models)."""
    base_map = S.make_config(64, T, track="oval")
    sols, states = [], []
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
        sols.append(sol)
        states.append(st)
    return sols, states


@functools.lru_cache(maxsize=None)
def _pool_in_twos():
    """Every pool handle's result of the new call in a fleet of two (handles 2 q and 2 q + 1 together)."""
    sols, states = _pool()
    seqs, gains = [], []
    for q in range(0, len(sols), 2):
        seqs += capi.nominal_and_gains_batch(sols[q:q + 2], states[q:q + 2])
        assert _fused(sols[q:q + 2]) == [1, 1]
        gains += [s.feedback_gains() for s in sols[q:q + 2]]
    return seqs, gains


@pytest.mark.parametrize("n", [2, 64, 65, 130])
def test_fleet_sizes(n):
    sols, states = _pool()
    seqs2, gains2 = _pool_in_twos()
    for s, st in zip(sols[:n], states[:n]):
        capi.nominal_and_gains_batch([s], [st])   # a call of one last: the two calls on the host, fused is 0 before the call
    assert _fused(sols[:n]) == [0] * n
    got = capi.nominal_and_gains_batch(sols[:n], states[:n])
    assert _fused(sols[:n]) == [1] * n
    for i in range(n):
        _same_seqs(got[i], seqs2[i], "n=%d handle %d against the fleet of two" % (n, i))
        _same_gains(sols[i].feedback_gains(), gains2[i], "n=%d handle %d against the fleet of two" % (n, i))
    print("NOMGAINS sizes n=%d (%d launches): every handle has the bits of its fleet of two" % (n, (n + 63) // 64))


def _raw(sols, states, fill=9.0, null_state_seq=(), null_control_seq=()):
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
    return sols[0].L.mppi_nominal_and_gains_batch(hs, st.ctypes.data_as(fp), ssp, csp, n), out


def test_one_handle_runs_the_two_calls():
    sols, states = _pool()
    capi.nominal_and_gains_batch(sols[:2], states[:2])
    assert _fused(sols[:2]) == [1, 1]
    seqs, gains = _two_calls(sols[:1], states[:1])   # n = 1: both on the host
    got = capi.nominal_and_gains_batch(sols[:1], states[:1])
    assert _fused(sols[:1]) == [0] and sols[0].debug_nominal_info() == 0 and sols[0].debug_ddp_info() == 0
    _same_seqs(got[0], seqs[0], "n = 1")
    _same_gains(sols[0].feedback_gains(), gains[0], "n = 1")


def test_a_basis_function_handle_sends_the_set_to_the_two_calls(golden_dir):
    sols, states = _pool()
    W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    cfg = S.make_config(64, 5, track="oval", bf_W=W)
    bf = capi.Solver(cfg)
    try:
        bf.set_control_seq(warm_U(cfg))
        capi.nominal_and_gains_batch(sols[:2], states[:2])
        assert _fused(sols[:2]) == [1, 1]
        fleet, st = [sols[0], bf, sols[1]], [states[0], cfg["start_state"], states[1]]
        seqs, gains = _two_calls(fleet, st)
        got = capi.nominal_and_gains_batch(fleet, st)
        assert _fused(fleet) == [0, 0, 0]
        assert [s.debug_nominal_info() for s in fleet] == [0, 0, 0] and [s.debug_ddp_info() for s in fleet] == [0, 0, 0]
        for s, g, q, w, what in zip(fleet, got, seqs, gains, ("0", "bf", "1")):
            _same_seqs(g, q, "with bf: " + what)
            _same_gains(s.feedback_gains(), w, "with bf: " + what)
    finally:
        bf.close()


def test_an_unready_handle_fails_as_the_two_calls_do_and_nothing_is_written():
    from tests.test_fleet16_gpu import _bare_solver
    sols, states = _pool()
    cfg = S.make_config(64, 5, layers=[6, 8, 4], track="oval")
    bare = _bare_solver(cfg)
    try:
        capi.nominal_and_gains_batch(sols[:2], states[:2])
        before = [s.feedback_gains() for s in sols[:2]]
        fleet, st = [sols[0], sols[1], bare], [states[0], states[1], cfg["start_state"]]
        with pytest.raises(capi.MppiError) as two:   # the first of the two calls refuses the set
            capi.nominal_traj_batch(fleet, st)
        rc, out = _raw(fleet, st)
        assert rc == two.value.status == capi.ERR_STATE
        assert "mppi_set_nn_params" in bare.L.mppi_last_error(bare.h).decode()
        assert all(np.all(a == 9.0) and np.all(b == 9.0) for a, b in out)
        assert _fused(fleet) == [0, 0, 0]
        for s, b in zip(sols[:2], before):   # nothing ran: the earlier gains stand
            _same_gains(s.feedback_gains(), b, "beside an unready handle")
    finally:
        bare.close()


def test_one_nan_state_of_five_fails_alone_and_its_sequences_are_delivered():
    sols, states = _pool()
    five, st = sols[10:15], [s.copy() for s in states[10:15]]
    four = [five[0], five[1], five[3], five[4]]
    without = capi.nominal_and_gains_batch(four, [st[0], st[1], st[3], st[4]])
    assert _fused(four) == [1] * 4
    gains = [s.feedback_gains() for s in four]
    st[2][4] = np.float32(np.nan)
    alone = five[2].nominal_traj(st[2])
    rc, got = _raw(five, st)
    assert rc == capi.ERR_STATE
    assert "factorised" in five[2].L.mppi_last_error(five[2].h).decode()   # the bad handle's own message
    assert _fused(five) == [1] * 5
    with pytest.raises(capi.MppiError):
        five[2].feedback_gains()
    assert not np.any(got[2][0] == 9.0) and not np.any(got[2][1] == 9.0)   # its nominal buffers are filled
    np.testing.assert_array_equal(np.isfinite(got[2][0]), np.isfinite(alone[0]))
    _bits_equal(got[2][1], alone[1], "the NaN handle's control_seq")
    for s, g, q, w in zip(four, [got[0], got[1], got[3], got[4]], without, gains):
        _same_seqs(g, q, "beside the NaN instance")
        _same_gains(s.feedback_gains(), w, "beside the NaN instance")


@pytest.mark.parametrize("what", ["handle_twice", "null_state_seq", "null_control_seq"])
def test_malformed_sets_of_real_handles_are_refused_and_nothing_is_written(what):
    """The same handle at positions 0 and 2 of three, a NULL state_seqs[1], a NULL control_seqs[1] among valid handles:
    MPPI_ERR_INVALID, every buffer and every handle's earlier DDP result as it was, nothing run."""
    sols, states = _pool()
    three, st = sols[20:23], states[20:23]
    capi.nominal_and_gains_batch(three, st)
    before, fused = [s.feedback_gains() for s in three], _fused(three)
    assert fused == [1, 1, 1]
    if what == "handle_twice":
        rc, out = _raw([three[0], three[1], three[0]], [st[0], st[1], st[0]])
    elif what == "null_state_seq":
        rc, out = _raw(three, st, null_state_seq=(1,))
    else:
        rc, out = _raw(three, st, null_control_seq=(1,))
    assert rc == capi.ERR_INVALID
    assert all(np.all(a == 9.0) and np.all(b == 9.0) for a, b in out)
    assert _fused(three) == fused
    for s, b in zip(three, before):
        _same_gains(s.feedback_gains(), b, what)


# ------------------------------------------------------------------------------------------------------------------ 7, 8
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


def test_ticks_of_a_fleet16_fleet_closed_with_the_call():
    """Three ticks: the fleet solves in shared launches and closes with the new call; its twins solve the same way and close with the
    two calls.  Sequences and gains agree bit for bit on every tick, and a handle armed on its own stream stays armed across the call."""
    net, K, T, n = [6, 32, 32, 4], 64, 17, 3
    base = S.make_config(K, T, layers=net, track="oval")
    U0 = warm_U(base)
    fleet, states = _fleet16(n, base, U0, 500)
    twins, _ = _fleet16(n, base, U0, 500)
    extra = capi.Solver(base)
    extra.set_control_seq(U0)
    extra.seed(77, 0)
    everyone, all_states = fleet + [extra], states + [np.array(base["start_state"], np.float32)]
    try:
        capi.nominal_and_gains_batch(everyone, all_states)   # the first call on a device allocates the call's buffers: not beside a gated launch
        _two_calls(twins, states)
        for tick in range(3):
            extra.arm(0.05)
            assert extra.is_armed()
            capi.compute_control_batch(fleet, states)
            got = capi.nominal_and_gains_batch(everyone, all_states)
            assert _fused(everyone) == [1] * (n + 1)
            assert extra.is_armed()
            capi.compute_control_batch(twins, states)
            seqs, gains = _two_calls(twins, states)
            for i, (s, t) in enumerate(zip(fleet, twins)):
                what = "tick %d handle %d" % (tick, i)
                _bits_equal(s.get_results()["U"], t.get_results()["U"], what + ": the control sequence")
                _same_seqs(got[i], seqs[i], what)
                _same_gains(s.feedback_gains(), gains[i], what)
                s.slide_control_seq(1)
                t.slide_control_seq(1)
            extra.compute_control(all_states[-1])   # opens the armed solve
        print("NOMGAINS ticks: 3 ticks x %d handles, sequences and gains bit-equal to the twins' two calls; the armed handle stayed armed" % n)
    finally:
        _close(everyone + twins)


def test_pending_fleet16_solves_are_collected_and_the_new_controls_tracked():
    net, K, T, n = [6, 32, 32, 4], 64, 17, 3
    base = S.make_config(K, T, layers=net, track="oval")
    U0 = warm_U(base)
    fleet, states = _fleet16(n, base, U0, 900)
    try:
        capi.nominal_and_gains_batch(fleet, states)   # the first call on a device allocates the call's buffers
        capi.compute_control_batch(fleet, states, blocking=False)
        assert [s.debug_launch_info() for s in fleet] == [(n, 0)] * n
        first = capi.nominal_and_gains_batch(fleet, states)   # collects the three pending solves
        assert _fused(fleet) == [1] * n
        g_first = [s.feedback_gains() for s in fleet]
        for s in fleet:
            s.synchronize()   # nothing is pending any more
        again = capi.nominal_and_gains_batch(fleet, states)
        lo, hi = np.asarray(base["u_lo"], np.float32), np.asarray(base["u_hi"], np.float32)
        for i, (s, a, b, g) in enumerate(zip(fleet, first, again, g_first)):
            Unew = s.get_results()["U"]
            assert np.any(Unew != U0), "the solve moved the control sequence"
            _bits_equal(a[1], np.clip(Unew, lo, hi), "handle %d: control_seq is the NEW sequence, clamped" % i)
            _same_seqs(a, b, "handle %d against the call after an explicit synchronise" % i)
            _same_gains(s.feedback_gains(), g, "handle %d against the call after an explicit synchronise" % i)
        print("NOMGAINS pending: %d pending fleet16 solves collected by the call; replay and gains are the new sequence's" % n)
    finally:
        _close(fleet)


# ------------------------------------------------------------------------------------------------------------------ 9
@pytest.mark.timing
def test_the_call_beats_the_two_calls_at_64_handles():
    """6-32-32-4 and 6-64-64-64-64-4, T = 100, n = 64: the median of 200 calls of the new entry against the two entries in sequence
    (each side with the host's copy of the replay's outputs into the target buffers), alternating within one run
    (tools/fleet_time.py --finish).  Measured (MI355X): one call 0.963 / 2.101 ms, two calls 1.277 / 2.801 ms; DESIGN.md 4.26 has
    the table for n = 2 .. 64."""
    spec = importlib.util.spec_from_file_location("fleet_time", os.path.join(ROOT, "tools", "fleet_time.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    rows = [ft.finish_ms(net, 64, T=100, calls=200) for net in ([6, 32, 32, 4], [6, 64, 64, 64, 64, 4])]
    for row in rows:
        print("NOMGAINS timing n=64 T=100 net=%s: one call %.4f ms, two calls %.4f ms, ratio %.2f" % (
            row["net"], row["fused_ms"], row["two_ms"], row["two_ms"] / row["fused_ms"]))
    for row in rows:
        assert row["fused"] == 1, row
        assert row["fused_ms"] < row["two_ms"], row
