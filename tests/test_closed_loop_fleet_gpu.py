"""Closed-loop ticks of a fleet on the device (mppi_closed_loop_ticks_batch -> enqueue of every tick on the batch stream, the plant
step in csrc/plant_fleet.hip).  The call is defined as a loop of public calls -- batched solve, batched nominal replay, log, take
row `stride` of the replay as the next state, slide -- and "the reference" below is a TWIN fleet driven by that loop from Python
(_reference).  Every case that claims the device path asserts on_device == 1 (mppi_debug_closed_loop_info): a silent fall-back to
the loop cannot pass.  All comparisons are bit for bit (uint32 views) unless a case says otherwise.
  1. per form (fleet16, fleet_multi4, fleet_glb16 with three layer lists, K and T): 6 ticks, stride 1 -- the logs, the final states
     and every handle's U, history, results and applied controls;
  2. strides: 2 and 1 with optimization_stride 1, 3 with optimization_stride 3;
  3. continuation: 6 + 3 ticks are one call of 9, and one more batched solve agrees with the reference's;
  4. sizes: one tick, n = 2, n = 64, n = 65 (the loop: on_device == 0);
  5. fall-backs (on_device == 0, the reference's bits) and refusals (nothing written, nothing moved);
  6. neighbours: an armed handle outside the set stays armed; pending solves of the set are collected first;
  7. one NaN start state of three; 8. distance from the loop whose plant is the host replay; 9. (timing) device loop < reference loop.
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
from tests.helpers import warm_U

pytestmark = pytest.mark.gpu

U32 = np.uint32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE_BOUND = 1e-4   # the project's state bound (tests/test_nominal_fleet_gpu.py)
NET, K, T = [6, 32, 32, 4], 192, 17


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    assert hasattr(capi.lib(), "mppi_closed_loop_ticks_batch"), "the library has no closed-loop entry"


def _close(*fleets):
    for f in fleets:
        for s in f:
            s.close()


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, what
    np.testing.assert_array_equal(a.view(U32), b.view(U32), err_msg=what)


@functools.lru_cache(maxsize=None)
def _base(net=tuple(NET), k=K, t=T, opt_stride=1, num_iters=1):
    return S.make_config(k, t, layers=list(net), track="oval", opt_stride=opt_stride, num_iters=num_iters)


def _states(base, n):
    out = []
    for i in range(n):
        st = np.array(base["start_state"], np.float32)
        st[0] += np.float32(0.3 * i)
        st[4] += np.float32(0.05 * (i % 7))
        out.append(st)
    return out


def _fleet(n, variant="fleet16", base=None, seed0=300, bases=None):
    """n handles with generator noise (distinct seeds) and warm_U; bases: one configuration per handle instead of `base`; variant:
    one name, or one per handle."""
    bases = bases or [base or _base()] * n
    names = list(variant) if isinstance(variant, (list, tuple)) else [variant] * n   # None: the automatic form
    sols = []
    for i, (b, v) in enumerate(zip(bases, names)):
        sol = capi.Solver(b)
        if v:
            sol.set_rollout_variant(v)
        sol.set_control_seq(warm_U(b, seed=7 + i))
        sol.seed(seed0 + i, 0)
        sols.append(sol)
    return sols


def _reference(sols, states, n_ticks, stride, host_plant=False):
    """The loop the call is defined as, from Python -> (final states, [(state log, control log, cost log)]).  host_plant: the replay of
    every handle is the single host call (what the library's loop does for one handle and for a set with a basis-function handle)."""
    st = [np.array(s, np.float32) for s in states]
    logs = [(np.zeros((n_ticks + 1, 7), np.float32), np.zeros((n_ticks, stride, 2), np.float32), np.zeros(n_ticks, np.float32)) for _ in sols]
    for tick in range(n_ticks):
        capi.compute_control_batch(sols, st)
        if host_plant:
            seqs = [s.nominal_traj(x) for s, x in zip(sols, st)]
        else:
            seqs = capi.nominal_traj_batch(sols, st)
            assert [s.debug_nominal_info() for s in sols] == [1] * len(sols), "the reference's replay runs on the device"
        for i, s in enumerate(sols):
            logs[i][0][tick] = st[i]
            logs[i][1][tick] = seqs[i][1][:stride]
            logs[i][2][tick] = s.get_results(with_vectors=False)["traj_cost"]
            st[i] = seqs[i][0][stride].copy()
            logs[i][0][tick + 1] = st[i]
            s.slide_control_seq(stride)
    return st, logs


def _run(sols, states, n_ticks, stride):
    """The entry -> (final states, logs)."""
    logs = capi.closed_loop_ticks_batch(sols, states, n_ticks, stride)
    return [l[0][-1].copy() for l in logs], logs


def _snapshot(s):
    r = s.get_results()
    return dict(U=s.get_control_seq(), hist=s.get_control_hist(), res_U=r["U"], costs=r["costs"], w=r["w"],
                traj_cost=np.float32(r["traj_cost"]), V=s.get_applied_controls())


def _same(fleet, twins, got, ref, tag, snapshots=True):
    """Final states, logs and (snapshots) every handle against its twin, bit for bit."""
    (fin, logs), (rfin, rlogs) = got, ref
    for i in range(len(fleet)):
        t = "%s handle %d" % (tag, i)
        _bits(logs[i][0], rlogs[i][0], t + ": state_log")
        _bits(logs[i][1], rlogs[i][1], t + ": control_log")
        _bits(logs[i][2], rlogs[i][2], t + ": cost_log")
        _bits(fin[i], rfin[i], t + ": final state")
        if snapshots:
            a, b = _snapshot(fleet[i]), _snapshot(twins[i])
            for key in a:
                _bits(a[key], b[key], "%s: %s" % (t, key))


def _info(sols):
    return [s.debug_closed_loop_info() for s in sols]


def _loop_pair(n, n_ticks, stride, variant="fleet16", base=None, bases=None, seed0=300, tag=""):
    """A fleet through the entry and its twins through the reference loop; -> (fleet, twins, got, ref)."""
    fleet, twins = _fleet(n, variant, base, seed0, bases), _fleet(n, variant, base, seed0, bases)
    states = _states(bases[0] if bases else (base or _base()), n)
    got = _run(fleet, states, n_ticks, stride)
    ref = _reference(twins, states, n_ticks, stride)
    return fleet, twins, got, ref


# ------------------------------------------------------------------------------------------------------------------ 1
GLB = [((6, 32, 32, 4), 192, 17), ((6, 160, 4), 128, 13), ((6, 48, 24, 48, 4), 64, 21)]


@pytest.mark.parametrize("form", ["fleet16", "fleet_multi4", "fleet_glb16"])
def test_six_ticks_have_the_bits_of_the_reference_loop(form):
    bases = [_base(net, k, t) for net, k, t in GLB] if form == "fleet_glb16" else None
    fleet, twins, got, ref = _loop_pair(3, 6, 1, form, bases=bases)
    try:
        assert _info(fleet) == [(1, 6)] * 3
        assert [s.debug_launch_info() for s in fleet] == [(3, 0)] * 3
        _same(fleet, twins, got, ref, form)
        moved = float(np.max(np.abs(got[1][0][0][-1] - got[1][0][0][0])))
        assert moved > 1e-2, "the plant moves the car"
        print("CLOSEDLOOP %s: 6 ticks x 3 handles on the device, every log, state, U, history, result and applied control bit-equal to the "
              "reference loop; handle 0 moved %.3f" % (form, moved))
    finally:
        _close(fleet, twins)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("stride,opt_stride", [(2, 1), (1, 1), (3, 3)])
def test_strides(stride, opt_stride):
    base = _base(opt_stride=opt_stride)
    fleet, twins, got, ref = _loop_pair(3, 4, stride, base=base, seed0=410)
    try:
        assert _info(fleet) == [(1, 4)] * 3
        _same(fleet, twins, got, ref, "stride %d (optimization_stride %d)" % (stride, opt_stride))
        # the next solve uploads nothing and starts from the slid device copy: one more tick agrees too
        capi.compute_control_batch(fleet, got[0])
        capi.compute_control_batch(twins, ref[0])
        for i, (a, b) in enumerate(zip(fleet, twins)):
            _bits(a.get_results()["U"], b.get_results()["U"], "stride %d handle %d: the solve behind the run" % (stride, i))
        print("CLOSEDLOOP stride %d, optimization_stride %d: 4 ticks bit-equal to the reference loop, and the solve behind them" % (stride, opt_stride))
    finally:
        _close(fleet, twins)


# ------------------------------------------------------------------------------------------------------------------ 3
def test_two_calls_continue_where_one_call_would_be():
    states = _states(_base(), 3)
    split, whole, twins = _fleet(3, seed0=520), _fleet(3, seed0=520), _fleet(3, seed0=520)
    try:
        fin_a, logs_a = _run(split, states, 6, 1)
        fin_b, logs_b = _run(split, fin_a, 3, 1)
        assert _info(split) == [(1, 3)] * 3
        joined = [(np.concatenate([a[0], b[0][1:]]), np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]])) for a, b in zip(logs_a, logs_b)]
        got9 = _run(whole, states, 9, 1)
        assert _info(whole) == [(1, 9)] * 3
        ref = _reference(twins, states, 9, 1)
        _same(split, twins, (fin_b, joined), ref, "6 + 3 ticks")
        _same(whole, twins, got9, ref, "9 ticks")
        # generator stream, device U, in_cur and seq: one more batched solve on the fleet and on the reference
        capi.compute_control_batch(split, fin_b)
        capi.compute_control_batch(twins, ref[0])
        for i, (a, b) in enumerate(zip(split, twins)):
            ra, rb = a.get_results(), b.get_results()
            for key in ("U", "costs", "w"):
                _bits(ra[key], rb[key], "handle %d: %s of the solve behind the run" % (i, key))
            _bits(a.get_applied_controls(), b.get_applied_controls(), "handle %d: applied controls of the solve behind the run" % i)
        print("CLOSEDLOOP continuation: 6 + 3 ticks == 9 ticks == the reference loop, and the next batched solve agrees bit for bit")
    finally:
        _close(split, whole, twins)


@pytest.mark.parametrize("n_ticks", [1, 4])
def test_traces_behind_the_call_replay_from_the_last_ticks_state(n_ticks):
    """mppi_trace_rollouts / mppi_trace_rollouts_batch replay from the state of the handle's last solve: behind the call that is the
    state tick n_ticks - 1 started from -- for one tick the start state, which only the host holds.  The fleet's traces, handle by
    handle and in one batched call, against the twins' behind the reference loop; the traced states' first row is that state."""
    fleet, twins, got, ref = _loop_pair(3, n_ticks, 1, seed0=560)
    try:
        assert _info(fleet) == [(1, n_ticks)] * 3
        _same(fleet, twins, got, ref, "%d ticks" % n_ticks, snapshots=False)
        ks = [0, 5, K - 1]
        for i, (a, b) in enumerate(zip(fleet, twins)):
            ta, tb = a.trace_rollouts(ks), b.trace_rollouts(ks)
            for key in ("states", "controls", "step_costs", "costs"):
                _bits(ta[key], tb[key], "%d ticks handle %d: traced %s" % (n_ticks, i, key))
            np.testing.assert_array_equal(ta["first_crash"], tb["first_crash"])
            for r in range(len(ks)):
                _bits(ta["states"][r][0], got[1][i][0][n_ticks - 1], "%d ticks handle %d: the trace starts from the last tick's state" % (n_ticks, i))
        fa, fb = capi.trace_rollouts_batch(fleet, [4] * 3), capi.trace_rollouts_batch(twins, [4] * 3)
        for i, (ta, tb) in enumerate(zip(fa, fb)):
            for key in ("states", "controls", "step_costs", "costs"):
                _bits(ta[key], tb[key], "%d ticks handle %d: batched trace %s" % (n_ticks, i, key))
        print("CLOSEDLOOP traces: behind %d tick(s) the fleet's traces (single and batched) are the twins' bit for bit and start from "
              "the last tick's state" % n_ticks)
    finally:
        _close(fleet, twins)


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("what,n,n_ticks", [("one_tick", 3, 1), ("n2", 2, 3), ("n64", 64, 3), ("n65", 65, 2)])
def test_sizes(what, n, n_ticks):
    base = _base(k=64, t=9) if n >= 64 else _base()
    fleet, twins, got, ref = _loop_pair(n, n_ticks, 1, base=base, seed0=600)
    try:
        assert _info(fleet) == [(1 if n <= 64 else 0, n_ticks)] * n
        _same(fleet, twins, got, ref, what, snapshots=n < 64)
        for i in range(0, n, 9 if n >= 64 else 1):
            _bits(fleet[i].get_control_seq(), twins[i].get_control_seq(), "%s handle %d: U" % (what, i))
            _bits(fleet[i].get_control_hist(), twins[i].get_control_hist(), "%s handle %d: history" % (what, i))
        print("CLOSEDLOOP sizes %s: n = %d, %d ticks, on_device %d, bit-equal to the reference loop" % (what, n, n_ticks, _info(fleet)[0][0]))
    finally:
        _close(fleet, twins)


# ------------------------------------------------------------------------------------------------------------------ 5
def _bf_base(golden_dir):
    W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    return S.make_config(K, T, track="oval", bf_W=W, opt_stride=1)


@pytest.mark.parametrize("what", ["one_handle", "basis_function", "mixed_forms", "num_iters_2", "explicit_noise"])
def test_fallbacks_run_the_loop_with_its_bits(what, golden_dir):
    n, variant, bases, host_plant = 3, "fleet16", None, False
    if what == "one_handle":
        n, host_plant = 1, True
    elif what == "basis_function":
        bases, variant, host_plant = [_base(), _bf_base(golden_dir), _base()], ["fleet16", None, "fleet16"], True
    elif what == "mixed_forms":
        variant = ["fleet16", "fleet_multi4", "fleet16"]
    elif what == "num_iters_2":
        bases = [_base(num_iters=2)] * 3
    fleet, twins = _fleet(n, variant, None, 700, bases), _fleet(n, variant, None, 700, bases)
    try:
        if what == "explicit_noise":
            eps = np.random.RandomState(5).standard_normal((K, T, 2)).astype(np.float32)
            fleet[1].set_noise(eps)
            twins[1].set_noise(eps)
        states = _states(_base(), n)
        got = _run(fleet, states, 3, 1)
        assert _info(fleet) == [(0, 3)] * n
        ref = _reference(twins, states, 3, 1, host_plant=host_plant)
        _same(fleet, twins, got, ref, what)
        print("CLOSEDLOOP fallback %s: on_device 0, 3 ticks bit-equal to the loop of public calls" % what)
    finally:
        _close(fleet, twins)


def _raw(sols, states, n_ticks, stride, fill=9.0):
    """The C call on buffers filled with `fill` -> (status, states, [(state log, control log, cost log)])."""
    n = len(sols)
    fp = C.POINTER(C.c_float)
    hs = (C.c_void_p * n)(*[s.h for s in sols])
    st = np.ascontiguousarray(np.stack([np.asarray(x, np.float32).reshape(7) for x in states]), np.float32)
    nt, sd = max(n_ticks, 1), max(stride, 1)
    out = [(np.full((nt + 1, 7), fill, np.float32), np.full((nt, sd, 2), fill, np.float32), np.full(nt, fill, np.float32)) for _ in sols]
    ptrs = [(fp * n)(*[o[k].ctypes.data_as(fp) for o in out]) for k in range(3)]
    rc = sols[0].L.mppi_closed_loop_ticks_batch(hs, st.ctypes.data_as(fp), n, int(n_ticks), int(stride), *ptrs)
    return rc, st, out


@pytest.mark.parametrize("what", ["handle_twice", "stride_T", "no_ticks", "unready"])
def test_refusals_write_nothing_and_move_nothing(what):
    from tests.test_fleet16_gpu import _bare_solver
    fleet = _fleet(3, seed0=800)
    bare = _bare_solver(_base()) if what == "unready" else None
    try:
        states = _states(_base(), 3)
        _run(fleet, states, 2, 1)
        before_info, before_U = _info(fleet), [s.get_control_seq() for s in fleet]
        sols, n_ticks, stride, want = list(fleet), 2, 1, capi.ERR_INVALID
        if what == "handle_twice":
            sols = [fleet[0], fleet[1], fleet[0]]
        elif what == "stride_T":
            stride = T
        elif what == "no_ticks":
            n_ticks = 0
        else:
            sols, want = [fleet[0], fleet[1], bare], capi.ERR_STATE   # the unready handle LAST: the two before it must not have moved
        rc, st, out = _raw(sols, states, n_ticks, stride)
        assert rc == want, (what, rc)
        if bare is not None:
            assert "mppi_set_nn_params" in bare.L.mppi_last_error(bare.h).decode()
        _bits(st, np.stack(states), what + ": states")
        assert all(np.all(a == 9.0) and np.all(b == 9.0) and np.all(c == 9.0) for a, b, c in out), what + ": the logs"
        assert _info(fleet) == before_info
        for s, u in zip(fleet, before_U):
            _bits(s.get_control_seq(), u, what + ": U")
        print("CLOSEDLOOP refusal %s: status %d, nothing written, nothing moved" % (what, rc))
    finally:
        _close(fleet, [bare] if bare is not None else [])


# ------------------------------------------------------------------------------------------------------------------ 6
def test_an_armed_handle_outside_the_set_stays_armed_and_pending_solves_are_collected():
    states = _states(_base(), 3)
    fleet, twins = _fleet(3, seed0=900), _fleet(3, seed0=900)
    outsider, its_twin = _fleet(1, None, seed0=950)[0], _fleet(1, None, seed0=950)[0]
    try:
        x0 = np.array(_base()["start_state"], np.float32)
        for s in (outsider, its_twin):
            s.compute_control(x0)
            s.slide_control_seq(1)
        _run(fleet, states, 1, 1)   # the first call on a device allocates the run's buffers: not beside a gated launch
        _reference(twins, states, 1, 1)
        outsider.arm(0.05)
        assert outsider.is_armed()
        capi.compute_control_batch(fleet, states, blocking=False)   # pending solves of the set: the call collects them first
        got = _run(fleet, states, 3, 1)
        assert outsider.is_armed(), "the call leaves a handle outside the set armed"
        outsider.compute_control(x0)   # opens the armed solve
        its_twin.compute_control(x0)
        _bits(outsider.get_results()["U"], its_twin.get_results()["U"], "the armed solve of the handle outside the set")
        capi.compute_control_batch(twins, states)
        ref = _reference(twins, states, 3, 1)
        assert _info(fleet) == [(1, 3)] * 3
        _same(fleet, twins, got, ref, "behind pending solves")
        print("CLOSEDLOOP neighbours: pending solves of the set collected, the armed outsider stayed armed and opened with its twin's bits")
    finally:
        _close(fleet, twins, [outsider, its_twin])


# ------------------------------------------------------------------------------------------------------------------ 7
def test_one_nan_start_state_of_three_stays_alone():
    states = _states(_base(), 3)
    bad = [s.copy() for s in states]
    bad[1][4] = np.float32(np.nan)
    fleet, twins, clean = _fleet(3, seed0=1000), _fleet(3, seed0=1000), _fleet(3, seed0=1000)
    try:
        got = _run(fleet, bad, 3, 1)
        assert _info(fleet) == [(1, 3)] * 3
        ref = _reference(twins, bad, 3, 1)
        without = _run(clean, states, 3, 1)
        _same(fleet, twins, got, ref, "one NaN state", snapshots=False)
        assert not np.all(np.isfinite(got[1][1][0])), "the NaN spreads through that handle's states"
        assert np.all(np.isfinite(got[1][1][1])), "its controls stay finite (clamped means of clamped controls)"
        for i in (0, 2):
            for k in range(3):
                _bits(got[1][i][k], without[1][i][k], "beside the NaN handle: handle %d log %d" % (i, k))
            _bits(fleet[i].get_control_seq(), clean[i].get_control_seq(), "beside the NaN handle: handle %d U" % i)
        print("CLOSEDLOOP NaN: handle 1's logs carry the reference's bits, NaN patterns included; handles 0 and 2 are untouched")
    finally:
        _close(fleet, twins, clean)


# ------------------------------------------------------------------------------------------------------------------ 8
def test_distance_from_the_loop_with_the_host_plant():
    """Against a loop whose plant is the host's mppi_nominal_traj (glibc's sinf / cosf): the states after the FIRST tick are one
    Euler step apart by at most an ulp of sin / cos, inside the project's state bound.  Later ticks are printed, not asserted: a 1-ulp
    difference passes through the solve, and no bound for that has been measured."""
    states = _states(_base(), 3)
    fleet, hosts = _fleet(3, seed0=1100), _fleet(3, seed0=1100)
    try:
        got = _run(fleet, states, 6, 1)
        ref = _reference(hosts, states, 6, 1, host_plant=True)
        per_tick = [max(float(np.max(np.abs(got[1][i][0][t] - ref[1][i][0][t]))) for i in range(3)) for t in range(1, 7)]
        print("CLOSEDLOOP host plant: largest state distance after tick 1..6: %s (bound after tick 1: %.0e)" % (
            " ".join("%.2e" % d for d in per_tick), STATE_BOUND))
        assert per_tick[0] <= STATE_BOUND
    finally:
        _close(fleet, hosts)


# ------------------------------------------------------------------------------------------------------------------ 9
@pytest.mark.timing
def test_the_device_loop_beats_the_reference_loop():
    """n = 64, K = 1920, T = 100, 200 ticks, stride 1: 6-32-32-4 under fleet_multi4 and 6-64x4-4 under fleet16; the median of three runs
    of the device loop against the reference loop inside the library, alternating in one process (tools/fleet_time.py --closed-loop).
    Measured (MI355X): see DESIGN.md 4.28."""
    spec = importlib.util.spec_from_file_location("fleet_time", os.path.join(ROOT, "tools", "fleet_time.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    rows = [ft.closed_loop_ms(net, variant, n=64, K=1920, T=100, ticks=200, stride=1)
            for net, variant in (([6, 32, 32, 4], "fleet_multi4"), ([6, 64, 64, 64, 64, 4], "fleet16"))]
    for row in rows:
        print("CLOSEDLOOP timing n=64 K=1920 T=100 net=%s %s: device loop %.4f ms per tick, reference loop %.4f ms, from Python %.4f ms, "
              "ratio %.2f" % (row["net"], row["variant"], row["device_ms"], row["reference_ms"], row["python_ms"],
                              row["reference_ms"] / row["device_ms"]))
    for row in rows:
        assert row["on_device"] == 1 and row["reference_on_device"] == 0, row
        assert row["device_ms"] < row["reference_ms"], row
