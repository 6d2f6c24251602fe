"""Closed-loop ticks of a fleet against a plant of its own (mppi_closed_loop_sim_batch).  The call is defined as a loop of public
calls -- batched solve, batched nominal replay (with the gains where feedback is on), mppi_plant_drive_batch, log, slide -- and "the
reference" below is a TWIN fleet driven by that loop from Python (_reference).  All comparisons are bit for bit (uint32 views).
Without feedback the eligible sets run the device path (every tick enqueued on the batch stream, the plant in
csrc/plant_drive_fleet.hip reading the device copy of U): those cases assert on_device == 1, so a silent fall-back cannot pass.  With
feedback the library runs its loop of public calls (on_device == 0): the cases hold it to the Python loop all the same.
  1. per form (fleet16, fleet_multi4, fleet_glb16), feedback off and on, (m, stride) in {(1, 2), (4, 1)}; (4, 2) for fleet16: 4 ticks --
     the logs, the final states and every handle's U, history, results and applied controls; one more batched solve agrees;
  2. 4 + 2 ticks equal 6;
  3. m = 1, no feedback, no plant model: bit for bit mppi_closed_loop_ticks_batch on a twin;
  4. a perturbed plant, stride 2: the feedback run and the feed-forward run differ, both finite; the distances to the nominal's row
     `stride` are printed;
  5. the fall-backs run the loop of public calls and give its bits; refusals write nothing;
  6. (timing) the device loop is faster than the library's loop of public calls at n = 64.
Each case prints what it measured."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import params as P
from tests import plant_drive_cases as PC
from tests.test_closed_loop_fleet_gpu import GLB, T, _base, _bits, _close, _fleet, _info, _snapshot, _states

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANTS = ("scaled", [6, 24, 4], [6, 64, 64, 64, 64, 4], [6, 200, 256, 4], [6, 65, 4])


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    assert hasattr(capi.lib(), "mppi_closed_loop_sim_batch"), "the library has no closed loop against a plant of its own"


def _give_plants(sols, plants=PLANTS):
    """Handle i's plant: the controller's own weights scaled by 1.05, or another layer list; both signs of negate_yaw_der.  The DDP
    weights of tests/plant_drive_cases.py: gains large enough to show."""
    for i, s in enumerate(sols):
        kind = plants[i % len(plants)]
        if kind == "scaled":
            s.set_plant_model(s.cfg["layers"], np.asarray(s.cfg["theta"], np.float32) * np.float32(1.05), s.cfg["negate_yaw_der"])
        elif kind is not None:
            l, th = P.synthetic_model(list(kind), seed=20 + i)
            s.set_plant_model(l, np.array(th, np.float32), bool(i % 2))
        s.set_ddp_weights(PC.DDP_Q, PC.DDP_R, PC.DDP_QF)


def _reference(sols, states, n_ticks, stride, m, feedback):
    """The loop the call is defined as, from Python -> (final states, [(state log, control log, cost log)])."""
    st = [np.array(s, np.float32) for s in states]
    logs = [(np.zeros((n_ticks + 1, 7), np.float32), np.zeros((n_ticks, stride * m, 2), np.float32), np.zeros(n_ticks, np.float32)) for _ in sols]
    for tick in range(n_ticks):
        capi.compute_control_batch(sols, st)
        seqs = capi.nominal_and_gains_batch(sols, st) if feedback else capi.nominal_traj_batch(sols, st)
        nxt, applied = capi.plant_drive_batch(sols, st, seqs, stride, m, feedback)
        for i, s in enumerate(sols):
            logs[i][0][tick] = st[i]
            logs[i][1][tick] = applied[i]
            logs[i][2][tick] = s.get_results(with_vectors=False)["traj_cost"]
            st[i] = nxt[i].copy()
            logs[i][0][tick + 1] = st[i]
            s.slide_control_seq(stride)
    return st, logs


def _run(sols, states, n_ticks, stride, m, feedback):
    logs = capi.closed_loop_sim_batch(sols, states, n_ticks, stride, m, feedback)
    return [l[0][-1].copy() for l in logs], logs


def _same(fleet, twins, got, ref, tag, snapshots=True):
    (fin, logs), (rfin, rlogs) = got, ref
    for i in range(len(fleet)):
        t = "%s handle %d" % (tag, i)
        for k, what in enumerate(("state_log", "control_log", "cost_log")):
            _bits(logs[i][k], rlogs[i][k], "%s: %s" % (t, what))
        _bits(fin[i], rfin[i], t + ": final state")
        if snapshots:
            a, b = _snapshot(fleet[i]), _snapshot(twins[i])
            for key in a:
                _bits(a[key], b[key], "%s: %s" % (t, key))


def _pair(n, variant="fleet16", bases=None, seed0=300, plants=PLANTS):
    fleet, twins = _fleet(n, variant, None, seed0, bases), _fleet(n, variant, None, seed0, bases)
    _give_plants(fleet, plants)
    _give_plants(twins, plants)
    return fleet, twins


# ------------------------------------------------------------------------------------------------------------------ 1
CASES = [(form, fb, m, stride) for form in ("fleet16", "fleet_multi4", "fleet_glb16") for fb in (False, True) for m, stride in ((1, 2), (4, 1))]
CASES += [("fleet16", False, 4, 2), ("fleet16", True, 4, 2)]


@pytest.mark.parametrize("form,feedback,m,stride", CASES)
def test_four_ticks_have_the_bits_of_the_loop_of_public_calls(form, feedback, m, stride):
    bases = [_base(net, k, t) for net, k, t in GLB] if form == "fleet_glb16" else None
    fleet, twins = _pair(3, form, bases, seed0=1300)
    try:
        states = _states(bases[0] if bases else _base(), 3)
        got = _run(fleet, states, 4, stride, m, feedback)
        assert _info(fleet) == [(0 if feedback else 1, 4)] * 3
        if not feedback:
            assert [s.debug_launch_info() for s in fleet] == [(3, 0)] * 3
        ref = _reference(twins, states, 4, stride, m, feedback)
        tag = "%s feedback=%d m=%d stride=%d" % (form, feedback, m, stride)
        _same(fleet, twins, got, ref, tag)
        assert got[1][0][1].shape == (4, stride * m, 2)
        # the next solve starts from the slid copy: one more batched solve agrees too
        capi.compute_control_batch(fleet, got[0])
        capi.compute_control_batch(twins, ref[0])
        for i, (a, b) in enumerate(zip(fleet, twins)):
            _bits(a.get_results()["U"], b.get_results()["U"], "%s handle %d: the solve behind the run" % (tag, i))
        moved = float(np.max(np.abs(got[1][0][0][-1] - got[1][0][0][0])))
        assert moved > 1e-2 and np.all(np.isfinite(got[0])), "the plant moves the car"
        print("CLOSEDLOOPSIM %s: 4 ticks x 3 handles, on_device %d, every log, state, U, history, result and applied control bit-equal to "
              "the loop of public calls, and the solve behind them; handle 0 moved %.3f" % (tag, _info(fleet)[0][0], moved))
    finally:
        _close(fleet, twins)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("feedback", [False, True])
def test_four_and_two_ticks_are_six(feedback):
    states = _states(_base(), 3)
    split, whole = _pair(3, seed0=1400)
    try:
        fin_a, logs_a = _run(split, states, 4, 1, 3, feedback)
        fin_b, logs_b = _run(split, fin_a, 2, 1, 3, feedback)
        assert _info(split) == [(0 if feedback else 1, 2)] * 3
        joined = [(np.concatenate([a[0], b[0][1:]]), np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]])) for a, b in zip(logs_a, logs_b)]
        got6 = _run(whole, states, 6, 1, 3, feedback)
        assert _info(whole) == [(0 if feedback else 1, 6)] * 3
        _same(split, whole, (fin_b, joined), got6, "4 + 2 ticks, feedback=%d" % feedback)
        print("CLOSEDLOOPSIM continuation feedback=%d: 4 + 2 ticks == 6 ticks bit for bit (m = 3)" % feedback)
    finally:
        _close(split, whole)


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("stride", [1, 2])
def test_one_substep_without_feedback_or_plant_model_is_the_closed_loop_of_the_own_model(stride):
    states = _states(_base(), 3)
    fleet, twins = _fleet(3, seed0=1500), _fleet(3, seed0=1500)
    try:
        got = _run(fleet, states, 5, stride, 1, False)
        assert _info(fleet) == [(1, 5)] * 3
        logs = capi.closed_loop_ticks_batch(twins, states, 5, stride)
        assert _info(twins) == [(1, 5)] * 3
        _same(fleet, twins, got, ([l[0][-1].copy() for l in logs], logs), "m = 1 against mppi_closed_loop_ticks_batch, stride %d" % stride)
        print("CLOSEDLOOPSIM equivalence stride %d: m = 1 without feedback or plant model is mppi_closed_loop_ticks_batch bit for bit" % stride)
    finally:
        _close(fleet, twins)


# ------------------------------------------------------------------------------------------------------------------ 4
def test_feedback_and_feed_forward_differ_against_a_perturbed_plant():
    """One tick of stride 2 with m = 4 against the controller's weights scaled by 1.05: the plant leaves the nominal trajectory, the
    feedback run corrects towards it.  How much nearer it ends is printed, not asserted: nobody has measured it."""
    states = _states(_base(), 3)
    fb, ff = _pair(3, seed0=1600, plants=("scaled",))
    nom = _fleet(3, seed0=1600)
    try:
        fin_fb, _ = _run(fb, states, 1, 2, 4, True)
        fin_ff, _ = _run(ff, states, 1, 2, 4, False)
        capi.compute_control_batch(nom, states)
        rows = [x[0][2] for x in capi.nominal_traj_batch(nom, states)]   # the nominal's row `stride` of the same solve
        for i in range(3):
            d_fb, d_ff = float(np.max(np.abs(fin_fb[i] - rows[i]))), float(np.max(np.abs(fin_ff[i] - rows[i])))
            print("CLOSEDLOOPSIM perturbed plant handle %d: distance of the final state from the nominal's row 2: feedback %.3e, feed-forward "
                  "%.3e" % (i, d_fb, d_ff))
            assert np.all(np.isfinite(fin_fb[i])) and np.all(np.isfinite(fin_ff[i]))
            assert np.any(fin_fb[i] != fin_ff[i]), "handle %d: the feedback changes the run" % i
    finally:
        _close(fb, ff, nom)


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("what", ["one_handle", "mixed_forms", "num_iters_2"])
def test_fallbacks_run_the_loop_with_its_bits(what):
    n, variant, bases = 3, "fleet16", None
    if what == "one_handle":
        n = 1
    elif what == "mixed_forms":
        variant = ["fleet16", "fleet_multi4", "fleet16"]
    else:
        bases = [_base(num_iters=2)] * 3
    fleet, twins = _pair(n, variant, bases, seed0=1700)
    try:
        states = _states(_base(), n)
        got = _run(fleet, states, 3, 1, 3, False)
        assert _info(fleet) == [(0, 3)] * n
        ref = _reference(twins, states, 3, 1, 3, False)
        _same(fleet, twins, got, ref, what)
        print("CLOSEDLOOPSIM fallback %s: on_device 0, 3 ticks bit-equal to the loop of public calls" % what)
    finally:
        _close(fleet, twins)


@pytest.mark.parametrize("what", ["handle_twice", "stride_T", "no_ticks", "substeps_17"])
def test_refusals_write_nothing_and_move_nothing(what):
    fleet = _fleet(3, seed0=1800)
    try:
        states = _states(_base(), 3)
        _run(fleet, states, 2, 1, 2, False)
        before_info, before_U = _info(fleet), [s.get_control_seq() for s in fleet]
        sols, n_ticks, stride, m = list(fleet), 2, 1, 2
        if what == "handle_twice":
            sols = [fleet[0], fleet[1], fleet[0]]
        elif what == "stride_T":
            stride = T
        elif what == "no_ticks":
            n_ticks = 0
        else:
            m = 17
        fp = C.POINTER(C.c_float)
        hs = (C.c_void_p * 3)(*[s.h for s in sols])
        st = np.ascontiguousarray(np.stack(states), np.float32)
        out = [(np.full((3, 7), 9.0, np.float32), np.full((2, 2, 2), 9.0, np.float32), np.full(2, 9.0, np.float32)) for _ in sols]
        ptrs = [(fp * 3)(*[o[k].ctypes.data_as(fp) for o in out]) for k in range(3)]
        rc = sols[0].L.mppi_closed_loop_sim_batch(hs, st.ctypes.data_as(fp), 3, n_ticks, stride, m, 0, *ptrs)
        assert rc == capi.ERR_INVALID, (what, rc)
        _bits(st, np.stack(states), what + ": states")
        assert all(np.all(a == 9.0) and np.all(b == 9.0) and np.all(c == 9.0) for a, b, c in out), what + ": the logs"
        assert _info(fleet) == before_info
        for s, u in zip(fleet, before_U):
            _bits(s.get_control_seq(), u, what + ": U")
    finally:
        _close(fleet)


# ------------------------------------------------------------------------------------------------------------------ 6
@pytest.mark.timing
def test_the_device_loop_beats_the_loop_of_public_calls():
    """n = 64, K = 1920, T = 100, 60 ticks, stride 1, m = 4, no feedback, 6-32-32-4 under fleet_multi4: the median of three runs of the
    device loop against the loop of public calls inside the library, alternating in one process (tools/fleet_time.py
    --closed-loop-sim).  Measured (MI355X): see DESIGN.md 4.29."""
    spec = importlib.util.spec_from_file_location("fleet_time", os.path.join(ROOT, "tools", "fleet_time.py"))
    ft = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ft)
    row = ft.closed_loop_sim_ms([6, 32, 32, 4], "fleet_multi4", 4, False, n=64, K=1920, T=100, ticks=60, stride=1)
    print("CLOSEDLOOPSIM timing n=64 K=1920 T=100 m=4 feedback=0: device loop %.4f ms per tick, loop of public calls %.4f ms, ratio %.2f" % (
        row["device_ms"], row["reference_ms"], row["reference_ms"] / row["device_ms"]))
    assert row["on_device"] == 1 and row["reference_on_device"] == 0, row
    assert row["device_ms"] < row["reference_ms"], row
