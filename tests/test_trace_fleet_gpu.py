"""mppi_trace_rollouts_batch on the device: the traces of a fleet in one launch (csrc/rollout_trace.hip: rollout_trace_fleet_kernel,
rollout_trace_fleet_bf_kernel) with the largest weights chosen on the device (trace_select_fleet_kernel).

The new kernels are never compared with themselves: every record is held to the handle's own mppi_trace_rollouts /
mppi_top_rollouts BIT FOR BIT, costs to mppi_get_results, states and first_crash to the float64 reference of
tests/trace_cases.py (TOL_STATE and the decided sets are its: measured and capped on the CPU, tests/test_trace_cpu.py)."""
import ctypes as C
import time

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import synthetic as S
from tests import trace_cases as TC

pytestmark = pytest.mark.gpu

U32 = np.uint32
K = TC.K
WAIT = 0.1
FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int)
KEYS = ("states", "controls", "step_costs", "costs", "first_crash")

# (scene, net, T, stride, variant): 6-32-32-4, 6-64-64-4, 6-33-97-66-4, 6-197-67-4 (trace image in GLOBAL memory), basis functions;
# T = 37, 5, 2, 37, 5.  FLEET_A: the scenes differ; FLEET_B: patchwork / tilt-slide, where the branch terms fire
FLEET_A = [("oval", "32x2", 37, 1, "row_exact"), ("tilt_l1", "64x2", 5, 1, "oct"), ("oval", "33-97-66", 2, 0, "lds128"),
           ("patchwork", "197-67", 37, 0, "valu_lds"), ("tilt_l1", "bf", 5, 3, "bf3")]
FLEET_B = [("tilt_l1", "32x2", 37, 1, "row_exact"), ("patchwork", "64x2", 5, 3, "oct"), ("patchwork", "33-97-66", 2, 0, "lds128"),
           ("tilt_l2", "197-67", 37, 1, "valu_lds"), ("patchwork", "bf", 5, 1, "bf3")]


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


def _bits(x):
    return np.ascontiguousarray(x).view(U32)


def _solved(case, **over):
    scene, net, T, stride, variant = case
    cfg, U0, eps = TC.problem(scene, net, T, stride)
    if over:
        cfg = dict(cfg, **over)
    sol = capi.Solver(cfg)
    sol.set_rollout_variant(variant)
    sol.set_control_seq(U0)
    sol.set_noise(eps)
    sol.compute_control(cfg["start_state"])
    return sol


_fleets = {}


def _fleet(name):
    """the five solved handles of FLEET_A / FLEET_B, made once; tests that change a handle make their own"""
    if name not in _fleets:
        _fleets[name] = [_solved(c) for c in (FLEET_A if name == "A" else FLEET_B)]
    return _fleets[name]


@pytest.fixture(scope="module", autouse=True)
def _close_fleets():
    yield
    for sols in _fleets.values():
        for s in sols:
            s.close()
    _fleets.clear()


def _same(got, sol, ks, what, keys=KEYS):
    """one handle's records of the batch call against its own mppi_trace_rollouts of the same indices, bit for bit"""
    want = sol.trace_rollouts(ks, with_costs="costs" in keys)
    np.testing.assert_array_equal(got["ks"], np.asarray(ks, np.int32), err_msg="%s ks" % what)
    for k in keys:
        np.testing.assert_array_equal(_bits(got[k]), _bits(want[k]), err_msg="%s %s" % (what, k))
    return want


def _sentinels(sols, counts, with_costs=True):
    outs = []
    for s, c in zip(sols, counts):
        o = dict(ks=np.full(c, -9, np.int32), states=np.full((c, s.T, 7), 9.0, np.float32), controls=np.full((c, s.T, 2), 9.0, np.float32),
                 first_crash=np.full(c, -9, np.int32))
        if with_costs:
            o.update(step_costs=np.full((c, s.T), 9.0, np.float32), costs=np.full(c, 9.0, np.float32))
        outs.append(o)
    return outs


def _untouched(outs):
    return all(np.all(a == (-9 if a.dtype == np.int32 else 9.0)) for o in outs for a in o.values())


def test_mixed_five_fleet_equals_the_single_calls():
    sols = _fleet("A")
    rng = np.random.RandomState(5)
    ks = [np.array([0, 127, 64, 64, 3], np.int32), np.array([127, 0, 127], np.int32), np.zeros(0, np.int32), np.array([9, 0, 9, 127], np.int32),
          np.concatenate([[0, 127, 127], rng.permutation(K)[:61]]).astype(np.int32)]
    counts = [k.size for k in ks]
    assert counts == [5, 3, 0, 4, 64]
    got = capi.trace_rollouts_batch(sols, counts, ks)
    for i, s in enumerate(sols):
        assert s.debug_trace_info() == 1, i
    for i, s in enumerate(sols):
        _same(got[i], s, ks[i], "member %d" % i)
        # all five forms keep the reference's order: the costs are the solve's own
        np.testing.assert_array_equal(_bits(got[i]["costs"]), _bits(s.get_results()["costs"][ks[i]]), err_msg="member %d" % i)
        assert s.debug_trace_info() == (0 if counts[i] else 1)   # a single call that traced something in between says so


def test_second_scene_set_against_float64():
    sols = _fleet("B")
    ks = [np.arange(K, dtype=np.int32)] * 5
    got = capi.trace_rollouts_batch(sols, [K] * 5, ks)
    assert [s.debug_trace_info() for s in sols] == [1] * 5
    for i, (s, case) in enumerate(zip(sols, FLEET_B)):
        key = case[:4]
        ref = TC.trace64(*key)
        dev = np.abs(got[i]["states"].astype(np.float64) - TC.states64(*key))
        dec = ref["decided"]
        wrong = dec & (got[i]["first_crash"] != ref["first"])
        print("TRACEFLEET %s-%s-T%d-s%d: states max dev %.2e (TOL_STATE %.1e); %d decided, %d of them flagged, first_crash wrong on %d" % (
            key + (dev.max(), TC.TOL_STATE, int(dec.sum()), int(np.sum(dec & (ref["first"] >= 0))), int(wrong.sum()))))
        assert dev.max() <= TC.TOL_STATE, i
        assert not wrong.any(), (i, np.nonzero(wrong)[0][:8])
        np.testing.assert_array_equal(_bits(got[i]["costs"]), _bits(s.get_results()["costs"]), err_msg="member %d" % i)
        np.testing.assert_array_equal(_bits(TC.fold_step_costs(got[i]["step_costs"])), _bits(got[i]["costs"]), err_msg="member %d" % i)


def _hold_top(sols, counts, what):
    got = capi.trace_rollouts_batch(sols, counts, None)
    assert [s.debug_trace_info() for s in sols] == [1] * len(sols)
    for i, (s, c) in enumerate(zip(sols, counts)):
        top = s.top_rollouts(c)
        np.testing.assert_array_equal(got[i]["ks"], top, err_msg="%s member %d" % (what, i))
        _same(got[i], s, top, "%s member %d" % (what, i))


def test_top_selection_equals_mppi_top_rollouts():
    _hold_top(_fleet("A"), [1, 7, K, 16, 16], "top")


def test_top_selection_on_hundreds_of_equal_weights():
    """gamma = 50 (tests/test_every_rollout_gpu.py's extreme): most weights are exactly 0, so the order among them is the tie
    rule alone -- the lower index first -- and every member is asked for all K."""
    sols = [_solved(c, gamma=50.0) for c in FLEET_A]
    try:
        zeros = [int(np.sum(s.get_results()["w"] == 0.0)) for s in sols]
        print("TRACEFLEET gamma=50: weights that are exactly 0 per member: %s of %d" % (zeros, K))
        assert sum(zeros) >= 200, zeros   # "hundreds": else the problem no longer tests the tie rule
        _hold_top(sols, [K] * 5, "gamma 50")
    finally:
        for s in sols:
            s.close()


def test_top_selection_beyond_one_tile_and_the_streaming_tail():
    """K = 4160: five staging tiles of the selection (the last one ragged), weights written by the streaming tail."""
    cfg = S.make_config(4160, 5, track="oval")
    big = capi.Solver(cfg)
    try:
        big.seed(11, 0)
        big.compute_control(cfg["start_state"])
        sols = [big, _fleet("A")[4]]
        _hold_top(sols, [100, 3], "K 4160")
        _hold_top(sols, [1024, 0], "K 4160, a whole chunk")
    finally:
        big.close()


def test_chosen_and_explicit_members_in_one_call():
    sols = _fleet("A")
    ks = [None, np.array([5, 5, 0], np.int32), None, np.array([127], np.int32), None]
    counts = [4, 3, 2, 1, 64]
    got = capi.trace_rollouts_batch(sols, counts, ks)
    assert [s.debug_trace_info() for s in sols] == [1] * 5
    for i, s in enumerate(sols):
        _same(got[i], s, s.top_rollouts(counts[i]) if ks[i] is None else ks[i], "member %d" % i)


def test_two_handles_and_an_all_zero_call():
    sols = [_fleet("A")[0], _fleet("A")[4]]
    ks = [np.array([3, 127], np.int32), np.array([0, 1, 2], np.int32)]
    got = capi.trace_rollouts_batch(sols, [2, 3], ks)
    assert [s.debug_trace_info() for s in sols] == [1, 1]
    for i, s in enumerate(sols):
        _same(got[i], s, ks[i], "member %d" % i)
    assert [s.debug_trace_info() for s in sols] == [0, 0]
    outs = _sentinels(sols, [4, 4])
    capi.trace_rollouts_batch(sols, [0, 0], None, outputs=outs)   # MPPI_OK
    assert _untouched(outs)
    assert [s.debug_trace_info() for s in sols] == [1, 1]


def test_sixty_four_and_sixty_five_handles():
    """K = 64, T = 5, two rollouts each: 64 handles are one launch, 65 are two; even members bring indices, odd ones choose."""
    sols = []
    try:
        for i in range(65):
            cfg = S.make_config(64, 5, track="oval", instance=i % 7)
            s = capi.Solver(cfg)
            s.seed(100 + i, 0)
            s.compute_control(cfg["start_state"])
            sols.append(s)
        ks = [np.array([i % 64, 63], np.int32) if i % 2 == 0 else None for i in range(65)]
        want = [s.trace_rollouts(s.top_rollouts(2) if k is None else k) for s, k in zip(sols, ks)]
        for n in (64, 65):
            got = capi.trace_rollouts_batch(sols[:n], [2] * n, ks[:n])
            assert [s.debug_trace_info() for s in sols[:n]] == [1] * n
            for i in range(n):
                for key in KEYS:
                    np.testing.assert_array_equal(_bits(got[i][key]), _bits(want[i][key]), err_msg="n %d member %d %s" % (n, i, key))
    finally:
        for s in sols:
            s.close()


def test_a_ragged_count_beside_a_whole_chunk():
    """K = 1024, T = 2: one member traces a whole chunk (its 1024 largest weights: all of them, in order), its neighbour seven
    rollouts -- no multiple of the four wavefronts of a workgroup."""
    sols = []
    try:
        for i in range(2):
            cfg = S.make_config(1024, 2, track="oval", instance=i)
            s = capi.Solver(cfg)
            s.seed(31 + i, 0)
            s.compute_control(cfg["start_state"])
            sols.append(s)
        ks = [None, np.array([1023, 0, 5, 5, 77, 512, 1], np.int32)]
        got = capi.trace_rollouts_batch(sols, [1024, 7], ks)
        assert [s.debug_trace_info() for s in sols] == [1, 1]
        _same(got[0], sols[0], sols[0].top_rollouts(1024), "chunk")
        _same(got[1], sols[1], ks[1], "ragged")
        got = capi.trace_rollouts_batch(sols[::-1], [7, 1024], ks[::-1])   # the ragged member first: it sets no grid
        _same(got[1], sols[0], sols[0].top_rollouts(1024), "chunk, second")
        _same(got[0], sols[1], ks[1], "ragged, first")
    finally:
        for s in sols:
            s.close()


def test_fallbacks_differ_in_one_thing_each():
    a, b = _fleet("A")[0], _fleet("A")[4]
    # n = 1
    got = capi.trace_rollouts_batch([a], [6], None)
    assert a.debug_trace_info() == 0
    _same(got[0], a, a.top_rollouts(6), "n = 1")
    # a count above the chunk (duplicates: 1025 indices of K = 128)
    many = (np.arange(1025) % K).astype(np.int32)
    got = capi.trace_rollouts_batch([a, b], [1025, 3], [many, None])
    assert [a.debug_trace_info(), b.debug_trace_info()] == [0, 0]
    _same(got[0], a, many, "above the chunk")
    _same(got[1], b, b.top_rollouts(3), "beside it")
    # ... and above K alone (129 indices of K = 128), though within the chunk
    got = capi.trace_rollouts_batch([a, b], [K + 1, 3], [many[:K + 1], None])
    assert [a.debug_trace_info(), b.debug_trace_info()] == [0, 0]
    _same(got[0], a, many[:K + 1], "above K")
    # the same two with K indices share the launch
    capi.trace_rollouts_batch([a, b], [K, 3], [many[:K], None])
    assert [a.debug_trace_info(), b.debug_trace_info()] == [1, 1]


def test_an_armed_handle_falls_back_and_stays_armed():
    own = _solved(FLEET_A[0])
    other = _fleet("A")[4]
    try:
        ks = np.array([0, 9, 127], np.int32)
        want = own.trace_rollouts(ks)
        top = other.top_rollouts(5)
        own.arm(WAIT)
        assert own.is_armed()
        t0 = time.perf_counter()
        got = capi.trace_rollouts_batch([own, other], [3, 5], [ks, None])
        dt = time.perf_counter() - t0
        assert own.is_armed(), "the trace disarmed the handle"
        assert [own.debug_trace_info(), other.debug_trace_info()] == [0, 0]
        own.disarm()
        print("TRACEFLEET armed fallback: %.4f s" % dt)
        for k in KEYS:
            np.testing.assert_array_equal(_bits(got[0][k]), _bits(want[k]), err_msg=k)
        _same(got[1], other, top, "beside the armed handle")
    finally:
        own.close()


def test_errors_leave_the_buffers_alone():
    solved = _fleet("A")[0]
    cfg, U0, eps = TC.problem(*FLEET_A[1][:4])
    fresh = capi.Solver(cfg)
    try:
        fresh.set_rollout_variant("oct")
        fresh.set_control_seq(U0)
        fresh.set_noise(eps)
        sols = [solved, fresh]
        ks = [np.array([1, 2], np.int32)] * 2
        # before its first solve
        outs = _sentinels(sols, [2, 2])
        with pytest.raises(capi.MppiError) as e:
            capi.trace_rollouts_batch(sols, [2, 2], ks, outputs=outs)
        assert e.value.status == capi.ERR_STATE and _untouched(outs)
        # mppi_rollout_only alone: indices are served, a choice by weight is not
        fresh.rollout_only(cfg["start_state"])
        with pytest.raises(capi.MppiError) as e:
            capi.trace_rollouts_batch(sols, [2, 2], [ks[0], None], outputs=outs)
        assert e.value.status == capi.ERR_STATE and _untouched(outs)
        got = capi.trace_rollouts_batch(sols, [2, 2], ks)
        assert [s.debug_trace_info() for s in sols] == [1, 1]
        _same(got[1], fresh, ks[1], "after rollout_only")
        # a control cost on one member: the cost outputs are refused for the call, the rest is served
        fresh.set_noise(eps)
        fresh.compute_control(cfg["start_state"])
        plain = fresh.trace_rollouts(ks[1])
        fresh.set_cost_params(dict(cfg["cost"], steering_coeff=0.7))
        with pytest.raises(capi.MppiError) as e:
            capi.trace_rollouts_batch(sols, [2, 2], ks, outputs=outs)
        assert e.value.status == capi.ERR_UNSUPPORTED and "control cost" in str(e.value) and _untouched(outs)
        got = capi.trace_rollouts_batch(sols, [2, 2], ks, with_costs=False)
        assert sorted(got[1]) == ["controls", "first_crash", "ks", "states"]
        for k in ("states", "controls", "first_crash"):
            np.testing.assert_array_equal(_bits(got[1][k]), _bits(plain[k]), err_msg=k)
        _same(got[0], solved, ks[0], "beside it", keys=("states", "controls", "first_crash"))
        # malformed calls with real handles
        L = capi.lib()
        o = _sentinels(sols, [2, 2], with_costs=False)
        hs = (C.c_void_p * 2)(solved.h, fresh.h)
        arr = lambda key, ptr: (ptr * 2)(*[x[key].ctypes.data_as(ptr) for x in o])
        args = (arr("ks", IP), arr("states", FP), arr("controls", FP), None, None, arr("first_crash", IP))
        two = (C.c_int * 2)(2, 2)
        f = L.mppi_trace_rollouts_batch
        assert f((C.c_void_p * 2)(solved.h, solved.h), 2, two, None, *args) == capi.ERR_INVALID
        assert f(hs, 2, (C.c_int * 2)(2, -1), None, *args) == capi.ERR_INVALID
        assert f(hs, 2, (C.c_int * 2)(2, K + 1), None, *args) == capi.ERR_INVALID
        bad = np.array([0, K], np.int32)
        assert f(hs, 2, two, (IP * 2)(ks[0].ctypes.data_as(IP), bad.ctypes.data_as(IP)), *args) == capi.ERR_INVALID
        hole = (FP * 2)(o[0]["states"].ctypes.data_as(FP), None)
        assert f(hs, 2, two, None, args[0], hole, *args[2:]) == capi.ERR_INVALID
        assert _untouched(o)
    finally:
        fresh.close()


def _update_data(layers, theta):
    """[W1|b1|W2|b2|..] -> updateModel's [W1|W2|..|b1|b2|..]"""
    Ws, bs, off = [], [], 0
    for nin, nout in zip(layers[:-1], layers[1:]):
        Ws.append(theta[off:off + nin * nout])
        bs.append(theta[off + nin * nout:off + nin * nout + nout])
        off += nin * nout + nout
    return np.concatenate(Ws + bs).astype(np.float32)


def test_live_changes_are_followed_as_the_single_call_follows_them():
    own = _solved(FLEET_A[1])
    other = _fleet("A")[0]
    try:
        ks = [np.array([0, 31, 127], np.int32), np.array([4, 4], np.int32)]
        before = own.trace_rollouts(ks[0])
        layers = list(own.cfg["layers"])
        own.update_model(layers, _update_data(layers, np.asarray(own.cfg["theta"], np.float32) * np.float32(0.75)))
        got = capi.trace_rollouts_batch([own, other], [3, 2], ks)
        assert [own.debug_trace_info(), other.debug_trace_info()] == [1, 1]
        after = _same(got[0], own, ks[0], "after mppi_update_model")
        assert np.any(_bits(after["states"]) != _bits(before["states"])), "the new model changed nothing: the test shows nothing"
        lo, hi = np.asarray(own.cfg["u_lo"], np.float32) * np.float32(0.25), np.asarray(own.cfg["u_hi"], np.float32) * np.float32(0.25)
        own.set_control_limits(lo, hi)
        got = capi.trace_rollouts_batch([own, other], [3, 2], ks)
        clamped = _same(got[0], own, ks[0], "after mppi_set_control_limits")
        assert np.any(_bits(clamped["controls"]) != _bits(after["controls"]))
        _same(got[1], other, ks[1], "the member beside it")
    finally:
        own.close()


@pytest.mark.timing
def test_sixteen_handles_in_one_call_beat_sixteen_calls():
    """16 handles of 6-32-32-4, K = 1920, T = 100, their 64 largest weights each: the batch call's median is below the per-handle
    median by more than the A/A spread of the batch call itself (two interleaved series of the same call)."""
    sols = []
    try:
        for i in range(16):
            cfg = S.make_config(1920, 100, track="oval", instance=i % 4)
            s = capi.Solver(cfg)
            s.seed(7 + i, 0)
            s.compute_control(cfg["start_state"])
            sols.append(s)
        counts = [64] * 16

        def batch():
            capi.trace_rollouts_batch(sols, counts, None)

        def single():
            for s in sols:
                s.trace_rollouts(s.top_rollouts(64))

        def clock(fn):
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0
        batch()
        single()
        a, b, c = [], [], []
        for _ in range(9):
            a.append(clock(batch))
            c.append(clock(single))
            b.append(clock(batch))
        ma, mb, mc = float(np.median(a)), float(np.median(b)), float(np.median(c))
        print("TRACEFLEET_TIME 16 handles x 64 rollouts: batch %.3f ms / %.3f ms (A/A spread %.3f ms), per handle %.3f ms" % (
            1e3 * ma, 1e3 * mb, 1e3 * abs(ma - mb), 1e3 * mc))
        assert [s.debug_trace_info() for s in sols] == [1] * 16
        assert mc - max(ma, mb) > abs(ma - mb)
    finally:
        for s in sols:
            s.close()
