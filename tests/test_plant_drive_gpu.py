"""A plant of its own on the device (mppi_set_plant_model, mppi_plant_drive_batch -> csrc/plant_drive_fleet.hip): the plants of a whole
fleet stepped at pose rate under the interpolated feed-forward and feedback law, one wave per controller.  Every case that claims the
kernel asserts on_device == 1 (mppi_debug_plant_drive_info): a silent fall-back to the host text cannot pass.
  1. distance: the fleet of tests/plant_drive_cases.py for every call (periods, substeps, feedback) -- device and host text
     (mppi_debug_plant_drive_host, fed the handle's own sequences and gains) each within the project's state bound of 1e-4 of the
     float64 restatement, applied controls within 1e-5; the device's largest distance at most 4 x the host text's largest (the rule
     of tests/test_nominal_fleet_gpu.py);
  2. exact bits where the heading stays 0 (the plant's output neuron 3 zeroed, psi = s6 = 0), with feedback, m in {1, 3};
  3. equivalence: m = 1, no feedback, no plant model -- the first `periods` rows of mppi_nominal_traj_batch, bit for bit;
  4. mppi_set_plant_model sets, clears and refuses;
  5. plumbing: n = 2 / 64 / 65 / 130 against fleets of two; n = 1 and a basis-function handle take the host text; feedback without
     a DDP result; an armed outsider stays armed; determinism.
Each case prints what it measured."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import params as P
from autorally_amd import synthetic as S
from tests import plant_drive_cases as PC
from tests.helpers import warm_U

pytestmark = pytest.mark.gpu

U32 = np.uint32
STATE_BOUND = 1e-4    # the project's state bound (tests/test_nominal_fleet_gpu.py)
CONTROL_BOUND = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    assert hasattr(capi.lib(), "mppi_plant_drive_batch"), "the library has no plant drive"


def _close(sols):
    for s in sols:
        s.close()


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, what
    np.testing.assert_array_equal(a.view(U32), b.view(U32), err_msg=what)


def _on_device(sols):
    return [s.debug_plant_drive_info() for s in sols]


def _solver(p):
    sol = capi.Solver(p["cfg"])
    sol.set_control_seq(p["U"])
    sol.set_ddp_weights(PC.DDP_Q, PC.DDP_R, PC.DDP_QF)
    if p["plant"] is not None:
        sol.set_plant_model(p["plant"]["layers"], p["plant"]["theta"], p["plant"]["negate"])
    return sol


def _prepared(probs):
    """Solvers of the problems with their nominal solutions and gains from ONE launch (mppi_nominal_and_gains_batch)."""
    sols = [_solver(p) for p in probs]
    seqs = capi.nominal_and_gains_batch(sols, [p["x0"] for p in probs])
    assert [s.debug_nominal_and_gains_info() for s in sols] == [1] * len(sols)
    gains = [s.feedback_gains()["feedback"] for s in sols]
    return sols, seqs, gains


@functools.lru_cache(maxsize=None)
def _fleet():
    """The fleet of tests/plant_drive_cases.py (computed once, not changed)."""
    probs = PC.problems()
    return (probs,) + _prepared(probs)


def _host_text(p, seq, K, periods, substeps):
    pc = p["plant_cfg"]
    return capi.debug_plant_drive_host(pc["layers"], pc["theta"], pc["negate_yaw_der"], np.float32(1.0 / PC.HZ), p["cfg"]["u_lo"],
                                       p["cfg"]["u_hi"], p["x_plant"], seq[0], seq[1], K, periods, substeps)


# ------------------------------------------------------------------------------------------------------------------ 1
def test_device_and_host_text_stay_within_the_state_bound_of_float64():
    probs, sols, seqs, gains = _fleet()
    assert [s.debug_plant_model_info() for s in sols] == [0 if p["plant"] is None else len(p["plant"]["layers"]) for p in probs]
    dev_max = host_max = 0.0
    for periods, substeps, feedback in PC.CALLS:
        got_x, got_u = capi.plant_drive_batch(sols, [p["x_plant"] for p in probs], seqs, periods, substeps, feedback)
        assert _on_device(sols) == [1] * len(sols)
        for i, p in enumerate(probs):
            K = gains[i] if feedback else None
            hx, hu = _host_text(p, seqs[i], K, periods, substeps)
            rx, ru, facts = PC.drive64(p["plant_cfg"], p["cfg"]["u_lo"], p["cfg"]["u_hi"], p["x_plant"], seqs[i][0], seqs[i][1], K, periods, substeps)
            dx, du = float(np.max(np.abs(got_x[i] - rx))), float(np.max(np.abs(got_u[i] - ru)))
            ex, eu = float(np.max(np.abs(hx - rx))), float(np.max(np.abs(hu - ru)))
            same = int(np.sum(got_x[i].view(U32) == hx.view(U32))) + int(np.sum(got_u[i].view(U32) == hu.view(U32)))
            print("PLANTDRIVE %s P=%d m=%d feedback=%d: from float64: device state %.2e controls %.2e, host text state %.2e controls %.2e "
                  "(bounds 1e-4 / 1e-5); %d of %d output floats bit-equal to the host text; largest |du| %.2e, clamp %s" % (
                      PC.tag(i), periods, substeps, feedback, dx, du, ex, eu, same, 7 + hu.size, facts["max_du"], facts["clamped"]))
            assert np.all(np.isfinite(got_x[i])) and np.all(np.isfinite(got_u[i]))
            assert dx <= STATE_BOUND and ex <= STATE_BOUND, (PC.tag(i), periods, substeps, feedback)
            assert du <= CONTROL_BOUND and eu <= CONTROL_BOUND, (PC.tag(i), periods, substeps, feedback)
            dev_max, host_max = max(dev_max, dx), max(host_max, ex)
    print("PLANTDRIVE fleet: largest state distance from float64: device %.2e, host text %.2e" % (dev_max, host_max))
    # both are fp32 evaluations of one operation sequence, apart by at most an ulp of sin / cos per step
    assert dev_max <= 4.0 * host_max, (dev_max, host_max)


def test_two_calls_in_a_row_give_the_same_bits():
    probs, sols, seqs, _ = _fleet()
    xs = [p["x_plant"] for p in probs]
    a = capi.plant_drive_batch(sols, xs, seqs, 2, 3, True)
    b = capi.plant_drive_batch(sols, xs, seqs, 2, 3, True)
    assert _on_device(sols) == [1] * len(sols)
    _bits(a[0], b[0], "states")
    for i in range(len(sols)):
        _bits(a[1][i], b[1][i], PC.tag(i))


# ------------------------------------------------------------------------------------------------------------------ 2
def test_exact_bits_where_the_heading_stays_zero():
    """The plant's output neuron 3 has zero weights and bias, psi = s6 = 0 at the start: the heading stays exactly 0, sin / cos are 0
    and 1 on both sides, and device and host text agree BIT FOR BIT -- the interpolation in double, the fmaf chain of the feedback, the
    NaN rule, the clamp, the network and the Euler step with dt / m."""
    probs = PC.problems(flat=True)
    sols, seqs, gains = _prepared(probs)
    try:
        for m in (1, 3):
            got_x, got_u = capi.plant_drive_batch(sols, [p["x_plant"] for p in probs], seqs, 2, m, True)
            assert _on_device(sols) == [1] * len(sols)
            for i, p in enumerate(probs):
                hx, hu = _host_text(p, seqs[i], gains[i], 2, m)
                fx, _ = _host_text(p, seqs[i], None, 2, m)
                assert hx[2] == 0.0 and hx[6] == 0.0, "the heading stays 0"
                assert np.any(hx != fx), "the feedback changes the state"
                diff = int(np.sum(got_x[i].view(U32) != hx.view(U32))) + int(np.sum(got_u[i].view(U32) != hu.view(U32)))
                print("PLANTDRIVE flat %s m=%d: %d of %d output floats differ from the host text's bits" % (PC.tag(i), m, diff, 7 + hu.size))
                _bits(got_x[i], hx, "flat %s m=%d: state" % (PC.tag(i), m))
                _bits(got_u[i], hu, "flat %s m=%d: applied controls" % (PC.tag(i), m))
    finally:
        _close(sols)


# ------------------------------------------------------------------------------------------------------------------ 3, 4
def test_one_substep_without_feedback_or_plant_model_is_the_nominal_replay_and_the_model_sets_clears_and_refuses(golden_dir):
    probs = PC.problems()[1:4]
    sols = [_solver(p) for p in probs]
    W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    bf = capi.Solver(S.make_config(64, PC.T, track="oval", bf_W=W, opt_stride=1))
    try:
        xs = [p["x_plant"] for p in probs]
        seqs = capi.nominal_traj_batch(sols, xs)
        with_plant = capi.plant_drive_batch(sols, xs, seqs, 3, 1, False)
        assert [s.debug_plant_model_info() for s in sols] == [3, 3, 6]
        # refusals change nothing
        s0, p0 = sols[0], probs[0]["plant"]
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        th = np.ascontiguousarray(p0["theta"], np.float32)
        for layers, n in (([6, 24, 4], th.size - 1), ([5, 24, 4], th.size), ([6, 24, 3], th.size), ([6, 300, 4], 2404), ([6], 0),
                          ([6, 8, 8, 8, 8, 8, 8, 8, 4], 600)):
            ls = (C.c_int * len(layers))(*layers)
            assert s0.L.mppi_set_plant_model(s0.h, ls, len(layers), th.ctypes.data_as(fp), n, 0) == capi.ERR_INVALID, layers
        assert s0.L.mppi_set_plant_model(s0.h, None, 0, th.ctypes.data_as(fp), th.size, 0) == capi.ERR_INVALID
        assert s0.L.mppi_set_plant_model(s0.h, (C.c_int * 3)(6, 24, 4), 3, None, th.size, 0) == capi.ERR_INVALID
        assert s0.debug_plant_model_info() == 3
        again = capi.plant_drive_batch(sols, xs, seqs, 3, 1, False)
        _bits(again[0], with_plant[0], "a refused model leaves the plant as it was")
        with pytest.raises(capi.MppiError) as e:
            bf.set_plant_model([6, 8, 4], np.zeros(92, np.float32))
        assert e.value.status == capi.ERR_INVALID and bf.debug_plant_model_info() == 0
        # cleared: the plant is the handle's own network, and m = 1 without feedback is the nominal replay's first rows
        for s in sols:
            s.set_plant_model()
        assert [s.debug_plant_model_info() for s in sols] == [0, 0, 0]
        got_x, got_u = capi.plant_drive_batch(sols, xs, seqs, 3, 1, False)
        assert _on_device(sols) == [1] * 3
        for i in range(3):
            _bits(got_x[i], seqs[i][0][3], "handle %d: the state after three periods is row 3 of state_seq" % i)
            _bits(got_u[i], seqs[i][1][:3], "handle %d: the applied controls are control_seq's first rows" % i)
            assert np.any(got_x[i] != with_plant[0][i]), "the plant model did change the drive"
        # set again: the bits of before
        for s, p in zip(sols, probs):
            s.set_plant_model(p["plant"]["layers"], p["plant"]["theta"], p["plant"]["negate"])
        _bits(capi.plant_drive_batch(sols, xs, seqs, 3, 1, False)[0], with_plant[0], "the model set again")
        print("PLANTDRIVE equivalence: m = 1 without feedback or plant model equals mppi_nominal_traj_batch's first 3 rows bit for bit; "
              "set / clear / set again and 9 refusals behave")
    finally:
        _close(sols + [bf])


# ------------------------------------------------------------------------------------------------------------------ 5
@functools.lru_cache(maxsize=None)
def _pool(n=130, T=5):
    """n small handles on one map (6-8-4 and 6-5-7-4 alternate) with plants of the other list, distinct states, controls and gains
    (computed once, not changed) -> (solvers, states, sequences)."""
    base_map = S.make_config(64, T, track="oval")
    sols, states = [], []
    for i in range(n):
        layers, other = ([6, 8, 4], [6, 5, 7, 4]) if i % 2 == 0 else ([6, 5, 7, 4], [6, 8, 4])
        l, th = P.synthetic_model(layers, seed=i % 17)
        cfg = dict(base_map, K=64, T=T, layers=l, theta=np.array(th, np.float32), negate_yaw_der=bool(i % 3), hz=(20, 50, 100)[i % 3])
        sol = capi.Solver(cfg)
        sol.set_control_seq(warm_U(cfg, seed=i))
        sol.set_ddp_weights(PC.DDP_Q, PC.DDP_R, PC.DDP_QF)
        pl, pth = P.synthetic_model(other, seed=(i + 5) % 17)
        sol.set_plant_model(pl, np.array(pth, np.float32), bool(i % 2))
        st = np.array(cfg["start_state"], np.float32)
        st[0] += np.float32(0.1 * i)
        st[4] += np.float32(0.05 * (i % 9))
        sols.append(sol)
        states.append(st)
    seqs = capi.nominal_and_gains_batch(sols, states)
    return sols, states, seqs


@pytest.mark.parametrize("n", [2, 64, 65, 130])
def test_sizes_against_fleets_of_two(n):
    sols, states, seqs = _pool()
    moved = [s + np.float32(0.03) for s in states]
    got_x, got_u = capi.plant_drive_batch(sols[:n], moved[:n], seqs[:n], 2, 3, True)
    assert _on_device(sols[:n]) == [1] * n
    for at in range(0, n - 1, 2):
        px, pu = capi.plant_drive_batch(sols[at:at + 2], moved[at:at + 2], seqs[at:at + 2], 2, 3, True)
        _bits(got_x[at:at + 2], px, "n=%d handles %d, %d: states" % (n, at, at + 1))
        for q in range(2):
            _bits(got_u[at + q], pu[q], "n=%d handle %d: applied controls" % (n, at + q))
    assert np.all(np.isfinite(got_x))
    print("PLANTDRIVE sizes: n = %d in launches of up to 64 equals fleets of two bit for bit" % n)


def test_one_handle_and_a_basis_function_handle_take_the_host_text(golden_dir):
    probs, sols, seqs, gains = _fleet()
    p = probs[2]
    got_x, got_u = capi.plant_drive_batch([sols[2]], [p["x_plant"]], [seqs[2]], 2, 4, True)
    assert _on_device([sols[2]]) == [0]
    hx, hu = _host_text(p, seqs[2], gains[2], 2, 4)
    _bits(got_x[0], hx, "one handle: the host text's state")
    _bits(got_u[0], hu, "one handle: the host text's applied controls")
    W = P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))
    cfg = S.make_config(64, PC.T, track="oval", bf_W=W, opt_stride=1)
    bf = capi.Solver(cfg)
    try:
        bf.set_control_seq(warm_U(cfg, seed=3))
        x = np.array(cfg["start_state"], np.float32)
        bseq = bf.nominal_traj(x)
        mixed = [sols[1], bf, sols[3]]
        mx, mu = capi.plant_drive_batch(mixed, [probs[1]["x_plant"], x, probs[3]["x_plant"]], [seqs[1], bseq, seqs[3]], 2, 1, False)
        assert _on_device(mixed) == [0, 0, 0]
        _bits(mx[1], bseq[0][2], "the basis-function handle's plant is its own model: row 2 of its host replay")
        _bits(mu[1], bseq[1][:2], "the basis-function handle's applied controls")
        _bits(mx[0], _host_text(probs[1], seqs[1], None, 2, 1)[0], "a network handle beside it: the host text")
        print("PLANTDRIVE fall-backs: n = 1 and a set with a basis-function handle ran the host text, with its bits")
    finally:
        bf.close()


def test_feedback_without_a_ddp_result_is_refused_and_writes_nothing():
    probs = PC.problems()[:2]
    sols = [_solver(p) for p in probs]
    try:
        xs = [p["x_plant"] for p in probs]
        seqs = capi.nominal_traj_batch(sols, xs)   # no gains
        out = (np.full((2, 7), 9.0, np.float32), [np.full((6, 2), 9.0, np.float32) for _ in sols])
        with pytest.raises(capi.MppiError) as e:
            capi.plant_drive_batch(sols, xs, seqs, 2, 3, True, outputs=out)
        assert e.value.status == capi.ERR_STATE
        for bad in (dict(periods=0), dict(periods=PC.T), dict(substeps=0), dict(substeps=17)):
            args = dict(periods=2, substeps=3)
            args.update(bad)
            with pytest.raises(capi.MppiError) as e:
                capi.plant_drive_batch(sols, xs, seqs, args["periods"], args["substeps"], False, outputs=out)
            assert e.value.status == capi.ERR_INVALID, bad
        with pytest.raises(capi.MppiError) as e:
            capi.plant_drive_batch([sols[0], sols[0]], xs, seqs, 2, 3, False, outputs=out)
        assert e.value.status == capi.ERR_INVALID
        assert np.all(out[0] == 9.0) and all(np.all(a == 9.0) for a in out[1])
        capi.plant_drive_batch(sols, xs, seqs, 2, 3, False, outputs=out)   # without feedback the same set runs
        assert np.all(out[0] != 9.0) and _on_device(sols) == [1, 1]
    finally:
        _close(sols)


def test_an_armed_outsider_stays_armed():
    probs, sols, seqs, _ = _fleet()
    base = S.make_config(192, PC.T, layers=list(PC.NET), track="oval", opt_stride=1)
    outsider, twin = capi.Solver(base), capi.Solver(base)
    try:
        x0 = np.array(base["start_state"], np.float32)
        pl, pth = P.synthetic_model([6, 24, 4], seed=2)
        for s in (outsider, twin):
            s.set_control_seq(warm_U(base, seed=7))
            s.seed(77, 0)
            s.compute_control(x0)
            s.slide_control_seq(1)
        outsider.set_plant_model(pl, pth, False)   # the first call allocates the image: not beside a gated launch
        outsider.arm(0.05)
        assert outsider.is_armed()
        outsider.set_plant_model(pl, np.array(pth, np.float32) * np.float32(1.01), True)   # touches no solve state
        assert outsider.is_armed(), "mppi_set_plant_model leaves an armed handle armed"
        capi.plant_drive_batch(sols, [p["x_plant"] for p in probs], seqs, 2, 4, True)
        assert _on_device(sols) == [1] * len(sols)
        assert outsider.is_armed(), "the batched drive leaves a handle outside the set armed"
        outsider.compute_control(x0)   # opens the armed solve
        twin.compute_control(x0)
        _bits(outsider.get_results()["U"], twin.get_results()["U"], "the armed solve of the handle outside the set")
    finally:
        _close([outsider, twin])
