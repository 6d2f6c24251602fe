"""The float64 statement of the solve (tests/ref64.py) and the flip-free ramp scene (tests/scenes.py) on the CPU: ref64 against
the reference-generated NN fixtures and the basis-function restatement, the oracle in both of its plain arithmetic modes
against ref64 on EVERY rollout of the ramp, the scene's own flip-freedom, and a record of the gap the every-rollout bar
closes (the statistical bar of the GPU parity tests accepts a corrupted rollout slot in every 256; this one does not)."""
import os

import numpy as np
import pytest

from autorally_amd import params as P
from oracle import oracle as O
from tests import ref64 as R
from tests import scenes as SC
from tests.scenes import TOL64, TOL_MODE
from tests.helpers import load_nn_golden, noise_for, rel_err
from tests.test_oracle_golden import MODELS


NETS = [None, [6, 32, 32, 32, 32, 4], [6, 64, 64, 4], [6, 64, 64, 64, 64, 4], [6, 16, 8, 4], [6, 5, 7, 4], [6, 24, 4], "bf"]


def _bf_W(golden_dir):
    return P.load_bf_npz(os.path.join(golden_dir, "models", "basis_function_09_12_2018.npz"))


def _cfg(golden_dir, net, K, T, **over):
    if net == "bf":
        return SC.ramp_config(K, T, bf_W=_bf_W(golden_dir), **over)
    return SC.ramp_config(K, T, layers=net, **over)


@pytest.mark.parametrize("name", MODELS)
def test_ref64_network_against_the_reference_python(golden_dir, name):
    """The reference's Python NN utilities (float64 weights) wrote the fixtures; ref64 reads the packed fp32 weights, so the
    two differ by the weights' rounding only (2^-24 relative per weight)."""
    g = load_nn_golden(golden_dir)
    layers, theta = P.load_model_npz(os.path.join(golden_dir, "models", name + ".npz"))
    cfg = dict(SC.ramp_config(8, 4), layers=layers, theta=theta, negate_yaw_der=bool(g[name + "/negate_yaw_der"][0]))
    r = R.Ref64(cfg)
    s = g[name + "/states"].astype(np.float32).astype(np.float64)
    u = g[name + "/controls"].astype(np.float32).astype(np.float64)
    d = g[name + "/state_ders"]
    sd = r.state_deriv(s, u)
    err = np.abs(sd - d) / np.maximum(1.0, np.abs(d))
    assert float(err.max()) < 2e-6, float(err.max())
    if name == MODELS[0]:
        out = r.nn(g["sample_in"].astype(np.float32).astype(np.float64)[None])[0]
        np.testing.assert_allclose(out, g["sample_out"], atol=2e-6, rtol=0)


def test_ref64_basis_functions_against_the_numpy_restatement_and_the_oracle(golden_dir):
    from tests.test_basis_funcs import _samples
    cfg = SC.ramp_config(8, 4, bf_W=_bf_W(golden_dir))
    orc = O.Oracle(cfg)
    s, u = _samples(300, seed=5)
    s64, u64 = s.astype(np.float64), u.astype(np.float64)
    phi = R.basis_k(s64, u64)
    ref = np.stack([R._np_basis(s[i], u[i]) for i in range(s.shape[0])])
    np.testing.assert_allclose(phi, ref, rtol=1e-14, atol=1e-300)  # the same float64 expressions, over K rows (vector pow: an ulp)
    sd = R.Ref64(cfg).state_deriv(s64, u64)
    np.testing.assert_allclose(sd[:, 3:], ref @ cfg["bf_W"].astype(np.float64).T, rtol=1e-12, atol=1e-15)
    assert np.all(sd[:, 2] == -s64[:, 6])
    so = np.stack([orc.state_deriv(s[i], u[i]) for i in range(s.shape[0])])
    np.testing.assert_allclose(so[:, 3:], sd[:, 3:], rtol=2e-4, atol=2e-4)


@pytest.mark.parametrize("net", NETS, ids=lambda n: "default" if n is None else "bf" if n == "bf" else "x".join(map(str, n)))
def test_oracle_both_modes_against_ref64_on_every_rollout(golden_dir, net):
    """Every rollout's cost of the fp32 oracle, with and without fused multiply-adds, within TOL64 of ref64; the applied
    controls within an ulp; weights, eta, trajectory cost and the smoothed controls of the whole solve."""
    K, T = (2048, 100) if net in (None, "bf") else (1024, 60)
    cfg = _cfg(golden_dir, net, K, T)
    U0 = SC.ramp_U(cfg)
    hist = np.array([0.01, 0.3, -0.02, 0.33], np.float32)
    eps = noise_for(cfg, 1234)
    ref = R.Ref64(cfg).compute_control(cfg["start_state"], U0, hist, eps)
    assert not ref["crash"].any()
    for mode in (1, 0):
        o = O.Oracle(cfg, fma_mode=mode, nthreads=8).compute_control(cfg["start_state"], U0, hist, eps)
        err = rel_err(o["costs"], ref["costs"])
        print("ref64 %s mode %d: max %.2e over %d rollouts (bar %.0e)" % (net, mode, float(err.max()), K, TOL64))
        assert float(err.max()) <= 0.2 * TOL64, float(err.max())
        assert float(np.max(np.abs(o["V"][-1] - ref["V"]))) <= 1.2e-7  # U + eps nu rounded in fp32, twice (|V| < 2)
        w64 = np.exp(-ref64_gamma(cfg) * (ref["costs"] - ref["costs"].min()))
        np.testing.assert_allclose(ref["w"], w64, rtol=1e-15)
        # dw = gamma w (dJ - d beta): each within the cost bar above, plus expf's own rounding
        assert float(np.max(np.abs(o["w"] - ref["w"]))) <= 2 * ref64_gamma(cfg) * 0.2 * TOL64 * float(ref["costs"].max()) + 2e-7
        assert abs(o["traj_cost"] - ref["traj_cost"]) <= 1e-5 * ref["traj_cost"]
        assert float(np.max(np.abs(o["U"] - ref["U"]))) <= 2e-6


def ref64_gamma(cfg):
    return float(np.float32(cfg["gamma"]))


def test_oracle_two_iterations_against_ref64_teacher_forced(golden_dir):
    cfg = _cfg(golden_dir, None, 1024, 50, num_iters=2)
    U0 = SC.ramp_U(cfg)
    hist = np.zeros(4, np.float32)
    eps = noise_for(cfg, 99)
    orc = O.Oracle(dict(cfg, num_iters=1), fma_mode=1, nthreads=8)
    U_raw, costs = [], []
    U = U0
    for i in range(2):
        c, V, _ = orc.rollouts(cfg["start_state"], U, eps[i])
        w, _, eta, _ = orc.weights(c)
        U = orc.weighted_reduction(w, eta, V)
        U_raw.append(U)
        costs.append(c)
    refs = R.teacher_forced(cfg, {"U_raw": np.stack(U_raw)}, U0, hist, eps)
    assert len(refs) == 2
    for i in range(2):
        assert float(rel_err(costs[i], refs[i]["costs"]).max()) <= 0.2 * TOL64
        assert float(np.max(np.abs(U_raw[i] - refs[i]["U_raw"]))) <= 2e-6
    whole = orc.compute_control(cfg["start_state"], U0, hist, eps, num_iters=2)
    assert float(np.max(np.abs(whole["U"] - refs[1]["U"]))) <= 2e-6


@pytest.mark.parametrize("net,K,T", [(None, 4096, 100), ([6, 64, 64, 4], 2048, 100), ([6, 32, 32, 32, 32, 4], 1024, 100),
                                     ([6, 64, 64, 64, 64, 4], 1024, 100), ([6, 5, 7, 4], 1024, 100), ("bf", 2048, 100),
                                     (None, 2048, 300), (None, 1984, 2), (None, 1984, 17)])
def test_the_ramp_scene_has_no_flips(golden_dir, net, K, T):
    """The oracle's two arithmetic modes (a re-rounding of every multiply-add) agree to 1e-6 on every rollout, no crash flag
    is set, and the switches stay out of reach: u_x > 1 (the 0.001 stabilizing and the basis functions' .1 switch), |roll| and
    |slip| far from 1.57 / max_slip_ang."""
    cfg = _cfg(golden_dir, net, K, T)
    assert SC.RAMP_FLIP_BOUND <= 1e-6 and cfg["cost"]["max_slip_ang"] >= np.pi / 2 and cfg["cost"]["track_slop"] == 0.0
    U0 = SC.ramp_U(cfg)
    eps = noise_for(cfg, 4321)[0]
    c1, _, cr1 = O.Oracle(cfg, fma_mode=1, nthreads=8).rollouts(cfg["start_state"], U0, eps)
    c0, _, cr0 = O.Oracle(cfg, fma_mode=0, nthreads=8).rollouts(cfg["start_state"], U0, eps)
    assert not cr1.any() and not cr0.any()
    err = rel_err(c1, c0)
    assert float(err.max()) <= 1e-6, float(err.max())
    assert float(c1.min()) >= SC.MIN_COST and float(c1.max()) < 0.65 * 200 + 1e3
    # the switches, on every step of every rollout (ref64's trajectories)
    r = R.Ref64(cfg)
    V, _ = r.controls(U0, eps)
    s = np.tile(cfg["start_state"].astype(np.float64), (K, 1))
    lo = np.inf
    hi_roll = hi_slip = hi_map = 0.0
    for t in range(T):
        u = np.clip(V[:, t], r.u_lo, r.u_hi)
        s = s + r.state_deriv(s, u) * r.dt
        lo = min(lo, float(s[:, 4].min()))
        hi_roll = max(hi_roll, float(np.abs(s[:, 3]).max()))
        hi_slip = max(hi_slip, float(np.abs(np.arctan(s[:, 5] / np.abs(s[:, 4]))).max()))
        hi_map = max(hi_map, float(np.abs(s[:, :2]).max()))
    assert lo > 1.0 and hi_roll < 0.5 and hi_slip < 1.0, (lo, hi_roll, hi_slip)
    assert hi_map < SC.MAP_HALF - 1.0  # the texel clamp at the border is never reached


def test_every_rollout_bar_sees_what_the_statistical_bar_accepts():
    """One rollout slot in every 256 (k % 256 == 255) computing 5e-4 relative wrong -- a bad DPP source row, an LDS slot two
    waves share, a second dispatch round reading stale state: the bar of the GPU parity tests (at most K / 200 rollouts
    beyond 1e-4, p99 of the relative error < 5e-6, |dU| <= 1e-4) accepts it; the every-rollout bar rejects it."""
    cfg = SC.ramp_config(4096, 100)
    U0 = SC.ramp_U(cfg)
    hist = np.zeros(4, np.float32)
    eps = noise_for(cfg, 1234)
    orc = O.Oracle(cfg, fma_mode=1, nthreads=8)
    ref = orc.compute_control(cfg["start_state"], U0, hist, eps)
    K = cfg["K"]
    bad = np.arange(K) % 256 == 255
    costs = ref["costs"].copy()
    costs[bad] = (costs[bad].astype(np.float64) * (1.0 + 5e-4)).astype(np.float32)
    w, _, eta, tc = orc.weights(costs)
    U = orc.savgol(orc.weighted_reduction(w, eta, ref["V"][-1]), hist)
    err = rel_err(costs, ref["costs"])
    # the statistical bar passes
    assert int(np.sum(err > 1e-4)) <= max(K // 200, 1)
    assert float(np.percentile(err, 99)) < 5e-6
    assert float(np.max(np.abs(U - ref["U"]))) <= 1e-4
    assert abs(tc - ref["traj_cost"]) <= 1e-4 * abs(ref["traj_cost"])
    # the every-rollout bar fails, on exactly the corrupted slots
    e64 = rel_err(costs, R.Ref64(cfg).rollouts(cfg["start_state"], U0, eps[0])[0])
    assert float(e64.max()) > TOL64 and np.array_equal(e64 > TOL64, bad)
    assert float(err.max()) > TOL_MODE
