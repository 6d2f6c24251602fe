"""Every rollout of every kernel form held to a float64 statement of the solve (tests/ref64.py), with no count allowance.

The parity tests elsewhere hold costs to the oracle statistically (p99, at most K / 200 beyond 1e-4), because their scenes
have discontinuities a one-ulp difference can cross.  On the flip-free ramp (tests/scenes.py) no rollout can flip, so a
kernel that computes one rollout slot in every 256 wrongly -- which the statistical bar accepts (tests/test_ref64.py:
test_every_rollout_bar_sees_what_the_statistical_bar_accepts) -- fails here:
  (a) every form x its layer lists x shapes (K = 64, an odd number of 64-blocks, the form's resident capacity and beyond it,
      T from 2 to 300): V bit-exact against the oracle, every cost within TOL64 of ref64 and TOL_MODE of the oracle in the
      form's own arithmetic mode;
  (b) the noise permuted along K inside its position classes: costs, V and w come back permuted bit for bit; batched
      instances in another order: every instance's bits unchanged;
  (c) the tail stage at the weighting extremes, one-chunk and streaming, against ref64's weighting, reduction and smoothing
      fed with the GPU's own costs and V;
  (d) the every-rollout bar on a batched launch, an armed solve, an armed batch and a two-iteration solve (teacher-forced).
Each case prints its measured maxima and margins."""
import functools

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import params as P
from oracle import oracle as O
from tests import branch_cases as BC
from tests import ref64 as R
from tests import scenes as SC
from tests.helpers import noise_for, oracle_mode_for, rel_err, solve_with_iterations
from tests.scenes import TOL64, TOL_MODE
from tests.test_lds16_gpu import lds16_name

pytestmark = pytest.mark.gpu

U32 = np.uint32
SHIPPED, N32X4, N64X2, N64X4 = "32x2", "32x4", "64x2", "64x4"
NET_LAYERS = {SHIPPED: None, N32X4: [6, 32, 32, 32, 32, 4], N64X2: [6, 64, 64, 4], N64X4: [6, 64, 64, 64, 64, 4],
              "16-8": [6, 16, 8, 4], "5-7": [6, 5, 7, 4], "24": [6, 24, 4], "bf": None}
NET_LAYERS.update({n: BC.NET_LAYERS[n] for n in ("65", "128x3")})   # the permutation test (b) of the "lds16" form
NET_HN = {SHIPPED: (32, 2), N32X4: (32, 4), N64X2: (64, 2), N64X4: (64, 4)}
_MULTI = ["multi2", "multi2_gen", "multi4", "multi4_gen", "multi4_tree", "multi4_tree_gen"]
_MFMA = ["quad", "block64", "fused"]
FORMS = {
    SHIPPED: ["row_exact", "row_tree"] + _MFMA + _MULTI + ["valu", "valu_lds"],
    N32X4: _MFMA + _MULTI + ["valu", "valu_lds"],
    N64X2: ["m44", "m44_chain", "row64_r16", "oct", "oct_gen"] + _MFMA + _MULTI + ["valu", "valu_lds"],
    N64X4: ["m44", "m44_chain", "row64_r16", "oct", "oct_gen"] + _MFMA + ["valu", "valu_lds"],
    "16-8": ["valu_lds"], "5-7": ["valu_lds"], "24": ["valu_lds"],
    "bf": ["bf3", "bf_row", "quad", "fused"],
}
# groups of 16 rollouts per CU a form keeps resident (csrc/abi_forms.hip: kFormRules, max_groups_per_cu)
GROUPS_PER_CU = {"row_exact": 2, "row_tree": 2, "m44": 2, "m44_chain": 2, "oct": 2, "oct_gen": 2, "quad": 1, "multi2": 2,
                 "multi2_gen": 2}
LONG_T = 300


def expected_name(variant, net):
    """What mppi_rollout_variant names the form a variant request selects."""
    if net == "bf":
        return {"bf3": "basis_funcs25_valu_3w", "bf_row": "basis_funcs25_row8w", "quad": "basis_funcs25_valu_2w",
                "fused": "basis_funcs25_valu"}[variant]
    if variant == "lds16":
        return lds16_name(NET_LAYERS[net] or [6, 32, 32, 4])
    if net not in NET_HN:
        return "valu_lds"
    if variant in ("valu", "valu_lds"):
        return {"valu": "valu_reg_lds", "valu_lds": "valu_lds"}[variant]
    h, n = NET_HN[net]
    gen = "_gen" if variant.endswith("_gen") else ""
    base = variant[:-4] if gen else variant
    tag = "h%d_l%d" % (h, n)
    return {"row_exact": "valu_row8w_" + tag, "row_tree": "valu_row8w_tree_" + tag,
            "m44": "mfma4x4x1_%s_m44_split_tree" % tag, "m44_chain": "mfma4x4x1_%s_m44_tree" % tag,
            "row64_r16": "valu_row64_r16_tree_" + tag, "oct": "mfma16x16x4_%s_oct8w%s" % (tag, gen),
            "quad": "mfma16x16x4_%s_quad4w" % tag, "block64": "mfma16x16x4_%s_fused_b64" % tag,
            "fused": "mfma16x16x4_%s_fused_b256" % tag,
            "multi2": "mfma16x16x4_%s_multi2%s" % (tag, gen), "multi4": "mfma16x16x4_%s_multi4%s" % (tag, gen),
            "multi4_tree": "mfma16x16x4_%s_multi4_tree%s" % (tag, gen)}[base]


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


@functools.lru_cache(maxsize=None)
def _cus():
    """The device's CU count, torch.cuda.get_device_properties(0).multi_processor_count -- asked in a child process: torch
    brings a HIP runtime of its own, which does not see the device in a process where the library's runtime has opened it.
    test_the_automatic_choice_at_its_switch cross-checks the count against the library's own choice."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    n = int(out.stdout.split()[-1])
    assert 32 <= n <= 1024, n
    return n


@functools.lru_cache(maxsize=None)
def _bf_W():
    import os
    return P.load_bf_npz(os.path.join(os.path.dirname(__file__), "golden", "models", "basis_function_09_12_2018.npz"))


def _cfg(net, K, T, **over):
    if net == "bf":
        return SC.ramp_config(K, T, bf_W=_bf_W(), **over)
    return SC.ramp_config(K, T, layers=NET_LAYERS[net], **over)


@functools.lru_cache(maxsize=None)
def _problem(net, K, T, inst=0):
    """One problem on the ramp; instance inst > 0 (a batched launch) has a start pose, cost parameters, nominal sequence and
    noise of its own."""
    over = {}
    if inst:
        over = dict(start_state=SC.ramp_start(x=1.0 + 3.0 * inst, y=-2.0 - 2.0 * inst, heading=0.3 + 0.05 * inst,
                                              speed=6.0 - 0.4 * inst))
    cfg = _cfg(net, K, T, **over)
    if inst:
        cfg["cost"] = dict(cfg["cost"], desired_speed=8.0 - 0.5 * inst, speed_coeff=4.25 + 0.75 * inst,
                           steering_coeff=0.7 + 0.1 * inst)
    return cfg, SC.ramp_U(cfg, seed=K % 31 + T + 7 * inst), noise_for(cfg, 1000 + T + 50 * inst)


@functools.lru_cache(maxsize=None)
def _ref64(net, K, T, inst=0):
    cfg, U0, eps = _problem(net, K, T, inst)
    costs, V, crash = R.Ref64(cfg).rollouts(cfg["start_state"], U0, eps[0])
    assert not crash.any()
    return costs


@functools.lru_cache(maxsize=None)
def _oracle(net, K, T, mode, inst=0):
    cfg, U0, eps = _problem(net, K, T, inst)
    costs, V, crash = O.Oracle(cfg, fma_mode=mode, nthreads=16).rollouts(cfg["start_state"], U0, eps[0])
    return costs, V


def _solver(cfg, variant, U0, eps, hist=None, seed=None):
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


def _hold(tag, net, K, T, got, want_name=None, inst=0):
    """The every-rollout bar: the form's name, V bit-exact against the oracle, every cost within TOL64 of ref64 and TOL_MODE
    of the oracle in the form's own mode -- on costs that differ from rollout to rollout (a rollout that read another's
    state or noise would not be seen among identical ones)."""
    if want_name is not None:
        assert got["variant"] == want_name, (got["variant"], want_name)
    assert len(np.unique(got["costs"])) > K // 2, "the rollouts of this case are not distinct"
    mode = oracle_mode_for(got["variant"])
    costs_o, V_o = _oracle(net, K, T, mode, inst)
    np.testing.assert_array_equal(got["V"].view(U32), V_o.view(U32))
    e64 = rel_err(got["costs"], _ref64(net, K, T, inst))
    eo = rel_err(got["costs"], costs_o)
    k64, ko = int(np.argmax(e64)), int(np.argmax(eo))
    print("EVERY_ROLLOUT %s net=%s K=%d T=%d form=%s mode=%d: ref64 max %.2e (k=%d, margin x%.1f)  oracle max %.2e (k=%d, "
          "margin x%.1f)" % (tag, net, K, T, got["variant"], mode, e64[k64], k64, TOL64 / max(e64[k64], 1e-30), eo[ko], ko,
                             TOL_MODE / max(eo[ko], 1e-30)))
    assert float(e64[k64]) <= TOL64, ("ref64", k64, float(e64[k64]), int(np.sum(e64 > TOL64)))
    assert float(eo[ko]) <= TOL_MODE, ("oracle mode %d" % mode, ko, float(eo[ko]), int(np.sum(eo > TOL_MODE)))


def _solve(net, K, T, variant):
    cfg, U0, eps = _problem(net, K, T)
    sol = _solver(cfg, variant, U0, eps)
    try:
        sol.compute_control(cfg["start_state"])
        return _results(sol)
    finally:
        sol.close()


# ---------------------------------------------------------------------------------------------------------------- (a)
def _capacity(variant, net):
    """Rollouts the form keeps resident at once: CUs x groups per CU x 16 where the selection table limits the form; the
    basis-function forms one wave per SIMD (abi_forms.hip form_of: three waves per 64 rollouts, two) -- but "bf_row", the row
    form's group of 16 rollouts, of which two per CU stay resident, as of the row forms; forms without a limit at
    the largest capacity of the table, two groups per CU.  Every basis-function form is named: a new one has to say its rule."""
    if net == "bf":
        return {"bf3": (4 * _cus() // 3) * 64, "quad": 4 * _cus() * 64, "bf_row": 2 * _cus() * 16, "fused": 2 * _cus() * 16}[variant]
    return GROUPS_PER_CU.get(variant, 2) * _cus() * 16


A_CASES = [(net, v, K, T) for net, vs in FORMS.items() for v in vs for K, T in ((64, 17), (1984, 100), (1984, 2))]
A_CASES += [(net, v, 1984, LONG_T) for net, v in ((SHIPPED, "row_tree"), (SHIPPED, "row_exact"), (SHIPPED, "multi4_tree"),
                                                (SHIPPED, "quad"), (SHIPPED, "valu"), (N64X2, "m44"), (N64X2, "oct"),
                                                (N64X2, "row64_r16"), (N64X4, "m44_chain"), ("5-7", "valu_lds"))]


@pytest.mark.parametrize("net,variant,K,T", A_CASES)
def test_every_rollout_of_every_form(net, variant, K, T):
    _hold("a", net, K, T, _solve(net, K, T, variant), expected_name(variant, net))


@pytest.mark.parametrize("net,variant", [(net, v) for net, vs in FORMS.items() for v in vs])
def test_every_rollout_at_and_beyond_the_resident_capacity(net, variant):
    """Every form on every layer list at its resident capacity (_capacity) and one 64-block beyond it -- a second dispatch
    round for the forms that keep their rollouts resident."""
    cap = _capacity(variant, net)
    for K in (cap, cap + 64):
        _hold("a-cap", net, K, 17, _solve(net, K, 17, variant), expected_name(variant, net))


@pytest.mark.parametrize("net,below,above", [(SHIPPED, "row_tree", "multi4_tree_gen"), (N64X2, "m44", "multi4_tree_gen")])
def test_the_automatic_choice_at_its_switch(net, below, above):
    """8192 rollouts: the two-groups-per-CU form; 8256: the multi4-tree form takes over -- both held to the same bar."""
    cap = 2 * _cus() * 16
    for K, v in ((cap, below), (cap + 64, above)):
        _hold("a-auto", net, K, 17, _solve(net, K, 17, "auto"), expected_name(v, net))


# ---------------------------------------------------------------------------------------------------------------- (b)
def _classes(K):
    """Position classes of the rollout bookkeeping: {0} (noise-free), [1, k99) (U + noise), [k99, K) (pure noise), k99 the
    first k with k >= .99 K in double."""
    k99 = int(np.ceil(.99 * K))
    assert k99 >= .99 * K and k99 - 1 < .99 * K
    return [np.arange(0, 1), np.arange(1, k99), np.arange(k99, K)]


def _perm_in_classes(K, how, rng):
    p = np.arange(K)
    for c in _classes(K):
        n = len(c)
        if how == "reverse":
            q = c[::-1]
        elif how == "rot1":
            q = np.roll(c, 1)
        elif how == "rot16":
            q = np.roll(c, 16)
        elif how == "halves":
            q = np.concatenate([c[n // 2:], c[:n // 2]])
        else:
            q = c[rng.permutation(n)]
        p[c] = q
    return p


B_FORMS = [(net, v) for net, vs in FORMS.items() if net in (SHIPPED, N64X2, N64X4, "5-7", "bf") for v in vs]
# "lds16": at K = 1984 a workgroup of 256 threads holds four waves and the last workgroup is three-quarters full -- a rollout that
# reads another wave's operand shows here; a list narrower than a tile, an odd tile count, the 8-tile instance on its largest image
B_FORMS += [("5-7", "lds16"), ("65", "lds16"), ("128x3", "lds16")]


@pytest.mark.parametrize("net,variant", B_FORMS)
def test_rearranged_noise_comes_back_rearranged_bit_for_bit(net, variant):
    """Rollout k's cost depends on its noise and its position class only: the noise permuted along K inside the classes
    gives the costs, V and w (unnormalised, the same beta) permuted bit for bit; U within 2e-6 (eta's summation order
    changes).  With every rollout of a class given the same noise, every cost of the class is the same bits."""
    K, T = 1984, 17
    cfg, U0, eps = _problem(net, K, T)
    rng = np.random.RandomState(11)
    sol = _solver(cfg, variant, U0, eps)
    try:
        sol.compute_control(cfg["start_state"])
        base = _results(sol)
        assert base["variant"] == expected_name(variant, net)
        for how in ("reverse", "rot1", "rot16", "halves", "random"):
            p = _perm_in_classes(K, how, rng)
            sol.set_control_seq(U0)
            sol.set_noise(eps[:, p])
            sol.compute_control(cfg["start_state"])
            got = _results(sol)
            for key in ("costs", "w"):
                np.testing.assert_array_equal(got[key].view(U32), base[key][p].view(U32), err_msg="%s %s" % (how, key))
            np.testing.assert_array_equal(got["V"].view(U32), base["V"][p].view(U32), err_msg=how)
            assert float(np.max(np.abs(got["U"] - base["U"]))) <= 2e-6, how
        rep = eps.copy()
        for c in _classes(K):
            rep[:, c] = eps[:, c[len(c) // 2]][:, None]
        sol.set_control_seq(U0)
        sol.set_noise(rep)
        sol.compute_control(cfg["start_state"])
        got = _results(sol)
        for c in _classes(K)[1:]:
            assert len(np.unique(got["costs"][c].view(U32))) == 1, "replicated noise, costs differ inside a class"
            assert len(np.unique(got["V"][c].reshape(len(c), -1).view(U32), axis=0)) == 1
    finally:
        sol.close()


BATCH_KS = [(SHIPPED, (1984, 4096, 640)), (SHIPPED, (1920, 1920, 3968, 256)), (N64X2, (512, 1984)), (N64X4, (1920, 3968))]


def _batch(net, Ks, T, order, armed=False):
    """The instances of a batched launch, solved in `order`; armed: the gated solve draws its own noise (mppi_arm needs the
    in-kernel generator), seeded so that it is the explicit noise of noise_for."""
    sols, states = [], []
    for i, K in enumerate(Ks):
        cfg, U0, eps = _problem(net, K, T, i)
        sols.append(_solver(cfg, "auto", U0, None if armed else eps, seed=1000 + T + 50 * i if armed else None))
        states.append(cfg["start_state"])
    try:
        sols_o = [sols[i] for i in order]
        if armed:
            capi.arm_batch(sols_o, 0.1)
        capi.compute_control_batch(sols_o, [states[i] for i in order])
        return [_results(s) for s in sols]
    finally:
        for s in sols:
            s.close()


@pytest.mark.parametrize("net,Ks", BATCH_KS)
def test_batched_instances_in_any_order_keep_their_bits(net, Ks):
    T = 33
    n = len(Ks)
    first = _batch(net, Ks, T, list(range(n)))
    for order in (list(range(n))[::-1], list(range(1, n)) + [0]):
        again = _batch(net, Ks, T, order)
        for i in range(n):
            for key in ("U", "costs", "w", "V"):
                np.testing.assert_array_equal(again[i][key].view(U32), first[i][key].view(U32),
                                              err_msg="order %r instance %d %s" % (order, i, key))
            assert np.float32(again[i]["traj_cost"]).view(U32) == np.float32(first[i]["traj_cost"]).view(U32)


# ---------------------------------------------------------------------------------------------------------------- (c)
U_FP32 = 2.0 ** -24
# the tail kernel's sums (csrc/solve_kernels.hip): per chunk of 4096 rollouts every one of 512 threads adds its 8 exps in
# order, the threads' partials go through a tree of 9 levels, the chunks' sums are added in chunk order -- eta and the
# trajectory cost sum w^2 / eta; the weighted reduction keeps the reference's order (mppi_controller.cu:246, :256-260): a
# chain of 64 rollouts per partial, the partials in order
TAIL_CHUNK, TAIL_PER_THREAD, TAIL_TREE = 4096, 8, 9


def _tail_bounds(K, gamma, costs, w64, V):
    """First-order error bounds of the tail stage against ref64 fed with the same costs and V, from the summation structure
    above (u = 2^-24):
      * a weight: the exponent gamma (J - beta) is formed in fp32 (two roundings: 2^-23 of it absolute) and expf adds two
        ulps, eps_k = gamma (J_k - beta) 2^-23 + 2^-22; |dw_k| <= w_k eps_k, plus the smallest normal where the device
        flushes a subnormal weight to zero;
      * eta and sum w^2 / eta (positive terms): a sum of depth d = 8 + 9 + chunks errs by at most d u of its value;
      * the weighted reduction (terms of both signs): Higham's running error bound of its own order, u x (the magnitudes of
        every partial sum of every 64-rollout chain and of the ordered sum of the chains), plus u per product and division;
        the weights' errors move U by sum_k w_k / eta eps_k |V_k - U|, eta's by its relative error x |U|;
      * the smoothing: 5 taps of total weight 47/35 on U, plus its own 8 u.
    Returns (per-weight bound, bound on |dU| per [t, j], relative bound on the trajectory cost)."""
    J = costs.astype(np.float64)
    eps_k = gamma * (J - J.min()) * 2.0 ** -23 + 2.0 ** -22
    wbound = w64 * eps_k + 1.2e-38
    eta = float(w64.sum())
    wn = w64 / eta
    chunks = -(-K // TAIL_CHUNK)
    d_sum = TAIL_PER_THREAD + TAIL_TREE + chunks
    rel_eta = d_sum * U_FP32 + float(np.sum(wn * eps_k))
    V = V.astype(np.float64).reshape(K, -1)
    terms = wn[:, None] * V
    pad = -K % 64
    chains = np.concatenate([terms, np.zeros((pad, terms.shape[1]))]).reshape(-1, 64, terms.shape[1])
    part = np.cumsum(chains, axis=1)
    run = np.abs(part).sum(axis=(0, 1)) + np.abs(np.cumsum(part[:, -1], axis=0)).sum(axis=0)
    U_raw = terms.sum(axis=0)
    dU_raw = U_FP32 * (run + 2 * np.abs(terms).sum(axis=0)) + np.einsum("k,kc->c", wn * eps_k, np.abs(V - U_raw)) + \
        rel_eta * np.abs(U_raw)
    bU = 47.0 / 35.0 * (dU_raw.reshape(-1, 2).max(axis=0) + 8 * U_FP32 * np.abs(U_raw).reshape(-1, 2).max(axis=0))
    w2 = w64 * w64
    btc = (d_sum + 3) * U_FP32 + rel_eta + 2 * float(np.sum(w2 * eps_k) / np.sum(w2))
    return wbound, bU, btc


TAIL_KS = [64, 4096, 4160, 16384, 65600]


@pytest.mark.parametrize("gamma", [1e-3, 0.15, 5.0, 50.0])
@pytest.mark.parametrize("K", TAIL_KS)
def test_the_tail_stage_at_the_weighting_extremes(K, gamma):
    """w, eta (through U and the trajectory cost), the trajectory cost and U against ref64's weighting, reduction and smoothing
    fed with the GPU's own costs and V, within _tail_bounds; and against the oracle's fp32 reduction in the kernel's own
    order fed with the GPU's weights and an exactly rounded eta, within the 2e-6 of tests/test_stream_tail_gpu.py -- the
    check that sees one rollout left out of a reduction of 65 600 equal weights (about 1.5e-5 / |V_k - U|)."""
    T = 17
    cfg, U0, eps = _problem(SHIPPED, K, T)
    cfg = dict(cfg, gamma=gamma)
    hist = np.array([0.01, 0.3, -0.02, 0.33], np.float32)
    sol = _solver(cfg, "auto", U0, eps, hist)
    try:
        sol.compute_control(cfg["start_state"])
        got = _results(sol)
    finally:
        sol.close()
    e64 = rel_err(got["costs"], _ref64(SHIPPED, K, T))
    assert float(e64.max()) <= TOL64, float(e64.max())
    r = R.Ref64(cfg)
    w64, beta, eta64, tc64 = r.weights(got["costs"])
    U64 = r.savgol(r.weighted_reduction(w64, eta64, got["V"]), hist)
    wb, bU, btc = _tail_bounds(K, r.gamma, got["costs"], w64, got["V"])
    dw = np.abs(got["w"].astype(np.float64) - w64)
    assert np.all(dw <= wb), (int(np.argmax(dw - wb)), float(np.max(dw - wb)))
    dU = np.abs(got["U"] - U64).max(axis=0)
    dtc = abs(got["traj_cost"] - tc64) / tc64
    orc = O.Oracle(cfg, fma_mode=1, nthreads=16)
    eta_exact = np.float32(np.sum(got["w"], dtype=np.float64))
    U_ord = orc.savgol(orc.weighted_reduction(got["w"], eta_exact, got["V"]), hist)
    d_ord = float(np.max(np.abs(got["U"] - U_ord)))
    n_live = int(np.sum(got["w"] > 0))
    print("TAIL K=%d gamma=%g: %d of %d weights > 0, eta %.4g; |dw| max %.2e, |dU| %.2e %.2e (bound %.2e %.2e), traj cost "
          "rel %.2e (bound %.2e); in the kernel's order %.2e (bound 2e-6)" % (
              K, gamma, n_live, K, eta64, float(dw.max()), dU[0], dU[1], bU[0], bU[1], dtc, btc, d_ord))
    assert np.all(dU <= bU) and dtc <= btc
    assert d_ord <= 2e-6
    if gamma == 50.0:  # most weights below the smallest normal: a few rollouts carry about all the weight
        assert float(np.mean(w64 < 2.0 ** -126)) > 0.5
        print("TAIL K=%d gamma=50: the largest weight carries %.3f of eta" % (K, float(w64.max()) / eta64))
    if gamma == 1e-3:
        assert float(got["w"].min()) > 0.9


# ---------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("net,Ks", BATCH_KS[:1] + BATCH_KS[2:3])
@pytest.mark.parametrize("armed", [False, True])
def test_every_rollout_of_a_batched_launch(net, Ks, armed):
    T = 33
    outs = _batch(net, Ks, T, list(range(len(Ks))), armed=armed)
    for i, (K, got) in enumerate(zip(Ks, outs)):
        _hold("d-batch%s" % ("-armed" if armed else ""), net, K, T, got, inst=i)


@pytest.mark.parametrize("net,K,T", [(SHIPPED, 4096, 100), (SHIPPED, 1920, 100), (N64X2, 512, 100)])
def test_every_rollout_of_an_armed_solve(net, K, T):
    cfg, U0, eps = _problem(net, K, T)
    sol = _solver(cfg, "auto", U0, None, seed=1000 + T)  # the gated solve draws its own noise: the same as eps
    try:
        sol.arm(0.1)
        assert sol.is_armed()
        sol.compute_control(cfg["start_state"])
        assert not sol.is_armed()
        got = _results(sol)
    finally:
        sol.close()
    _hold("d-armed", net, K, T, got)


@pytest.mark.parametrize("net,K,variant", [(SHIPPED, 4096, "auto"), (SHIPPED, 12352, "auto"), (N64X2, 1984, "oct"),
                                           ("bf", 1984, "auto")])
def test_every_rollout_of_a_two_iteration_solve_teacher_forced(net, K, variant):
    T = 40
    cfg = _cfg(net, K, T, num_iters=2)
    U0 = SC.ramp_U(cfg)
    hist = np.array([0.01, 0.3, -0.02, 0.33], np.float32)
    eps = noise_for(cfg, 77)
    got, its, name = solve_with_iterations(cfg, variant, U0, hist, eps)
    if variant != "auto":
        assert name == expected_name(variant, net), name
    refs = R.teacher_forced(cfg, its, U0, hist, eps)
    orc = O.Oracle(dict(cfg, num_iters=1), fma_mode=oracle_mode_for(name), nthreads=16)
    for i in range(2):
        U_in = U0 if i == 0 else its["U_raw"][i - 1]
        costs_o, V_o, _ = orc.rollouts(cfg["start_state"], U_in, eps[i])
        np.testing.assert_array_equal(its["V"][i].view(U32), V_o.view(U32))
        e64 = rel_err(its["costs"][i], refs[i]["costs"])
        eo = rel_err(its["costs"][i], costs_o)
        print("EVERY_ROLLOUT d-iter%d net=%s K=%d T=%d form=%s: ref64 max %.2e  oracle max %.2e" % (
            i, net, K, T, name, float(e64.max()), float(eo.max())))
        assert float(e64.max()) <= TOL64 and float(eo.max()) <= TOL_MODE
        # what the cost differences move the weighted mean by, to first order (helpers.first_order_bound): dw_k / w_k =
        # -gamma (dJ_k - sum_j w_j dJ_j), so |dU| <= 2 gamma sum_k w_k |dJ_k| max |V - U|; plus 2e-6 of fp32 summation
        dJ = np.abs(its["costs"][i].astype(np.float64) - refs[i]["costs"])
        wn = refs[i]["w"] / refs[i]["eta"]
        fo = 2 * float(np.float32(cfg["gamma"])) * float(np.sum(wn * dJ)) * float(np.max(np.abs(refs[i]["V"] - refs[i]["U_raw"][None])))
        dU = float(np.max(np.abs(its["U_raw"][i] - refs[i]["U_raw"])))
        print("    |dU| %.2e (bound %.2e)" % (dU, 2e-6 + fo))
        assert dU <= 2e-6 + fo
    assert float(np.max(np.abs(got["U"] - refs[1]["U"]))) <= 2e-6 + fo
    assert abs(got["traj_cost"] - refs[1]["traj_cost"]) <= (1e-5 + 4 * float(np.float32(cfg["gamma"])) * float(dJ.max())) * refs[1]["traj_cost"]
