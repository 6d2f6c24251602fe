"""Every DECIDED rollout of every kernel form held to float64 OUTSIDE the box the other scenes keep the state in
(tests/scenes.py: border -- car points off the map, the clamp of the texel lookup at every border and two corners, headings in
the quadrants -7 .. 5; crawl -- |u_x| under 0.001 m/s, u_x negative, the slip limit crossed both ways, the basis functions'
u_x > .1; cap -- step costs replaced by (float)1e12, and just under it; stiff -- hidden units whose exp2 runs to inf and to 0).

The bar is that of tests/test_branch_rollouts_gpu.py (tests/edge_cases.py: hold): the form's name; V bit-equal to the oracle for
ALL rollouts; every decided rollout within TOL64 of ref64 and TOL_MODE of the oracle in the form's own mode, no allowance;
undecided rollouts (at most UNDECIDED_CAP of K) finite; a rollout ref64 caps on every step exactly (float)1e12.  ref64 says on
the host which rollouts are decided, before any GPU result is looked at; tests/test_edge_scenes.py shows on the CPU that the
bar rejects ten mutants of the clamp, the speed guard, the basis functions' switch and the cap.
  (a) every form x its layer lists x the four scenes x (K, T) = (64, 17), (1984, 37), the border also (1984, 100); a case runs
      every PART of its scene (six borders and corners, three start speeds, three cap settings, four headings), a solve each;
  (b) beyond the resident capacity, every workgroup size of "lds16", armed, and the shared two-handle launch, on the border and
      the crawl;
  (c) non-finite and huge start states for every form: capped rollouts exactly (float)1e12, the others held to the oracle, U to
      ref64's tail stages fed with the GPU's own costs and V;
  (d) mppi_trace_rollouts on 16 rollouts chosen from ref64's record.
Each solve prints its maxima, the margins to the bars and the event shares of its decided rollouts."""
import numpy as np
import pytest

from autorally_amd import capi
from tests import edge_cases as EC
from tests import ref64 as R
from tests import trace_cases as TC
from tests.helpers import oracle_mode_for
from tests.test_branch_rollouts_gpu import ARMED, FORM_CASES, _want
from tests.test_every_rollout_gpu import GROUPS_PER_CU, _cus, _results, _solver, expected_name
from tests.test_lds16_pack import packer, workgroup_threads  # noqa: F401 (packer: a fixture)

pytestmark = pytest.mark.gpu

U32 = np.uint32


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


def _solve(cfg, U0, eps, variant, state=None, hist=None):
    sol = _solver(cfg, variant, U0, eps, hist=hist)
    try:
        sol.compute_control(cfg["start_state"] if state is None else state)
        return _results(sol)
    finally:
        sol.close()


# ---------------------------------------------------------------------------------------------------------------- (a)
A_CASES = [(scene, net, v, K, T) for scene in EC.SCENES for net, v in FORM_CASES for K, T in EC.shapes(scene)]


@pytest.mark.parametrize("scene,net,variant,K,T", A_CASES)
def test_every_decided_rollout_of_every_form(scene, net, variant, K, T):
    for part in EC.parts(scene, net):
        cfg, U0, eps = EC.problem(scene, part, net, K, T)
        EC.hold("form", scene, part, net, K, T, _solve(cfg, U0, eps, variant), _want(variant, net))


# ---------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("net,variant", [("32x2", "row_tree"), ("64x2", "m44"), ("32x2", "multi4_tree"), ("32x3", "lds44"),
                                         ("128x2", "lds128")])
def test_beyond_the_resident_capacity_on_the_border(net, variant):
    """One 64-block more than the form keeps resident, a second dispatch round, at the two corners: rollouts that left the map
    and rollouts that did not sit side by side in both rounds."""
    K = GROUPS_PER_CU.get(variant, 2) * _cus() * 16 + 64
    for part in EC.CAPACITY_PARTS:
        cfg, U0, eps = EC.problem("border", part, net, K, 17)
        EC.hold("capacity", "border", part, net, K, 17, _solve(cfg, U0, eps, variant), _want(variant, net))


@pytest.mark.parametrize("net,per_cu,threads", EC.LDS16_THREADS)
def test_every_workgroup_size_of_lds16_on_the_border(net, per_cu, threads, packer):  # noqa: F811
    """The "lds16" form where its launcher's rule picks workgroups of 512 threads (6-128-128-128-4 at 128 rollouts per CU: one
    workgroup per CU) and of 1024 (6-64x6-4 at 256 per CU), at the two corners; K > 4096, so the streaming tail runs behind the
    rollouts: U within 2e-6 of ref64's weighting, reduction and smoothing fed with the solve's own costs and V, as
    edge_cases.hold_start_state holds it."""
    cus = _cus()
    K, T, layers = per_cu * cus, 17, EC.NET_LAYERS[net]
    # the library's own rule (lds16_block_threads, what the launcher calls with the handle's CU count) on this device's CUs
    assert packer(layers, launch=(K, cus))[3] == workgroup_threads(layers, K, cus) == threads, (packer(layers, launch=(K, cus)), threads)
    for part in EC.CAPACITY_PARTS:
        cfg, U0, eps = EC.problem("border", part, net, K, T)
        got = _solve(cfg, U0, eps, "lds16", hist=EC.START_HIST)
        EC.hold("threads%d" % threads, "border", part, net, K, T, got, _want("lds16", net))
        r = R.Ref64(cfg)
        w, beta, eta, tc = r.weights(got["costs"])
        dU = float(np.max(np.abs(r.savgol(r.weighted_reduction(w, eta, got["V"]), EC.START_HIST) - got["U"])))
        print("EDGE_ROLLOUT threads%d border/%s net=%s K=%d: |dU| %.2e against ref64's tail stages (bar 2e-6)" % (threads, part, net, K, dU))
        assert np.all(np.isfinite(got["U"])) and dU <= 2e-6, dU


@pytest.mark.parametrize("net", list(ARMED))
@pytest.mark.parametrize("scene", ["border", "crawl"])
def test_every_decided_rollout_of_an_armed_solve(scene, net):
    """The automatic choice (at K = 1984 the row-tree form on the shipped list, "m44" on 6-64-64-4) and, by name, the "bf_row" form
    of the basis-function model (its automatic choice has no gated kernel), armed (mppi_arm): the gated solve draws its own
    noise, seeded to be the explicit noise."""
    K, T = EC.SHAPES[1]
    for part in EC.parts(scene, net):
        cfg, U0, eps = EC.problem(scene, part, net, K, T)
        sol = _solver(cfg, ARMED[net][0], U0, None, seed=EC.noise_seed(T))
        try:
            sol.arm(0.1)
            assert sol.is_armed()
            sol.compute_control(cfg["start_state"])
            assert not sol.is_armed()
            got = _results(sol)
        finally:
            sol.close()
        EC.hold("armed", scene, part, net, K, T, got, expected_name(ARMED[net][1], net))


# the basis-function pair on the border only: the crawl's shared parts are network start speeds
SHARED_CASES = [(scene, net, v) for scene in EC.SHARED for net, v in (("64x2", "auto"), ("32x3", "lds44"), ("128x2", "lds128"))] + \
    [("border", "bf", "bf_row")]


def _launched_together(variant, Ks):
    """What batch_together (csrc/abi_solve.hip) decides for the pair.  The network pairs here: one launch.  The "bf_row" pair
    falls under the row forms' rule -- every dynamics wave of every group a SIMD of its own, four waves per 16 rollouts against four
    SIMDs per CU: 1984 + 1920 rollouts are 976 waves, one launch from 244 CUs on (the MI355X has 256); on a smaller device the
    handles are solved, and armed, one by one."""
    return variant != "bf_row" or sum(4 * (K // 16) for K in Ks) <= 4 * _cus()


@pytest.mark.parametrize("armed", [False, True], ids=["plain", "armed"])
@pytest.mark.parametrize("scene,net,variant", SHARED_CASES)
def test_every_decided_rollout_of_a_shared_launch(scene, net, variant, armed):
    """mppi_compute_control_batch on two handles of one layer list (or of the basis-function model), K = 1984 and 1920, the
    second handle on another part of the scene (the opposite corner, a negative start speed) with other cost parameters: ONE
    rollout launch (mppi_debug_launch_info reports what _launched_together says), gated after mppi_arm_batch; each instance
    held to the bar."""
    T, parts = EC.SHARED[scene]
    sols, states = [], []
    try:
        for i, K in enumerate(EC.SHARED_KS):
            cfg, U0, eps = EC.problem(scene, parts[i], net, K, T, i)
            sols.append(_solver(cfg, variant, U0, None if armed else eps, seed=EC.noise_seed(T, i) if armed else None))
            states.append(cfg["start_state"])
        if armed:
            capi.arm_batch(sols, 0.1)
            assert all(s.is_armed() for s in sols)
        capi.compute_control_batch(sols, states)
        assert not any(s.is_armed() for s in sols)
        infos = [s.debug_launch_info() for s in sols]
        assert infos == [(2 if _launched_together(variant, EC.SHARED_KS) else 1, 1 if armed else 0)] * 2, infos
        outs = [_results(s) for s in sols]
    finally:
        for s in sols:
            s.close()
    for i, (K, got) in enumerate(zip(EC.SHARED_KS, outs)):
        EC.hold("shared%s" % ("-armed" if armed else ""), scene, parts[i], net, K, T, got, _want("m44" if variant == "auto" else variant, net),
                inst=i)


# ---------------------------------------------------------------------------------------------------------------- (c)
# "lds44" and "lds128" on a list whose widths are no multiples of four: the padded k steps of a layer read lanes that hold no neuron
RAGGED_CASES = [("5-7", "lds44"), ("5-7", "lds128")]   # ("5-7", "lds16") and its other ragged lists are among FORM_CASES


@pytest.mark.parametrize("K", EC.START_KS)
@pytest.mark.parametrize("net,variant", FORM_CASES + RAGGED_CASES)
def test_non_finite_and_huge_start_states_for_every_form(net, variant, K):
    """NaN speed (a NaN cost, capped), +inf x, NaN heading (NaN through the look-ahead points: the clamp's NaN -> texel 0),
    -inf yaw rate, a speed of 1e30 (the speed cost overflows to inf, capped) and x = 1e20 (finite, far off the map) on the ramp."""
    for which in EC.START_STATES:
        cfg, U0, eps, state = EC.start_state_problem(net, K, which)
        got = _solve(cfg, U0, eps, variant, state=state, hist=EC.START_HIST)
        EC.hold_start_state("form", net, K, which, got, _want(variant, net))


# ---------------------------------------------------------------------------------------------------------------- (d)
TRACE_FORMS = [("32x2", "row_exact"), ("64x2", "oct"), ("64x2", "m44"), ("32x3", "lds44"), ("bf", "bf3"), ("33-97-66", "lds16")]
N_TRACED = 16


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(U32)


def _chosen(scene, part, tr, K, T):
    """16 rollouts from ref64's record: one that left the map across the part's border, one that came back, one that reversed,
    one capped part-way (where the case has such), the rest decided ones at random."""
    dec = tr["decided"]
    anyout = (tr["out_w"] | tr["out_e"] | tr["out_s"] | tr["out_n"])[:, 1:]
    back = ((np.cumsum(anyout, axis=1) > 0) & tr["inside"][:, 1:]).any(axis=1)
    cap = tr["capped"][:, 1:]
    wanted = [tr["out_" + part][:, 1:].any(axis=1) if scene == "border" else anyout.any(axis=1), back, tr["reversed"][:, 1:].any(axis=1),
              tr["slow"][:, 1:].any(axis=1), cap.any(axis=1) & ~cap.all(axis=1)]
    ks, kinds = [], []
    for i, m in enumerate(wanted):
        idx = np.nonzero(m & dec)[0]
        if idx.size:
            ks.append(int(idx[idx.size // 2]))
            kinds.append(i)
    rest = np.random.RandomState(K + T).permutation(np.nonzero(dec)[0])
    ks += [int(k) for k in rest if k not in ks][:N_TRACED - len(ks)]
    return np.array(ks, np.int32), kinds


@pytest.mark.parametrize("net,variant", TRACE_FORMS)
@pytest.mark.parametrize("scene", ["border", "crawl", "cap"])
def test_the_trace_kernel_on_chosen_rollouts(scene, net, variant):
    """mppi_trace_rollouts (control-cost coefficients 0, as tests/trace_cases.py: the library refuses the cost outputs
    otherwise): states within TOL_STATE of the float64 loop over the solve's own applied controls, the clamped controls equal,
    the folded step costs equal to the trace's costs -- and to mppi_get_results bit for bit on the order-exact forms --, the
    first crash step ref64's on the decided rollouts."""
    K, T = EC.SHAPES[1]
    for part in EC.parts(scene, net):
        cfg, U0, eps = EC.problem(scene, part, net, K, T, "trace")
        ref = EC.trace(scene, part, net, K, T, "trace")
        ks, kinds = _chosen(scene, part, ref, K, T)
        sol = _solver(cfg, variant, U0, eps)
        try:
            sol.compute_control(cfg["start_state"])
            got = _results(sol)
            tr = sol.trace_rollouts(ks)
        finally:
            sol.close()
        EC.hold("traced", scene, part, net, K, T, got, _want(variant, net), inst="trace")
        exact = oracle_mode_for(got["variant"]) == 1
        V = got["V"][ks]
        lo, hi = np.asarray(cfg["u_lo"], np.float32), np.asarray(cfg["u_hi"], np.float32)
        np.testing.assert_array_equal(_bits(tr["controls"]), _bits(np.clip(V, lo, hi)))
        np.testing.assert_array_equal(_bits(tr["states"][:, 0]), _bits(np.tile(np.asarray(cfg["start_state"], np.float32), (len(ks), 1))))
        dev = np.abs(tr["states"].astype(np.float64) - TC.loop64(cfg, V))
        fold = TC.fold_step_costs(tr["step_costs"])
        wrong = tr["first_crash"] != ref["first"][ks]
        print("EDGE_TRACE %s/%s net=%s form=%s (%s): rollouts %s (kinds %s); states max dev %.2e (TOL_STATE x%.1f); costs differ from "
              "get_results on %d of %d; first crash wrong on %d" % (
                  scene, part, net, got["variant"], "exact" if exact else "re-associating", ks.tolist(), kinds, dev.max(),
                  TC.TOL_STATE / max(dev.max(), 1e-30), int(np.sum(_bits(tr["costs"]) != _bits(got["costs"][ks]))), len(ks), int(wrong.sum())))
        assert dev.max() <= TC.TOL_STATE
        np.testing.assert_array_equal(_bits(fold), _bits(tr["costs"]))
        if exact:
            np.testing.assert_array_equal(_bits(tr["costs"]), _bits(got["costs"][ks]))
        assert not wrong.any(), (ks[wrong], tr["first_crash"][wrong], ref["first"][ks][wrong])
