"""Every DECIDED rollout of every kernel form held to float64 where the cost's branches FIRE (tests/scenes.py: the patchwork
for the track branches -- texel lookup behind the projective division, slop, boundary flag from either car point -- and the
tilt-slide for the state branches -- the sticky roll flag set after the update, the slip limit crossed both ways, both controls
cut at both limits, l2 / l1 speed cost, two discounts).

The flip-free ramp of tests/test_every_rollout_gpu.py keeps every discontinuity out of reach; the parity and fuzz tests reach
them but forgive whatever differs by more than 1e-4 as "flipped", up to 3 % of a draw.  Here ref64 says on the host, before any
GPU result is looked at, which rollouts are decided: every margin to a discontinuity (ref64.Ref64.trace) at least the DELTA of
its class (scenes.py, measured on the CPU).  The bar, per case:
  * the form's name is the one requested; V bit-equal to the oracle for ALL rollouts;
  * every decided rollout within TOL64 of ref64 and within TOL_MODE of the oracle in the form's own mode, no allowance;
  * undecided rollouts (at most UNDECIDED_CAP of K, asserted) finite.
tests/test_branch_scenes.py shows on the CPU that this bar rejects a flag one step early or late, a flag that is not sticky,
a boundary test of the front point only, a signed slip test, round for floor, a dropped division, the unclamped control in the
control cost and a scaled slop compare -- several of which the statistical bars accept.
Each case prints its maxima, the margins to the bar and the counts of decided, crashed and slipping rollouts."""
import numpy as np
import pytest

from autorally_amd import capi
from tests import branch_cases as BC
from tests import scenes as SC
from tests.helpers import oracle_mode_for, rel_err
from tests.scenes import TOL64, TOL_MODE
from tests.test_every_rollout_gpu import FORMS, GROUPS_PER_CU, NET_LAYERS, _cus, _results, _solver, expected_name
from tests.test_lds16_gpu import lds16_name
from tests.test_lds44_gpu import lds44_name
from tests.test_lds128_gpu import lds128_name

pytestmark = pytest.mark.gpu

U32 = np.uint32
assert all(BC.NET_LAYERS[n] == NET_LAYERS[n] for n in NET_LAYERS)


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


def _want(variant, net):
    if variant == "lds44":
        return lds44_name(BC.NET_LAYERS[net])
    if variant == "lds128":
        return lds128_name(BC.NET_LAYERS[net])
    if variant == "lds16":   # exact: the oracle's mode 1
        return lds16_name(BC.NET_LAYERS[net] or [6, 32, 32, 4])
    return expected_name(variant, net)


def _hold(tag, scene, net, K, T, got, want_name=None, inst=0):
    """The bar of this file on one solve's results.  The decided set and the cap come from ref64 on the host."""
    tr = BC.trace(scene, net, K, T, inst)
    dec = tr["decided"]
    n_und = int(K - dec.sum())
    assert n_und <= SC.UNDECIDED_CAP * K, (n_und, K)
    if want_name is not None:
        assert got["variant"] == want_name, (got["variant"], want_name)
    mode = oracle_mode_for(got["variant"])
    costs_o, V_o = BC.oracle(scene, net, K, T, mode, inst)
    np.testing.assert_array_equal(got["V"].view(U32), V_o.view(U32))
    assert np.all(np.isfinite(got["costs"])), "a cost is not finite"
    e64 = rel_err(got["costs"], tr["costs"])
    eo = rel_err(got["costs"], costs_o)
    d64, do = np.where(dec, e64, 0.0), np.where(dec, eo, 0.0)
    k64, ko = int(np.argmax(d64)), int(np.argmax(do))
    print("BRANCH_ROLLOUT %s %s net=%s K=%d T=%d form=%s mode=%d: %d decided (%d crashed, %d over the slip limit), %d undecided; "
          "decided: ref64 max %.2e (k=%d, margin x%.1f)  oracle max %.2e (k=%d, margin x%.1f); undecided: ref64 max %.2e" % (
              tag, scene, net, K, T, got["variant"], mode, int(dec.sum()), int(np.sum(dec & (tr["crash"] > 0))),
              int(np.sum(dec & tr["over"].any(axis=1))), n_und, d64[k64], k64, TOL64 / max(d64[k64], 1e-30), do[ko], ko,
              TOL_MODE / max(do[ko], 1e-30), float(e64[~dec].max()) if n_und else 0.0))
    assert float(d64[k64]) <= TOL64, ("ref64", k64, float(d64[k64]), int(np.sum(d64 > TOL64)), int(tr["first"][k64]), int(tr["source"][k64]))
    assert float(do[ko]) <= TOL_MODE, ("oracle mode %d" % mode, ko, float(do[ko]), int(np.sum(do > TOL_MODE)))


def _solve(scene, net, K, T, variant):
    cfg, U0, eps = BC.problem(scene, net, K, T)
    sol = _solver(cfg, variant, U0, eps)
    try:
        sol.compute_control(cfg["start_state"])
        return _results(sol)
    finally:
        sol.close()


FORM_CASES = [(net, v) for net, vs in FORMS.items() for v in vs] + [(net, "lds44") for net in BC.LDS44_NETS] + \
    [(net, "lds128") for net in BC.LDS128_NETS] + [(net, "lds16") for net in BC.LDS16_NETS]


@pytest.mark.parametrize("K,T", BC.SHAPES)
@pytest.mark.parametrize("net,variant", FORM_CASES)
@pytest.mark.parametrize("scene", BC.SCENES)
def test_every_decided_rollout_of_every_form(scene, net, variant, K, T):
    _hold("form", scene, net, K, T, _solve(scene, net, K, T, variant), _want(variant, net))


@pytest.mark.parametrize("net,variant", [("32x2", "row_tree"), ("64x2", "m44"), ("32x2", "multi4_tree"), ("32x3", "lds44"),
                                         ("128x2", "lds128")])
def test_beyond_the_resident_capacity_on_the_patchwork(net, variant):
    """One 64-block more than the form keeps resident, a second dispatch round; the fan of rollouts is cut by a boundary
    texel during the last three steps, so that crashed and uncrashed rollouts sit side by side in both rounds
    (tests/test_branch_scenes.py asserts the shares for this K)."""
    K = GROUPS_PER_CU.get(variant, 2) * _cus() * 16 + 64
    _hold("capacity", "patchwork", net, K, 17, _solve("patchwork", net, K, 17, variant), _want(variant, net))


# net -> (the variant requested, the form that runs) of the armed solves
ARMED = {"32x2": ("auto", "row_tree"), "64x2": ("auto", "m44"), "bf": ("bf_row", "bf_row")}


@pytest.mark.parametrize("K,T", BC.SHAPES[1:])
@pytest.mark.parametrize("net", list(ARMED))
@pytest.mark.parametrize("scene", BC.SCENES)
def test_every_decided_rollout_of_an_armed_solve(scene, net, K, T):
    """The automatic choice (at K = 1984 the row-tree form on the shipped list, "m44" on 6-64-64-4) and, by name, the "bf_row" form
    of the basis-function model (its automatic choice, "bf3", has no gated kernel), armed (mppi_arm): the gated solve draws its
    own noise, seeded to be the explicit noise."""
    cfg, U0, eps = BC.problem(scene, net, K, T)
    sol = _solver(cfg, ARMED[net][0], U0, None, seed=BC.noise_seed(T))
    try:
        sol.arm(0.1)
        assert sol.is_armed()
        sol.compute_control(cfg["start_state"])
        assert not sol.is_armed()
        got = _results(sol)
    finally:
        sol.close()
    _hold("armed", scene, net, K, T, got, expected_name(ARMED[net][1], net))


@pytest.mark.parametrize("armed", [False, True], ids=["plain", "armed"])
@pytest.mark.parametrize("net,variant", [("64x2", "auto"), ("32x3", "lds44"), ("128x2", "lds128")])
def test_every_decided_rollout_of_a_shared_launch(net, variant, armed):
    """mppi_compute_control_batch on two handles of one layer list, K = 1984 and 1920, on the patchwork, the second handle on
    another start pose with other cost parameters: ONE rollout launch (mppi_debug_launch_info), gated after mppi_arm_batch;
    each instance held to the bar."""
    T, Ks = 100, (1984, 1920)
    sols, states = [], []
    try:
        for i, K in enumerate(Ks):
            cfg, U0, eps = BC.problem("patchwork", net, K, T, i)
            sols.append(_solver(cfg, variant, U0, None if armed else eps, seed=BC.noise_seed(T, i) if armed else None))
            states.append(cfg["start_state"])
        if armed:
            capi.arm_batch(sols, 0.1)
            assert all(s.is_armed() for s in sols)
        capi.compute_control_batch(sols, states)
        assert not any(s.is_armed() for s in sols)
        infos = [s.debug_launch_info() for s in sols]
        assert infos == [(2, 1 if armed else 0)] * 2, infos
        outs = [_results(s) for s in sols]
    finally:
        for s in sols:
            s.close()
    for i, (K, got) in enumerate(zip(Ks, outs)):
        _hold("shared%s" % ("-armed" if armed else ""), "patchwork", net, K, T, got, _want("m44" if variant == "auto" else variant, net), inst=i)
