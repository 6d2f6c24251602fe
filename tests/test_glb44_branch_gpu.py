"""The "glb44" rollout form held to float64 where the cost's branches FIRE and outside the box the other scenes keep the state in:
the branch scenes of tests/branch_cases.py (patchwork, tilt-slide) and the edge scenes of tests/edge_cases.py (border, crawl,
cap, stiff), at those files' own bars, K and T -- tests/test_branch_rollouts_gpu.py's _hold and edge_cases.hold, imported:
  * the form's name; V bit-equal to the mode-1 oracle for ALL rollouts;
  * every decided rollout (ref64 says which, on the host) within TOL64 of ref64 and TOL_MODE of the oracle, no allowance;
  * undecided rollouts finite; a rollout capped on every step exactly (float)1e12.
"glb44" on 6-129-4 (three halves, one neuron in the third) and on 6-200-256-4 (four ragged halves and four input sets, an image
beyond the LDS: resident and streamed quads), "glb44_r1" on 6-65-4 (two halves with all but one quad streamed).  The two wide
lists get names in branch_cases.NET_LAYERS while this file runs; the file itself is as it was."""
from unittest import mock

import pytest

from autorally_amd import capi
from tests import branch_cases as BC
from tests import edge_cases as EC
from tests.test_branch_rollouts_gpu import _hold, _solve as _branch_solve
from tests.test_edge_rollouts_gpu import _solve as _edge_solve
from tests.test_glb44_gpu import EXTRA_LISTS, glb44_name

pytestmark = pytest.mark.gpu

CASES = [("129", "glb44"), ("200-256", "glb44"), ("65", "glb44_r1")]


def _layers(net):
    return EXTRA_LISTS.get(net) or BC.NET_LAYERS[net]


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"
    with mock.patch.dict(BC.NET_LAYERS, EXTRA_LISTS):
        yield


@pytest.mark.parametrize("K,T", BC.SHAPES)
@pytest.mark.parametrize("net,variant", CASES)
@pytest.mark.parametrize("scene", BC.SCENES)
def test_every_decided_rollout_on_the_branch_scenes(scene, net, variant, K, T):
    _hold(variant, scene, net, K, T, _branch_solve(scene, net, K, T, variant), glb44_name(_layers(net)))


EDGE_CASES = [(scene, net, v, K, T) for scene in EC.SCENES for net, v in CASES for K, T in EC.shapes(scene)]


@pytest.mark.parametrize("scene,net,variant,K,T", EDGE_CASES)
def test_every_decided_rollout_on_the_edge_scenes(scene, net, variant, K, T):
    """A case runs every PART of its scene (six borders and corners, three start speeds, three cap settings, four headings), a
    solve each."""
    for part in EC.parts(scene, net):
        cfg, U0, eps = EC.problem(scene, part, net, K, T)
        EC.hold(variant, scene, part, net, K, T, _edge_solve(cfg, U0, eps, variant), glb44_name(_layers(net)))
