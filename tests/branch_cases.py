"""The cases of the branch scenes (tests/scenes.py: patchwork, tilt-slide) shared by tests/test_branch_scenes.py (CPU: caps,
coverage, the oracle against ref64, mutants) and tests/test_branch_rollouts_gpu.py (every kernel form): problems, ref64 traces,
decided sets and oracle results, each computed once."""
import functools
import os

import numpy as np

from autorally_amd import params as P
from oracle import oracle as O
from tests import ref64 as R
from tests import scenes as SC
from tests.helpers import noise_for

SCENES = ["patchwork", "tilt_l2", "tilt_l1"]
SHAPES = [(64, 17), (1984, 37), (1984, 100)]
# the layer lists of tests/test_every_rollout_gpu.py (FORMS) and those the "lds44", "lds128" and "lds16" forms are held on here
NET_LAYERS = {"32x2": None, "32x4": [6, 32, 32, 32, 32, 4], "64x2": [6, 64, 64, 4], "64x4": [6, 64, 64, 64, 64, 4],
              "16-8": [6, 16, 8, 4], "5-7": [6, 5, 7, 4], "24": [6, 24, 4], "bf": None,
              "32x3": [6, 32, 32, 32, 4], "16-24": [6, 16, 24, 4], "64x6": [6, 64, 64, 64, 64, 64, 64, 4],
              "128x2": [6, 128, 128, 4], "33-97-66": [6, 33, 97, 66, 4], "65": [6, 65, 4], "128x3": [6, 128, 128, 128, 4]}
LDS44_NETS, LDS128_NETS = ["32x3", "16-24", "64x6"], ["128x2", "33-97-66"]
# "lds16": the 4-tile and the 8-tile instance, a layer narrower than a tile, half-full last tiles, odd tile counts (6-65-4: five,
# a single tile behind two pairs), no middle layer, seven weight layers, the largest image
LDS16_NETS = ["32x2", "5-7", "24", "16-24", "65", "33-97-66", "64x6", "128x2", "128x3"]


@functools.lru_cache(maxsize=None)
def bf_W():
    return P.load_bf_npz(os.path.join(os.path.dirname(__file__), "golden", "models", "basis_function_09_12_2018.npz"))


def config(scene, net, K, T, **over):
    kw = dict(bf_W=bf_W()) if net == "bf" else dict(layers=NET_LAYERS[net])
    if scene == "patchwork":
        return SC.patchwork_config(K, T, **kw, **over)
    return SC.tilt_slide_config(K, T, variant=scene[5:], **kw, **over)


def noise_seed(T, inst=0):
    return 1000 + T + 50 * inst


@functools.lru_cache(maxsize=None)
def problem(scene, net, K, T, inst=0):
    """(cfg, U0, eps).  Instance 1 (the second handle of a shared launch, patchwork only): another start pose, other cost
    parameters, its own nominal sequence and noise."""
    if inst:
        assert scene == "patchwork"
        cfg = config(scene, net, K, T, start=SC.PATCH_START_2[SC.family(NET_LAYERS[net], None), SC.patch_horizon(T)])
        cfg["cost"] = dict(cfg["cost"], desired_speed=7.0, speed_coeff=5.0, steering_coeff=0.9, crash_coeff=8000.0, track_slop=0.045)
    else:
        cfg = config(scene, net, K, T)
    return cfg, SC.ramp_U(cfg, seed=K % 31 + T + 7 * inst), noise_for(cfg, noise_seed(T, inst))


@functools.lru_cache(maxsize=None)
def trace(scene, net, K, T, inst=0):
    cfg, U0, eps = problem(scene, net, K, T, inst)
    tr = R.Ref64(cfg).trace(cfg["start_state"], U0, eps[0])
    tr["decided"] = SC.decided(cfg, tr)
    return tr


@functools.lru_cache(maxsize=None)
def oracle(scene, net, K, T, mode, inst=0):
    cfg, U0, eps = problem(scene, net, K, T, inst)
    costs, V, crash = O.Oracle(cfg, fma_mode=mode, nthreads=16).rollouts(cfg["start_state"], U0, eps[0])
    return costs, V
