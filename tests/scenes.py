"""A flip-free scene (tests/ only): a problem on which every rollout's cost is a smooth function of the arithmetic, so that
every rollout of every kernel form can be held to a float64 statement (tests/ref64.py) with no allowance for "flipped" ones.

What makes the default scenes flip (tests/helpers.py: first_order_bound) are the discontinuities of the cost: the nearest-texel
lookup, the boundary / roll / slip crash thresholds, the 0.001 stabilizing switch and the basis functions' u_x > .1 switch.
Here:
  * the costmap is a linear ramp in texel space so gentle that a texel step of both car points along both axes on EVERY step
    of a rollout moves its cost by less than RAMP_FLIP_BOUND relative (a tenth of the 1e-5 bar), far below
    boundary_threshold, with track_slop = 0, behind a projective transform (w != 1).  For the same reason the texel lookup
    and the projective division are EXERCISED here, not verified: dropping the division or reading the next texel moves a
    cost by less than the bar.  The lookup is pinned elsewhere (the debug cost raster and the oval-track parity tests);
  * max_slip_ang >= pi/2 (|atan| never exceeds it), the roll and u_x stay well inside (checked by the CPU tests: no crash
    flag, u_x > 1 on every step of every rollout);
  * the start pose and its front and back points lie at least a fifth of a texel from every texel edge, and the control-cost
    coefficients are non-zero so that the clamped u / unclamped du rule is in every cost;
  * the optimization stride is 2 (the noise-free first steps are part of the bookkeeping under test), but 1 where the horizon
    is shorter than 4 steps: at T = 2 a stride of 2 would make every rollout the noise-free one.
"""
import numpy as np

from autorally_amd import params as P
from autorally_amd import synthetic as S

# The every-rollout bars (tests/test_every_rollout_gpu.py), fixed from CPU measurements before any GPU run: the oracle in
# modes 1 and 0 against ref64 on this scene, every rollout, at most 9e-7 up to T = 100 and 1.4e-6 at T = 300
# (tests/test_ref64.py holds the oracle to a fifth of them)
TOL64 = 1e-5      # a kernel's cost against ref64
TOL_MODE = 1e-5   # a kernel's cost against the oracle in the kernel form's own arithmetic mode

RAMP_BASE = 0.3          # channel-0 value at texel (0, 0); boundary_threshold is 0.65
RAMP_DI, RAMP_DJ = 1.6e-7, 1e-7   # value step per texel column / row (5 and 3 fp32 ulps of RAMP_BASE)
MAP_HALF, MAP_PPM = 64.0, 5   # [-64, 64]^2 m at 5 texels per metre: 640 x 640 texels
PROJ = (4e-4, -3e-4)     # the transform's third row: w = 1 + PROJ[0] x + PROJ[1] y
MIN_COST = 55.0          # every rollout's cost is above this: track_coeff x RAMP_BASE = 60 less the control-cost terms
# in one step (< 0.2 m at these speeds: less than a texel) the front and the back point can each cross one column and one row
# edge, which moves the step's track cost, track_coeff x (|tf| + |tb|) / 2, by at most track_coeff x (RAMP_DI + RAMP_DJ); if
# that happened on every step, the running mean would move by as much
RAMP_FLIP_BOUND = 200.0 * (RAMP_DI + RAMP_DJ) / MIN_COST


def ramp_map():
    n = int(2 * MAP_HALF * MAP_PPM)
    i = np.arange(n, dtype=np.float64)
    ch0 = (RAMP_BASE + RAMP_DI * i[None, :] + RAMP_DJ * i[:, None]).astype(np.float32)
    return S.map_rgba_from_channel0(ch0)


def ramp_transform():
    """coorTransform's R columns and translation (costs.cu:351-357) for the map's bounds, with a projective third row."""
    r_c1, r_c2, trs = P.costmap_transform(-MAP_HALF, MAP_HALF, -MAP_HALF, MAP_HALF)
    r_c1 = r_c1.copy()
    r_c2 = r_c2.copy()
    r_c1[2], r_c2[2] = np.float32(PROJ[0]), np.float32(PROJ[1])
    return r_c1, r_c2, trs


def ramp_start(x=1.0, y=-2.0, heading=0.4, speed=6.0):
    """A start pose whose front and back points (+-0.5 m along the heading) fall inside texels: the position is moved until
    both are at least a fifth of a texel from every edge of the projective grid."""
    r_c1, r_c2, trs = ramp_transform()
    n = 2 * MAP_HALF * MAP_PPM

    def frac(px, py):
        w = r_c1[2] * px + r_c2[2] * py + trs[2]
        return [((r_c1[0] * px + r_c2[0] * py + trs[0]) / w * n) % 1.0, ((r_c1[1] * px + r_c2[1] * py + trs[1]) / w * n) % 1.0]

    c, s = np.cos(heading), np.sin(heading)
    for i in range(40):  # over a texel (0.2 m) in x and in y, 0.01 m apart
        for j in range(40):
            px, py = x + 0.01 * i, y + 0.01 * j
            fr = frac(px + 0.5 * c, py + 0.5 * s) + frac(px - 0.5 * c, py - 0.5 * s) + frac(px, py)
            if all(0.2 < f < 0.8 for f in fr):
                return np.array([px, py, heading, 0.0, speed, 0.0, 0.0], np.float32)
    raise AssertionError("no start pose off the texel edges")


def gentle_model(layers, seed=4, out_scale=0.25):
    """A synthetic network (params.synthetic_model) whose output layer is scaled down, so that the roll, the speed and the
    yaw rate stay well inside the thresholds over a few hundred steps; the weights are still generic dense values."""
    layers, theta = P.synthetic_model(layers, seed=seed)
    theta = theta.copy()
    n_out = layers[-2] * layers[-1] + layers[-1]
    theta[-n_out:] *= np.float32(out_scale)
    return layers, theta


def ramp_config(K, T, layers=None, theta=None, bf_W=None, **over):
    """The problem dict of synthetic.make_config on the flip-free ramp.  layers None: the shipped 6-32-32-4 model (or the
    basis-function model when bf_W is given); any other layer list: gentle_model."""
    if bf_W is None and layers is not None and theta is None:
        layers, theta = gentle_model(layers)
    kw = dict(layers=layers, theta=theta) if layers is not None else {}
    if bf_W is not None:
        kw["bf_W"] = bf_W
    cfg = S.make_config(K, T, track="oval", **kw)
    r_c1, r_c2, trs = ramp_transform()
    cost = dict(cfg["cost"], max_slip_ang=1.6, track_slop=0.0, steering_coeff=0.7, throttle_coeff=0.4)
    cfg.update(map_rgba=ramp_map(), r_c1=r_c1, r_c2=r_c2, trs=trs, cost=cost, start_state=ramp_start(), track="ramp",
               opt_stride=2 if T >= 4 else 1)
    cfg.update(over)
    return cfg


def ramp_U(cfg, seed=7):
    """A smooth nominal control sequence inside the limits: gentle steering, throttle that keeps u_x up."""
    T = cfg["T"]
    t = np.arange(T, dtype=np.float64)
    rng = np.random.RandomState(seed)
    U = np.stack([0.08 * np.sin(t / 11.0 + rng.uniform(0, 1)), 0.35 + 0.05 * np.cos(t / 13.0)], axis=1)
    return U.astype(np.float32)
