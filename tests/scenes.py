"""A flip-free scene (tests/ only): a problem on which every rollout's cost is a smooth function of the arithmetic, so that
every rollout of every kernel form can be held to a float64 statement (tests/ref64.py) with no allowance for "flipped" ones.

What makes the default scenes flip (tests/helpers.py: first_order_bound) are the discontinuities of the cost: the nearest-texel
lookup, the boundary / roll / slip crash thresholds, the 0.001 stabilizing switch and the basis functions' u_x > .1 switch.
Here:
  * the costmap is a linear ramp in texel space so gentle that a texel step of both car points along both axes on EVERY step
    of a rollout moves its cost by less than RAMP_FLIP_BOUND relative (a tenth of the 1e-5 bar), far below
    boundary_threshold, with track_slop = 0, behind a projective transform (w != 1).  For the same reason the texel lookup
    and the projective division are EXERCISED here, not verified: dropping the division or reading the next texel moves a
    cost by less than the bar.  The lookup and the division are VERIFIED on the patchwork scene below (patchwork_config: coarse
    texels whose neighbours differ by 0.03 or more, held to float64 rollout by rollout by tests/test_branch_rollouts_gpu.py);
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


def ramp_start(x=1.0, y=-2.0, heading=0.4, speed=6.0, roll=0.0, u_y=0.0, n=2 * MAP_HALF * MAP_PPM, step=0.01):
    """A start pose whose front and back points (+-0.5 m along the heading) fall inside texels: the position is moved until
    both are at least a fifth of a texel from every edge of the projective grid (n texels across the map)."""
    r_c1, r_c2, trs = ramp_transform()

    def frac(px, py):
        w = r_c1[2] * px + r_c2[2] * py + trs[2]
        return [((r_c1[0] * px + r_c2[0] * py + trs[0]) / w * n) % 1.0, ((r_c1[1] * px + r_c2[1] * py + trs[1]) / w * n) % 1.0]

    c, s = np.cos(heading), np.sin(heading)
    for i in range(40):  # over a texel (0.2 m on the ramp) in x and in y, step (0.01 m) apart
        for j in range(40):
            px, py = x + step * i, y + step * j
            fr = frac(px + 0.5 * c, py + 0.5 * s) + frac(px - 0.5 * c, py - 0.5 * s) + frac(px, py)
            if all(0.2 < f < 0.8 for f in fr):
                return np.array([px, py, heading, roll, speed, u_y, 0.0], np.float32)
    raise AssertionError("no start pose off the texel edges")


def gentle_model(layers, seed=4, out_scale=0.25):
    """A synthetic network (params.synthetic_model) whose output layer is scaled down, so that the roll, the speed and the
    yaw rate stay well inside the thresholds over a few hundred steps; the weights are still generic dense values."""
    layers, theta = P.synthetic_model(layers, seed=seed)
    theta = theta.copy()
    n_out = layers[-2] * layers[-1] + layers[-1]
    theta[-n_out:] *= np.float32(out_scale)
    return layers, theta


IN_ROLL, IN_UX, IN_UY, IN_YAW_RATE, IN_STEER, IN_THROTTLE = range(6)   # the network's inputs: state[3 .. 6], then the controls
OUT_ROLL, OUT_UX, OUT_UY, OUT_YAW_RATE = range(4)                       # its outputs: the derivatives of state[3 .. 6]


def family(layers, bf_W):
    """Which dynamics a problem has: the basis-function model, the shipped network, or a synthetic wired one."""
    return "bf" if bf_W is not None else "shipped" if layers is None else "wired"


def wired_model(layers, wires, bias=None, seed=4, out_scale=0.25, wire_only=()):
    """gentle_model with a few wires laid through it, so that a control moves one state derivative by a chosen amount
    (the generic weights alone answer a control with millimetres over a hundred steps): wire i = (input, offset, output, gain)
    takes hidden unit i of every hidden layer -- its row is replaced by a single 1 on the input (first layer, bias -offset) or
    on unit i of the layer before (bias 0) -- and adds gain x tanh(.. tanh(input - offset)) to the output.  bias: {output:
    value added to its bias}; wire_only: outputs whose generic row and bias are zeroed first, so that only wires drive them.
    The other rows keep their generic dense values."""
    return lay_wires(*gentle_model(layers, seed=seed, out_scale=out_scale), wires, bias, wire_only)


def lay_wires(layers, theta, wires, bias=None, wire_only=()):
    """wired_model's wires through a given packed network."""
    assert len(wires) <= min(layers[1:-1])
    theta = theta.astype(np.float64)
    off = 0
    last = len(layers) - 2
    for l, (nin, nout) in enumerate(zip(layers[:-1], layers[1:])):
        W = theta[off:off + nout * nin].reshape(nout, nin)   # views: the edits land in theta
        b = theta[off + nout * nin:off + nout * nin + nout]
        if l == last:
            for out in wire_only:
                W[out, :] = 0.0
                b[out] = 0.0
        for i, (inp, offset, out, gain) in enumerate(wires):
            if l < last:
                W[i, :] = 0.0
                W[i, inp if l == 0 else i] = 1.0
                b[i] = -offset if l == 0 else 0.0
            else:
                W[out, i] += gain
        if l == last:
            for out, v in (bias or {}).items():
                b[out] += v
        off += nout * nin + nout
    return layers, theta.astype(np.float32)


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


# ------------------------------------------------------------------------------------------------------------------------
# The two branch scenes (tests/test_branch_scenes.py on the CPU, tests/test_branch_rollouts_gpu.py on the GPU): the cost's
# discontinuities FIRE here, and a rollout is held to float64 with no allowance wherever ref64 says it is DECIDED: every one of
# its margins (ref64.Ref64.trace) at least the DELTA of its class away from the discontinuity.
PATCH_TEXEL_M = 2.0      # texel edge of the patchwork map, metres: 64 x 64 texels over the ramp's bounds
PATCH_SLOP = 0.05
PATCH_LOW, PATCH_PLAIN, PATCH_HIGH = (0.005, 0.04), (0.1, 0.6), (0.7, 1.0)   # value classes: under the slop, plain, boundary
PATCH_SHARES = (0.3, 0.55, 0.15)
PATCH_MAP_SEED = 3
PATCH_STEER_GAIN = 12.0     # the steering wire of a synthetic network: yaw acceleration, rad / s^2, per tanh(.. tanh(steering))
# start poses per model family and horizon (up to 17 steps, up to 37, beyond), found by search: the stem of the fan of rollouts
# runs over texels off the boundary, the fan itself over boundary texels in part (the coverage tests of test_branch_scenes.py).
# At 17 steps the fan is 0.2 m wide and long: a boundary texel's edge cuts it during the last three steps
PATCH_START = {("shipped", 17): dict(x=8.51, y=2.37, heading=1.82), ("bf", 17): dict(x=2.89, y=9.05, heading=2.49),
               ("wired", 17): dict(x=5.56, y=0.73, heading=-1.29),
               ("shipped", 37): dict(x=-5.4, y=-13.2, heading=-2.97), ("shipped", 100): dict(x=14.9, y=-14.1, heading=2.29),
               ("bf", 37): dict(x=-5.4, y=-13.2, heading=-2.97), ("bf", 100): dict(x=15.9, y=-6.4, heading=2.62),
               ("wired", 37): dict(x=4.4, y=6.9, heading=-1.17), ("wired", 100): dict(x=-3.0, y=6.0, heading=-0.82)}
PATCH_START_2 = {("wired", 37): dict(x=-6.7, y=1.5, heading=0.7), ("wired", 100): dict(x=-4.8, y=14.2, heading=-0.57)}   # a second handle
PATCH_NEIGHBOUR_MIN = 0.03   # edge-sharing texels differ by at least this: a wrong texel moves the step's track cost by >= 3
                             # (track_coeff x 0.03 / 2), unless the slop zeroes the pair's average with either texel


def patch_horizon(T):
    """The key of PATCH_START a horizon falls under."""
    return 17 if T <= 17 else 37 if T <= 37 else 100


def patchwork_map(texel_m=PATCH_TEXEL_M, seed=PATCH_MAP_SEED):
    """Random values of three classes from a fixed seed; a texel closer than PATCH_NEIGHBOUR_MIN to its left or upper
    neighbour is drawn again."""
    n = int(round(2 * MAP_HALF / texel_m))
    rng = np.random.RandomState(seed)
    ranges = (PATCH_LOW, PATCH_PLAIN, PATCH_HIGH)

    def draw():
        lo, hi = ranges[rng.choice(3, p=PATCH_SHARES)]
        return rng.uniform(lo, hi)

    ch0 = np.zeros((n, n), np.float64)
    for j in range(n):
        for i in range(n):
            while True:
                v = draw()
                if (i == 0 or abs(v - ch0[j, i - 1]) >= PATCH_NEIGHBOUR_MIN) and (j == 0 or abs(v - ch0[j - 1, i]) >= PATCH_NEIGHBOUR_MIN):
                    break
            ch0[j, i] = v
    return S.map_rgba_from_channel0(ch0.astype(np.float32))


def check_patchwork_map(cfg):
    """The two conditions that leave the threshold compares to the texel alone: no value within 0.01 of boundary_threshold,
    no pair average (|a| + |b|) / 2 of two map values within 1e-3 of track_slop; and the neighbour rule of patchwork_map."""
    v = np.unique(np.abs(cfg["map_rgba"][:, :, 0].astype(np.float64)))
    assert np.all(np.abs(v - float(np.float32(cfg["cost"]["boundary_threshold"]))) >= 0.01)
    avg = (v[:, None] + v[None, :]) / 2.0
    assert np.all(np.abs(avg - float(np.float32(cfg["cost"]["track_slop"]))) >= 1e-3)
    m = cfg["map_rgba"][:, :, 0].astype(np.float64)
    assert np.all(np.abs(np.diff(m, axis=0)) >= PATCH_NEIGHBOUR_MIN - 1e-6) and np.all(np.abs(np.diff(m, axis=1)) >= PATCH_NEIGHBOUR_MIN - 1e-6)
    shares = [np.mean((m >= lo) & (m <= hi)) for lo, hi in (PATCH_LOW, PATCH_PLAIN, PATCH_HIGH)]
    assert abs(sum(shares) - 1.0) < 1e-12 and min(shares) > 0.1, shares


def patchwork_config(K, T, layers=None, bf_W=None, texel_m=PATCH_TEXEL_M, map_seed=PATCH_MAP_SEED, start=None, **over):
    """The TRACK branches: ramp_config (its projective transform, control-cost coefficients and stride) on a coarse random
    costmap whose texels are under the slop, plain, or on the boundary.  A wrong texel or a dropped division by w moves a
    step's cost far beyond the bar; the slop and the boundary compares are decided by the texel alone (check_patchwork_map).
    A synthetic network gets a steering wire into the yaw rate (wired_model), so that the rollouts fan out over the texels as
    those of the shipped models do."""
    theta = None
    if bf_W is None and layers is not None:
        layers, theta = wired_model(layers, [(IN_STEER, 0.0, OUT_YAW_RATE, PATCH_STEER_GAIN)])
    cfg = ramp_config(K, T, layers=layers, theta=theta, bf_W=bf_W)
    n = int(round(2 * MAP_HALF / texel_m))
    st = dict(PATCH_START[family(layers, bf_W), patch_horizon(T)], **(start or {}))
    cfg.update(map_rgba=patchwork_map(texel_m, map_seed), cost=dict(cfg["cost"], track_slop=PATCH_SLOP), track="patchwork",
               start_state=ramp_start(n=n, step=texel_m / 40.0, **st))
    cfg.update(over)
    return cfg


TILT_U_LO, TILT_U_HI = (-0.3, 0.1), (0.3, 0.6)   # both controls clamp on both sides (nu = 0.275, 0.3 about ramp_U)
TILT_SLIP = 0.25                                  # max_slip_ang
TILT_COSTS = {"l2": dict(l1_cost=False, discount=0.25), "l1": dict(l1_cost=True, discount=0.4)}   # the default discount is 0.1
TILT_ROLL_GAIN, TILT_UY_GAIN = 5.0, 10.0
TILT_ROLL_BELOW = 1.0   # the start roll under 1.57, in sigmas of the roll's random walk


# DELTA per margin class: ten times the largest margin at which ANY rollout of the fp32 oracle (modes 1 and 0) differs from
# ref64 by more than TOL64, over every case of tests/branch_cases.py (3 scenes x 13 layer lists x 3 shapes), rounded up; measured
# on the CPU by tests/measure_branch_deltas.py before any GPU run.  The factor stands for the device's tanh / sincos / atan
# against libm, as TOL64's own headroom does.
#   texel: 6.1e-6 m (27 such rollouts; patchwork, 6-32x4-4, K = 1984, T = 100, rollout 1042) -- fp32 positions within 20 m of the
#          origin carry 1e-6 m per ulp, a hundred state updates add up a few of them.  With start poses 40 m out the same
#          measurement gave 2.2e-5 m: the start poses stay within 20 m of the origin.
#   slip:  3.25e-8 rad (4 such rollouts; tilt-slide l2, 6-33-97-66-4, K = 1984, T = 100, rollout 90); an fp32 ulp of 0.25 is 3e-8
#   roll:  no oracle rollout beyond TOL64 has the roll as its nearest margin, so there is no measured figure.  From the number
#          format instead: the roll is a sum of up to 100 fp32 updates near 1.57, each rounded to half an ulp of 1.2e-7; a
#          hundred roundings of one sign would add up to 6e-6, their random sum to 6e-7: DELTA_ROLL = 1e-6, eight ulps.
# On the decided rollouts the oracle then agrees with ref64 to 1.5e-6 relative at most (the bar of the CPU tests: 2e-6).
DELTA_TEXEL, DELTA_ROLL, DELTA_SLIP = 7e-5, 1e-6, 5e-7   # metres, radians, radians
UNDECIDED_CAP = 0.10     # of K
# The edge scenes (tests/edge_cases.py: 4 scenes x 13 layer lists x their shapes and parts, 629 888 rollouts x 2 modes), by the
# same rule, measured by `python -m tests.measure_branch_deltas edge` before any GPU run:
#   texel, border: 1.19e-5 m (127 such rollouts; border/ne, 6-5-7-4, K = 1984, T = 100, mode 1, rollout 1188) -- twice the
#          patchwork's figure: the poses wind the heading up to -11.8 rad, where an fp32 ulp is 9.5e-7 rad, and reach 25 m from
#          the origin.  DELTA_TEXEL_BORDER = 1.2e-4 m; the cap scene (the patchwork itself: 3.57e-6 m, 4 rollouts) keeps DELTA_TEXEL.
#   ux, bf, slip on the crawl, cap: no oracle rollout beyond TOL64 has one of them as its nearest margin (crawl: 75 776 rollouts
#          x 2 modes, none beyond TOL64 at all), so from the number format:
#          DELTA_UX = 5e-6 m/s, for | |u_x| - 0.001 | and | u_x - 0.1 |: u_x is a sum of up to 100 fp32 updates of magnitude up to
#          0.25 (half an ulp of 3e-8 each: 1.5e-6 if all of one sign) of dt x (wire gain 5) x tanh, and the device's tanh is
#          within 2e-7 of libm's: 0.02 x 5 x 2e-7 = 2e-8 per step, 2e-6 over 100 steps.  Beside that a few ulps of 0.001 itself
#          (1.2e-10) are nothing: the distance to the switch is lost in u_x, not in the compare.
#          DELTA_SLIP_CRAWL = 1e-3 rad: where the slip angle atan(u_y / |u_x|) crosses max_slip_ang = 0.9 with u_y = 0.004,
#          |u_x| = 0.0032 and d slip / d u_x = u_y / (u_x^2 + u_y^2) = 154 rad per m/s: DELTA_UX of u_x is 7.7e-4 rad.
#          DELTA_CAP = 1e-5 relative: a step cost is a sum of five fp32 terms, within three ulps (2e-7) of its float64 value;
#          TOL64 itself, fifty times that.
DELTA_TEXEL_BORDER, DELTA_UX, DELTA_SLIP_CRAWL, DELTA_CAP = 1.2e-4, 5e-6, 1e-3, 1e-5   # metres, metres per second, radians, relative


def decided(cfg, tr):
    """[K] bool: the rollouts of a ref64 trace (ref64.Ref64.trace) whose every margin is at least the DELTA of its class, over
    the steps that enter the cost.  The texel class counts on the patchwork only (on the ramp a wrong texel moves a cost by
    less than RAMP_FLIP_BOUND); the roll class up to the first update after which |roll| exceeds 1.57 by DELTA_ROLL or more:
    the flag is sticky, no later roll reaches a cost."""
    T = int(cfg["T"])
    if T <= 1:
        return np.ones(int(cfg["K"]), bool)
    with np.errstate(invalid="ignore"):
        ok = tr["m_slip"][:, 1:T].min(axis=1) >= (DELTA_SLIP_CRAWL if cfg["track"] == "crawl" else DELTA_SLIP)
        if cfg["track"] in ("patchwork", "border"):
            ok &= tr["m_texel"][:, 1:T].min(axis=1) >= (DELTA_TEXEL_BORDER if cfg["track"] == "border" else DELTA_TEXEL)
        # the edge scenes' classes; on every other scene u_x > 1 and the costs are under 1e6: nothing changes there
        ok &= tr["m_ux"][:, 1:T].min(axis=1) >= DELTA_UX
        ok &= tr["m_bf"][:, :T - 1].min(axis=1) >= DELTA_UX   # the dynamics of the steps 0 .. T-2 reach a cost
        ok &= tr["m_cap"][:, 1:T].min(axis=1) >= DELTA_CAP
    m, over = tr["m_roll"][:, 1:T], tr["roll_over"][:, 1:T]    # after the updates 0 .. T-2: what the costs of 1 .. T-1 see
    sure = over & (m >= DELTA_ROLL)
    open_yet = np.cumsum(sure, axis=1) - sure == 0             # no decisive firing before this update
    ok &= np.where(open_yet, m, np.inf).min(axis=1) >= DELTA_ROLL
    return ok


def tilt_slide_config(K, T, layers=None, bf_W=None, variant="l2", roll_below=None, **over):
    """The STATE branches on the ramp map (the track stays flip-free): the start roll sits a little under 1.57 and the model's
    roll rate follows the steering, so that part of the rollouts tip over -- the sticky flag getCrash sets after the state
    update; the start lateral velocity puts the slip angle a little under max_slip_ang = TILT_SLIP and the lateral
    acceleration follows the throttle, so that |slip| goes over the limit and comes back (not sticky).  variant: the key of
    TILT_COSTS (speed cost l2 / l1, two discounts); roll_below: the start roll under 1.57 in sigmas of the roll's random walk,
    if not TILT_ROLL_BELOW (2.9: one or two rollouts in a hundred tip over)."""
    theta = None
    speed = 6.0
    sigma = 0.004 * np.sqrt(T)   # dt x the clamped steering noise through the wire (about 0.2), summed over T steps
    wires = [(IN_STEER, 0.0, OUT_ROLL, TILT_ROLL_GAIN), (IN_THROTTLE, 0.35, OUT_UY, TILT_UY_GAIN)]   # ramp_U's throttle: about 0.35
    if bf_W is not None:
        # the shipped weights at 3 % of their strength: a roll of 1.5 and a slide of 1.5 m/s are far outside what they were
        # fitted on (at a tenth the yaw rate still runs away within 100 steps); roll and u_y are driven by their wires alone
        bf_W = np.array(bf_W, np.float32).reshape(4, 25).copy() * np.float32(0.03)
        bf_W[OUT_UY, :] = 0.0
        bf_W[OUT_ROLL, :] = 0.0
        bf_W[OUT_ROLL, 8] += TILT_ROLL_GAIN    # basis function 8: sin(steering)
        bf_W[OUT_UY, 0] += TILT_UY_GAIN        # basis function 0: the throttle, less its 0.35 through function 1, u_x / 10
        bf_W[OUT_UY, 1] -= TILT_UY_GAIN * 0.35 / (0.1 * speed)
    elif layers is None:   # the shipped hidden layers, the output layer a tenth as strong (as above), and the wires
        layers, theta = S.default_model()
        theta = theta.copy()
        n_out = layers[-2] * layers[-1] + layers[-1]
        theta[-n_out:] *= np.float32(0.1)
        layers, theta = lay_wires(layers, theta, wires, wire_only=(OUT_ROLL, OUT_UY))
    else:
        layers, theta = wired_model(layers, wires, wire_only=(OUT_ROLL, OUT_UY))
    cfg = ramp_config(K, T, layers=layers, theta=theta, bf_W=bf_W)
    cfg.update(cost=dict(cfg["cost"], max_slip_ang=TILT_SLIP, **TILT_COSTS[variant]), track="tilt_slide", u_lo=TILT_U_LO, u_hi=TILT_U_HI,
               start_state=ramp_start(speed=speed, roll=1.57 - TILT_ROLL_GAIN * (roll_below or TILT_ROLL_BELOW) * sigma,
                                      u_y=speed * np.tan(TILT_SLIP - 0.005)))
    cfg.update(over)
    return cfg


# ------------------------------------------------------------------------------------------------------------------------
# The four edge scenes (tests/edge_cases.py; tests/test_edge_scenes.py on the CPU, tests/test_edge_rollouts_gpu.py on the GPU):
# what lies outside the box the scenes above keep the state in -- car points off the map (the border clamp of the lookup), a
# speed under 0.001 m/s and a negative one (the guard of the stabilizing cost, |u_x| in the slip angle, the basis functions'
# u_x > .1), a step cost at the 1e12 cap, hidden units far in tanh's saturation and headings in negative and high quadrants.
BORDER_W, BORDER_H = 20, 12      # texels of PATCH_TEXEL_M: x in [-20, 20], y in [-12, 12]; not square, so that a clamp with the
BORDER_MAP_SEED = 4              # two sizes swapped reads another texel
# start poses per border, model family and horizon: `d` metres inside the border (the corner poses: inside both), `along`
# metres along it from its middle, the heading `turn` radians off the outward normal plus `wind` whole turns.  The turns put
# sincos_fast's quadrant number at 4, -2, -3, -1, -7 and 3: on the ramp a wrong quadrant moves a cost by less than the bar, on
# 2 m texels that differ by 0.03 or more it does not.  Found by search (python -m tests.measure_branch_deltas --poses): the fan
# of rollouts leaves the map in part, and at T = 100 part of what left comes back.
BORDER_NORMAL = {"e": 0.0, "w": np.pi, "n": np.pi / 2, "s": -np.pi / 2, "ne": np.pi / 4, "sw": -3 * np.pi / 4}
BORDER_WIND = {"e": 1, "w": -1, "n": -1, "s": 0, "ne": -2, "sw": 1}
BORDER_POSES = list(BORDER_NORMAL)


BORDER_START = {
    ("shipped", 17, "e"): dict(d=1.6, turn=0.7), ("shipped", 17, "w"): dict(d=1.9, turn=0.7),
    ("shipped", 17, "n"): dict(d=2.02, turn=0.7), ("shipped", 17, "s"): dict(d=1.92, turn=0.7),
    ("shipped", 17, "ne"): dict(d=1.6, turn=0.0), ("shipped", 17, "sw"): dict(d=1.75, turn=0.0),
    ("shipped", 37, "e"): dict(d=3.39, turn=0.8), ("shipped", 37, "w"): dict(d=3.7, turn=0.8),
    ("shipped", 37, "n"): dict(d=3.81, turn=0.8), ("shipped", 37, "s"): dict(d=3.7, turn=0.8),
    ("shipped", 37, "ne"): dict(d=3.44, turn=0.0), ("shipped", 37, "sw"): dict(d=3.56, turn=0.0),
    ("shipped", 100, "e"): dict(d=1.88, along=-6., turn=1.1, steer=-0.25), ("shipped", 100, "w"): dict(d=2.32, along=-6., turn=1.1, steer=-0.25),
    ("shipped", 100, "n"): dict(d=2.32, along=-6., turn=1.1, steer=-0.25), ("shipped", 100, "s"): dict(d=2.17, along=-6., turn=1.1, steer=-0.25),
    ("shipped", 100, "ne"): dict(d=9.61, turn=0.0), ("shipped", 100, "sw"): dict(d=9.76, turn=0.0),
    ("bf", 17, "e"): dict(d=1.61, turn=0.7), ("bf", 17, "w"): dict(d=1.92, turn=0.7),
    ("bf", 17, "n"): dict(d=2.02, turn=0.7), ("bf", 17, "s"): dict(d=1.92, turn=0.7),
    ("bf", 17, "ne"): dict(d=1.61, turn=0.0), ("bf", 17, "sw"): dict(d=1.77, turn=0.0),
    ("bf", 37, "e"): dict(d=3.49, turn=0.8), ("bf", 37, "w"): dict(d=3.81, turn=0.8),
    ("bf", 37, "n"): dict(d=3.91, turn=0.8), ("bf", 37, "s"): dict(d=3.81, turn=0.8),
    ("bf", 37, "ne"): dict(d=3.43, turn=0.0), ("bf", 37, "sw"): dict(d=3.54, turn=0.0),
    ("bf", 100, "e"): dict(d=0.58, along=6., turn=-1.4), ("bf", 100, "w"): dict(d=0.87, along=6., turn=-1.4),
    ("bf", 100, "n"): dict(d=0.97, along=6., turn=-1.4), ("bf", 100, "s"): dict(d=0.87, along=6., turn=-1.4),
    ("bf", 100, "ne"): dict(d=6.53, turn=0.0), ("bf", 100, "sw"): dict(d=6.68, turn=0.0),
    ("wired", 17, "e"): dict(d=1.55, turn=0.7), ("wired", 17, "w"): dict(d=1.86, turn=0.7),
    ("wired", 17, "n"): dict(d=1.96, turn=0.7), ("wired", 17, "s"): dict(d=1.86, turn=0.7),
    ("wired", 17, "ne"): dict(d=1.55, turn=0.0), ("wired", 17, "sw"): dict(d=1.69, turn=0.0),
    ("wired", 37, "e"): dict(d=3.28, turn=0.8), ("wired", 37, "w"): dict(d=3.49, turn=0.8),
    ("wired", 37, "n"): dict(d=3.7, turn=0.8), ("wired", 37, "s"): dict(d=3.49, turn=0.8),
    ("wired", 37, "ne"): dict(d=3.05, turn=0.0), ("wired", 37, "sw"): dict(d=3.16, turn=0.0),
    ("wired", 100, "e"): dict(d=5.28, along=-6., turn=1.1, steer=0.25), ("wired", 100, "w"): dict(d=5.87, along=-6., turn=1.1, steer=0.25),
    ("wired", 100, "n"): dict(d=5.87, along=-6., turn=1.1, steer=0.25), ("wired", 100, "s"): dict(d=5.87, along=-6., turn=1.1, steer=0.25),
    ("wired", 100, "ne"): dict(d=6.62, turn=0.0), ("wired", 100, "sw"): dict(d=6.75, turn=0.0),
}


def border_map(seed=BORDER_MAP_SEED):
    """patchwork_map's rule on BORDER_W x BORDER_H texels: three value classes, a texel closer than PATCH_NEIGHBOUR_MIN to its
    left or upper neighbour is drawn again -- so every border row and column differs from texel to texel, and a value read from
    outside the map says which border texel the clamp went to."""
    rng = np.random.RandomState(seed)
    ranges = (PATCH_LOW, PATCH_PLAIN, PATCH_HIGH)
    ch0 = np.zeros((BORDER_H, BORDER_W), np.float64)
    for j in range(BORDER_H):
        for i in range(BORDER_W):
            while True:
                lo, hi = ranges[rng.choice(3, p=PATCH_SHARES)]
                v = rng.uniform(lo, hi)
                if (i == 0 or abs(v - ch0[j, i - 1]) >= PATCH_NEIGHBOUR_MIN) and (j == 0 or abs(v - ch0[j - 1, i]) >= PATCH_NEIGHBOUR_MIN):
                    break
            ch0[j, i] = v
    return S.map_rgba_from_channel0(ch0.astype(np.float32))


def border_transform():
    hx, hy = BORDER_W * PATCH_TEXEL_M / 2.0, BORDER_H * PATCH_TEXEL_M / 2.0
    r_c1, r_c2, trs = P.costmap_transform(-hx, hx, -hy, hy)
    r_c1, r_c2 = r_c1.copy(), r_c2.copy()
    r_c1[2], r_c2[2] = np.float32(PROJ[0]), np.float32(PROJ[1])
    return r_c1, r_c2, trs


def border_pose(border, d, turn, along=0.0, steer=0.0):
    """(x, y, heading) of a start pose given relative to a border or a corner of the border map."""
    hx, hy = BORDER_W * PATCH_TEXEL_M / 2.0, BORDER_H * PATCH_TEXEL_M / 2.0
    # `along` runs the way a positive `turn` heads: the outward normal turned left
    x, y = {"e": (hx - d, along), "w": (-hx + d, -along), "n": (-along, hy - d), "s": (along, -hy + d),
            "ne": (hx - d - along, hy - d + along), "sw": (-hx + d + along, -hy + d - along)}[border]
    return x, y, BORDER_NORMAL[border] + turn + 2.0 * np.pi * BORDER_WIND[border]


def border_config(K, T, border, layers=None, bf_W=None, start=None, **over):
    """OFF THE MAP: patchwork_config's problem on the small border map, started near one border or corner."""
    theta = None
    if bf_W is None and layers is not None:
        layers, theta = wired_model(layers, [(IN_STEER, 0.0, OUT_YAW_RATE, PATCH_STEER_GAIN)])
    cfg = ramp_config(K, T, layers=layers, theta=theta, bf_W=bf_W)
    r_c1, r_c2, trs = border_transform()
    cfg.update(map_rgba=border_map(), r_c1=r_c1, r_c2=r_c2, trs=trs, cost=dict(cfg["cost"], track_slop=PATCH_SLOP), track="border",
               border=border)
    st = start or BORDER_START[family(layers, bf_W), patch_horizon(T), border]
    cfg["steer_bias"] = float(st.get("steer", 0.0))
    x, y, heading = border_pose(border, **st)   # taken as it is: a point near a texel edge makes its rollout undecided, no more
    cfg["start_state"] = np.array([x, y, heading, 0.0, 6.0, 0.0, 0.0], np.float32)
    cfg.update(over)
    return cfg


CRAWL_SPEEDS = (0.03, 0.0, -0.05)   # start u_x, m/s; the basis-function case starts at CRAWL_BF_SPEED instead
CRAWL_BF_SPEED = 0.13
CRAWL_UY = 0.004                    # start u_y: the slip angle atan(u_y / |u_x|) goes through max_slip_ang at |u_x| = 0.0032
CRAWL_SLIP = 0.9
CRAWL_WIRE = (IN_THROTTLE, 0.35, OUT_UX, 5.0)
CRAWL_BF_GAIN = 5.0


def crawl_config(K, T, speed, layers=None, bf_W=None, **over):
    """AT A CRAWL, on the ramp map: u_x starts at `speed` and follows the throttle through a wire (the generic row of the
    output is zeroed), so that it passes under 0.001 m/s and through 0 both ways; with u_y a few mm/s the slip angle swings
    between nothing and pi / 2 and crosses max_slip_ang both ways.  The basis-function model at 3 % of its strength (as the
    tilt-slide) with u_x driven by the throttle function alone: u_x goes through .1 both ways."""
    theta = None
    if bf_W is not None:
        bf_W = np.array(bf_W, np.float32).reshape(4, 25).copy() * np.float32(0.03)
        bf_W[OUT_UX, :] = 0.0
        bf_W[OUT_UX, 0] = CRAWL_BF_GAIN   # basis function 0, the throttle itself (its nominal value is about -0.1: crawl_U)
    elif layers is None:
        layers, theta = S.default_model()
        theta = theta.copy()
        n_out = layers[-2] * layers[-1] + layers[-1]
        theta[-n_out:] *= np.float32(0.1)
        layers, theta = lay_wires(layers, theta, [CRAWL_WIRE], wire_only=(OUT_UX,))
    else:
        layers, theta = wired_model(layers, [CRAWL_WIRE], wire_only=(OUT_UX,))
    cfg = ramp_config(K, T, layers=layers, theta=theta, bf_W=bf_W)
    cfg.update(cost=dict(cfg["cost"], max_slip_ang=CRAWL_SLIP), track="crawl", start_state=ramp_start(speed=speed, u_y=CRAWL_UY))
    cfg.update(over)
    return cfg


def border_U(cfg, seed=7):
    """ramp_U with the pose's steering bias (`steer` of BORDER_START): at T = 100 the network models answer ramp_U's steering
    with too little yaw to bring a car that left the map back onto it; with a steady turn towards the map part of the fan does."""
    U = ramp_U(cfg, seed)
    U[:, 0] += np.float32(cfg.get("steer_bias", 0.0))
    return U


def crawl_U(cfg, seed=7):
    """ramp_U; for the basis-function model the throttle about -0.1 (no basis function is a constant to offset it with)."""
    U = ramp_U(cfg, seed)
    if cfg.get("bf_W") is not None:
        U[:, 1] -= np.float32(0.45)
    return U


CAP_SETTINGS = ("over", "under", "on")
CAP_UNDER = 0.99e12   # the discounted crash cost of the "under" setting


def cap_config(K, T, setting, layers=None, bf_W=None, **over):
    """AT THE CAP: the patchwork with its start poses and a crash_coeff that puts a crashed step's cost
      "over":  above 1e12 (crash_coeff 2e12): every step after the crash is replaced by (float)1e12;
      "under": at CAP_UNDER + the other terms, just under 1e12: not replaced;
      "on":    "over", started ON a boundary texel: every costed step of every rollout is capped.
    The stabilizing cost adds crash_coeff too where the slip limit is crossed; max_slip_ang stays at the ramp's 1.6, out of reach."""
    cfg = patchwork_config(K, T, layers=layers, bf_W=bf_W)
    disc = float(np.float32(cfg["cost"]["discount"]))
    coeff = 2e12 if setting != "under" else CAP_UNDER / (1.0 - disc)
    cfg["cost"] = dict(cfg["cost"], crash_coeff=coeff)
    cfg["cap"] = setting
    if setting == "on":
        m = cfg["map_rgba"][:, :, 0]
        n = m.shape[0]
        j, i = [(j, i) for j in range(n // 2, n) for i in range(n // 2, n) if m[j, i] >= PATCH_HIGH[0]][0]
        cfg["start_state"] = ramp_start(x=-MAP_HALF + PATCH_TEXEL_M * i + 0.8, y=-MAP_HALF + PATCH_TEXEL_M * j + 0.8, heading=0.0,
                                        n=n, step=0.01)
    cfg.update(over)
    return cfg


STIFF_HEADINGS = (-2.2, -3.0, 4.0, 6283.6)   # sincos_fast's quadrant numbers -1, -2, 3 and 4000
STIFF_FAR = 6283.6     # held to the fp32 oracle only: ref64 keeps the heading in float64, an fp32 ulp there is 4.9e-4 rad
STIFF_GAINS = (250.0, -400.0, 600.0)   # the steering coefficient of the scaled-up rows of hidden units 0, 1, 2
STIFF_SPAN = 200.0


def stiff_model(layers, theta, x0):
    """The first-layer rows of the hidden units 0 .. 2 scaled up until their steering coefficient is STIFF_GAINS, the bias set
    so that the pre-activation passes through 0 at the network input x0 (+- 0.5, 1 and 1.5): over steerings of +- 0.99 the
    pre-activations span more than +- STIFF_SPAN -- exp2 of +- 600 x 2.885 is inf and 0 in tanh_bias -- and pass through (-2, 2)."""
    theta = np.asarray(theta, np.float64).copy()
    nin, nout = layers[0], layers[1]
    W = theta[:nout * nin].reshape(nout, nin)
    b = theta[nout * nin:nout * nin + nout]
    for i, g in enumerate(STIFF_GAINS[:min(3, nout)]):
        W[i, :] *= g / W[i, IN_STEER]
        b[i] = -float(W[i, :] @ x0) + 0.5 * (i + 1)
    return list(layers), theta.astype(np.float32)


def stiff_config(K, T, heading, layers=None, bf_W=None, **over):
    """STIFF, on the ramp (flip-free: asserted by tests/test_edge_scenes.py as tests/test_ref64.py does for the ramp): hidden
    units deep in tanh's saturation on both sides, and start headings in negative and high quadrants.  The basis-function
    model has no hidden units: its case is the headings alone."""
    theta = None
    if bf_W is None:
        if layers is None:   # the shipped hidden layers, the output layer a tenth as strong (as the tilt-slide's): at full strength
            layers, theta = S.default_model()   # a unit with a gain of 600 turns an ulp of the steering into 1e-5 of a cost
            theta = theta.copy()
            theta[-(layers[-2] * layers[-1] + layers[-1]):] *= np.float32(0.1)
        else:
            layers, theta = gentle_model(layers)
        x0 = np.array([0.0, 6.0, 0.0, 0.0, 0.0, 0.35])
        layers, theta = stiff_model(layers, theta, x0)
    cfg = ramp_config(K, T, layers=layers, theta=theta, bf_W=bf_W)
    # the ramp's texels are exercised, not verified: the pose need not keep off their edges (at 4.0 rad no pose does)
    cfg.update(track="stiff", start_state=np.array([1.0, -2.0, heading, 0.0, 6.0, 0.0, 0.0], np.float32))
    cfg.update(over)
    return cfg
