"""The mixed fleet of the batched nominal replay (mppi_nominal_traj_batch -> csrc/nominal_fleet.hip): its problem list and a float64
replay.  A helper, not a test: tests/test_nominal_fleet_cpu.py holds the problems to a condition (the fp32 replay stays within
1e-5 of float64, clamping fires), tests/test_nominal_fleet_gpu.py runs them on the device.

A problem is drawn as tests/test_ddp_fleet_gpu.py::_problem draws (start state, model), except that the control sequence is scaled
PAST the limits, so that the clamp fires at both ends."""
import functools

import numpy as np

from autorally_amd import params as P
from autorally_amd import synthetic as S
from tests.helpers import warm_U
from tests.ref64 import Ref64

# layers, T, hz, negate_yaw_der, tightened limits: every layer-list seam of the kernel (one to four neuron chains per lane, ragged
# k ends, widths of 64 | 65, 128 | 129, 256; an image in LDS and one in global memory), every T of the issue, the three rates
FLEET = [
    ([6, 4], 2, 20, True, False),
    ([6, 24, 4], 3, 50, False, True),
    ([6, 5, 7, 4], 5, 100, True, False),
    ([6, 32, 32, 4], 17, 50, True, True),
    ([6, 64, 64, 4], 40, 20, False, False),
    ([6, 65, 4], 33, 100, True, False),
    ([6, 8, 8, 8, 8, 8, 4], 40, 50, False, True),
    ([6, 128, 129, 4], 5, 20, True, False),
    ([6, 200, 256, 4], 17, 100, False, True),
    ([6, 256, 256, 256, 4], 3, 50, True, False),
    ([6, 64, 64, 64, 64, 4], 100, 50, True, False),
    ([6, 32, 32, 4], 250, 100, False, True),
]
TIGHT = dict(u_lo=(-0.6, -0.3), u_hi=(0.7, 0.4))


def tag(i):
    return "%d %s T=%d" % (i, "-".join(map(str, FLEET[i][0])), FLEET[i][1])


def scaled_U(cfg, rng, seed):
    """warm_U's smooth sequence scaled past the limits: steering swings to 1.1 .. 1.8 of its limits, throttle about 0.1 with an
    amplitude past both of its limits."""
    w = warm_U(cfg, seed=seed).astype(np.float64)
    hi = np.asarray(cfg["u_hi"], np.float64)
    U = np.empty_like(w)
    U[:, 0] = w[:, 0] / 0.05 * hi[0] * rng.uniform(1.1, 1.8)
    U[:, 1] = 0.1 + (w[:, 1] - 0.3) / 0.05 * rng.uniform(1.2, 1.6)
    return U.astype(np.float32)


def make_problem(i, layers, T, hz, negate, tight, base_map, flat=False):
    """Problem number i (the seed of its draws).  flat: the network's output neuron 3 (the yaw-rate derivative) has zero weights and
    bias and the start state has psi = 0 and s6 = 0, so that the heading stays exactly 0 (sin / cos cannot differ between host
    and device)."""
    rng = np.random.RandomState(8000 + i)
    over = dict(negate_yaw_der=negate, hz=hz)
    if tight:
        over.update(TIGHT)
    l, th = P.synthetic_model(list(layers), seed=int(rng.randint(100)))
    th = np.array(th, np.float32)
    if flat:
        nin, nout = l[-2], l[-1]
        last = th.size - (nin * nout + nout)
        th[last + 3 * nin:last + 4 * nin] = 0.0
        th[last + nin * nout + 3] = 0.0
    cfg = dict(base_map, K=64, T=T, layers=l, theta=th, **over)
    x0 = np.array(cfg["start_state"], np.float32).copy()
    x0[4], x0[5], x0[6] = rng.uniform(0.05, 12), rng.uniform(-1, 1), rng.uniform(-1.5, 1.5)
    x0[3], x0[2] = rng.uniform(-0.2, 0.2), rng.uniform(-3, 3)
    if flat:
        x0[2] = x0[6] = 0.0
    if T >= 100:
        # every step rounds the position to its ulp (1e-6 at 10 m), and 100 .. 250 steps of that alone come near the 1e-5 the CPU
        # test holds the inputs to: the long instances start at the origin (the replay reads no map) and drive slowly
        x0[0] = x0[1] = 0.0
        x0[4] = np.float32(0.3 * x0[4])
    return dict(cfg=cfg, x0=x0, U=scaled_U(cfg, rng, i))


@functools.lru_cache(maxsize=None)
def base_map():
    return S.make_config(64, 5, track="oval")


@functools.lru_cache(maxsize=None)
def problems():
    """The mixed fleet's problems (computed once, not changed)."""
    return tuple(make_problem(i, *FLEET[i], base_map()) for i in range(len(FLEET)))


def replay64(cfg, x0, U):
    """mppi_nominal_traj in float64 on tests/ref64.Ref64.state_deriv: (state_seq [T][7], control_seq [T][2]).  The inputs are the
    fp32 values read as doubles; nothing after that is rounded."""
    r = Ref64(cfg)
    s = np.asarray(x0, np.float32).astype(np.float64)[None, :]
    U = np.asarray(U, np.float32).astype(np.float64)
    xs, us = np.zeros((r.T, 7)), np.zeros((r.T, 2))
    for t in range(r.T):
        xs[t] = s[0]
        u = np.where(U[t] < r.u_lo, r.u_lo, np.where(U[t] > r.u_hi, r.u_hi, U[t]))
        us[t] = u
        s = s + r.state_deriv(s, u[None, :]) * r.dt
    return xs, us
