"""The drive law of mppi_plant_drive_batch (csrc/plant_drive_fleet.hip, plant_drive_host of csrc/abi_host.hip): its problems and a
float64 restatement.  A helper, not a test: tests/test_plant_drive_cpu.py holds the problems to a condition (the host text stays
within 1e-5 of float64) and proves that the clamp and the feedback fire, tests/test_plant_drive_gpu.py runs them on the device.

The controller is 6-32-32-4 with T = 17 at 50 Hz (the closed-loop suite's shape).  A problem is one controller of a fleet: its start
state, its control sequence (scaled past the limits, as tests/nominal_cases.py scales it) and its PLANT -- None (the controller's own
network), another layer list, or the controller's weights scaled by 1.05.  A call is (periods, substeps, feedback) for the whole fleet."""
import functools

import numpy as np

from autorally_amd import params as P
from autorally_amd import synthetic as S
from tests import nominal_cases as NC
from tests.ref64 import Ref64

NET, T, HZ = [6, 32, 32, 4], 17, 50
# the plant of every handle of the fleet: (layers or "own" or "scaled", the plant's negate_yaw_der or None for the controller's) and the
# controller's negate_yaw_der -- an image in LDS (6-64x4-4) and one in global memory (6-200-256-4), a ragged k end (65), both signs
FLEET = [
    ("own", None, True),
    ([6, 24, 4], False, True),
    ([6, 65, 4], True, False),
    ([6, 64, 64, 64, 64, 4], False, False),
    ([6, 200, 256, 4], True, True),
    ("scaled", None, False),
]
# the DDP weights of every controller: initDDP's Q a hundredfold and R = 0.1 instead of 10 -- with the defaults the gains over 17 steps
# are of order 1e-4 and no correction would be visible
DDP_Q, DDP_R, DDP_QF = (50.0, 50.0, 25.0, 0.0, 5.0, 1.0, 1.0), (0.1, 0.1), (0.0,) * 7
# (periods, substeps, feedback): substeps 1, 3 and 4, strides 1 and 2 (and 3: more than one period behind an interpolated one)
CALLS =[(1, 1, False), (2, 1, True), (2, 3, True), (1, 4, False), (2, 4, True), (3, 3, False)]


def tag(i):
    kind = FLEET[i][0]
    return "%d plant %s" % (i, kind if isinstance(kind, str) else "-".join(map(str, kind)))


@functools.lru_cache(maxsize=None)
def base_map():
    return S.make_config(64, T, track="oval")


def make_problem(i, kind, plant_negate, negate, flat=False):
    """Problem i.  flat: the PLANT's output neuron 3 is zeroed and the start state has psi = s6 = 0: the heading stays exactly 0."""
    rng = np.random.RandomState(9100 + i)
    l, th = P.synthetic_model(list(NET), seed=int(rng.randint(100)))
    th = np.array(th, np.float32)
    cfg = dict(base_map(), K=64, T=T, layers=l, theta=th, negate_yaw_der=negate, hz=HZ, **NC.TIGHT)
    if kind == "own":
        pl, pth, pneg = l, th.copy(), negate
    elif kind == "scaled":
        pl, pth, pneg = l, (th * np.float32(1.05)).astype(np.float32), negate
    else:
        pl, pth = P.synthetic_model(list(kind), seed=int(rng.randint(100)))
        pth, pneg = np.array(pth, np.float32), plant_negate
    if flat:
        nin, nout = pl[-2], pl[-1]
        last = pth.size - (nin * nout + nout)
        pth[last + 3 * nin:last + 4 * nin] = 0.0
        pth[last + nin * nout + 3] = 0.0
        if kind == "own":   # the plant IS the controller's network: the handle holds the zeroed weights
            cfg = dict(cfg, theta=pth)
    x0 =np.array(cfg["start_state"], np.float32).copy()
    x0[4], x0[5], x0[6] = rng.uniform(0.5, 8), rng.uniform(-1, 1), rng.uniform(-1.5, 1.5)
    x0[3], x0[2] = rng.uniform(-0.2, 0.2), rng.uniform(-3, 3)
    if flat:
        x0[2] = x0[6] = 0.0
    # the plant starts beside the nominal trajectory's first row: the feedback has something to correct
    off = np.array([0.05, -0.04, 0.0 if flat else 0.02, 0.01, 0.15, -0.05, 0.0 if flat else 0.03], np.float32)
    return dict(cfg=cfg, x0=x0, x_plant=(x0 + off).astype(np.float32), U=NC.scaled_U(cfg, rng, i),
                plant=None if kind == "own" else dict(layers=list(pl), theta=pth, negate=bool(pneg)),
                plant_cfg=dict(cfg, layers=list(pl), theta=pth, negate_yaw_der=bool(pneg)))


@functools.lru_cache(maxsize=None)
def problems(flat=False):
    """The fleet's problems (computed once, not changed)."""
    return tuple(make_problem(i + (50 if flat else 0), *FLEET[i], flat=flat) for i in range(len(FLEET)))


def drive64(plant_cfg, u_lo, u_hi, x, xs, us, K, periods, substeps):
    """The law in float64 on tests/ref64.Ref64.state_deriv -> (state_out [7], applied [periods * substeps][2], facts).  The inputs are
    the fp32 values read as doubles (dt_sub is the law's ONE fp32 division); nothing after that is rounded.  facts: what the law met
    on the way -- the largest |du| added, whether the clamp changed a control, whether a NaN correction fell back to feed-forward."""
    r = Ref64(plant_cfg)
    m = int(substeps)
    dt_sub = float(np.float32(np.float32(1.0 / int(plant_cfg["hz"])) / np.float32(m)))
    lo_, hi_ = np.asarray(u_lo, np.float32).astype(np.float64), np.asarray(u_hi, np.float32).astype(np.float64)
    s = np.asarray(x, np.float32).astype(np.float64)
    us = np.asarray(us, np.float32).astype(np.float64)
    xs = np.asarray(xs, np.float32).astype(np.float64) if xs is not None else None
    K = np.asarray(K, np.float32).astype(np.float64) if K is not None else None
    applied = np.zeros((periods * m, 2))
    facts = dict(max_du=0.0, clamped=False, nan_fallback=False)
    with np.errstate(invalid="ignore"):
        for q in range(periods * m):
            lo, j = q // m, q % m
            if j == 0:
                u = us[lo].copy()
                xd, k = (xs[lo], K[lo]) if K is not None else (None, None)
            else:
                a = float(j) / float(m)
                u = (1 - a) * us[lo] + a * us[lo + 1]
                if K is not None:
                    xd, k = (1 - a) * xs[lo] + a * xs[lo + 1], (1 - a) * K[lo] + a * K[lo + 1]
            if K is not None:
                du = k @ (s - xd)
                if not np.any(np.isnan(du)):
                    u = u + du
                    facts["max_du"] = max(facts["max_du"], float(np.max(np.abs(du))))
                else:
                    facts["nan_fallback"] = True
            ap = np.where(u < lo_, lo_, np.where(u > hi_, hi_, u))
            facts["clamped"] = facts["clamped"] or bool(np.any(ap != u))
            applied[q] = ap
            s = s + r.state_deriv(s[None, :], ap[None, :])[0] * dt_sub
    return s, applied, facts
