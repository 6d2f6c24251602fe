"""The mixed fleet of the fused closing stages (mppi_nominal_and_gains_batch -> csrc/nominal_gains_fleet.hip): the problems of
tests/nominal_cases.py -- every layer-list seam, every T, three rates, both negate_yaw_der settings, tightened limits, controls
scaled past the limits -- with DDP weights drawn as tests/test_ddp_fleet_gpu.py::_problem draws them (zeros in Q, Qf on and off),
and the oracle's results.  A helper, not a test: tests/test_nominal_gains_fleet_cpu.py holds the problems to their conditions,
tests/test_nominal_gains_fleet_gpu.py runs them on the device."""
import functools

import numpy as np

from oracle import oracle as O
from tests import nominal_cases as NC


def weights(i):
    """DDP weights of instance i: a zero entry in Q in every instance (and more by chance), Qf on in the even instances."""
    rng = np.random.RandomState(9000 + i)
    Q = (rng.uniform(0, 1, 7) * (rng.rand(7) < 0.8)).astype(np.float32)
    Q[(i + 3) % 7] = 0.0
    R = rng.uniform(0.5, 20, 2).astype(np.float32)
    Qf = (rng.uniform(0, 2, 7) * (1.0 if i % 2 == 0 else 0.0)).astype(np.float32)
    return Q, R, Qf


@functools.lru_cache(maxsize=None)
def problems():
    """NC.problems() with Q, R, Qf added (computed once, not changed)."""
    out = []
    for i, p in enumerate(NC.problems()):
        Q, R, Qf = weights(i)
        out.append(dict(p, Q=Q, R=R, Qf=Qf))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def oracle_results():
    """Per problem: the oracle's nominal trajectory (state_seq, control_seq) and its DDP pass tracking that trajectory (computed once,
    not changed).  A factorisation that fails raises."""
    out = []
    for p in problems():
        orc = O.Oracle(p["cfg"])
        xs, us = orc.nominal_traj(p["x0"], p["U"])
        out.append((xs, us, orc.ddp_feedback_gains(p["x0"], xs, us, p["Q"], p["R"], p["Qf"])))
    return tuple(out)
