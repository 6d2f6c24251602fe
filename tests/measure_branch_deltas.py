"""The measurement behind DELTA_TEXEL, DELTA_ROLL and DELTA_SLIP of tests/scenes.py (a CPU probe, not a test; run it with
`python -m tests.measure_branch_deltas` after a change of a branch scene and write what it prints into the comment there).

For every case of tests/branch_cases.py it compares the fp32 oracle, modes 1 and 0, with ref64 on every rollout.  A rollout
beyond TOL64 is laid to the margin class it is nearest to (each margin taken against the fp32 resolution of its class: 1e-5 m,
1e-6 rad, 1e-6 rad); per class the LARGEST such margin is printed.  DELTA is ten times that, rounded up."""
import numpy as np

from tests import branch_cases as BC
from tests.helpers import rel_err
from tests.scenes import TOL64

SCALE = {"texel": 1e-5, "roll": 1e-6, "slip": 1e-6}


def measure():
    worst = {c: (0.0, None) for c in SCALE}
    n_bad = {c: 0 for c in SCALE}
    for scene in BC.SCENES:
        for net in BC.NET_LAYERS:
            for K, T in BC.SHAPES:
                tr = BC.trace(scene, net, K, T)
                mt = tr["m_texel"][:, 1:T].min(axis=1) if scene == "patchwork" else np.full(K, np.inf)
                ms = tr["m_slip"][:, 1:T].min(axis=1)
                m, over = tr["m_roll"][:, 1:T], tr["roll_over"][:, 1:T]
                sure = over & (m >= 1e-9)   # as scenes.decided: the roll counts up to its first firing
                mr = np.where(np.cumsum(sure, axis=1) - sure == 0, m, np.inf).min(axis=1)
                for mode in (1, 0):
                    e = rel_err(BC.oracle(scene, net, K, T, mode)[0], tr["costs"])
                    for k in np.nonzero(e > TOL64)[0]:
                        margins = {"texel": mt[k], "roll": mr[k], "slip": ms[k]}
                        cls = min(margins, key=lambda c: margins[c] / SCALE[c])
                        n_bad[cls] += 1
                        if margins[cls] > worst[cls][0]:
                            worst[cls] = (float(margins[cls]), (scene, net, K, T, mode, int(k), float(e[k])))
                print("%s net=%s K=%d T=%d: %d undecided" % (scene, net, K, T, int(K - tr["decided"].sum())), flush=True)
    for c in SCALE:
        print("DELTA %s: largest margin of an oracle rollout beyond TOL64 %.3g (%d such rollouts) at %s" % (c, worst[c][0], n_bad[c], worst[c][1]))


if __name__ == "__main__":
    measure()
