"""The measurement behind DELTA_TEXEL, DELTA_ROLL and DELTA_SLIP of tests/scenes.py (a CPU probe, not a test; run it with
`python -m tests.measure_branch_deltas` after a change of a branch scene and write what it prints into the comment there), and
behind the edge scenes' DELTA_UX, DELTA_SLIP_CRAWL and DELTA_CAP (`python -m tests.measure_branch_deltas edge [scene ...]`:
every case of tests/edge_cases.py, the classes of the branch scenes plus ux, bf -- both held to DELTA_UX -- and cap).

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


EDGE_SCALE = {"texel": 1e-5, "roll": 1e-6, "slip": 1e-6, "ux": 1e-7, "bf": 1e-7, "cap": 1e-6}


def measure_edge(scenes=None):
    """The edge scenes: a rollout of the fp32 oracle beyond TOL64 is laid to the class whose margin is nearest (texel on the
    border and on the cap's patchwork only; slip in radians on every scene: on the crawl a radian of slip is 6.5e-3 m/s of u_x where the limit is crossed)."""
    from tests import edge_cases as EC
    worst = {c: (0.0, None) for c in EDGE_SCALE}
    n_bad = {c: 0 for c in EDGE_SCALE}
    n_roll = 0
    for scene in (scenes or EC.SCENES):
        for net in EC.NET_LAYERS:
            for K, T in EC.shapes(scene):
                for part in EC.parts(scene, net):
                    if not EC.held_to_ref64(scene, part):
                        continue
                    tr = EC.trace(scene, part, net, K, T)
                    n_roll += K
                    inf = np.full(K, np.inf)
                    margins = {"texel": tr["m_texel"][:, 1:T].min(axis=1) if scene in ("border", "cap") else inf,
                               "slip": tr["m_slip"][:, 1:T].min(axis=1), "roll": tr["m_roll"][:, 1:T].min(axis=1),
                               "ux": tr["m_ux"][:, 1:T].min(axis=1), "bf": tr["m_bf"][:, :T - 1].min(axis=1),
                               "cap": tr["m_cap"][:, 1:T].min(axis=1)}
                    for mode in (1, 0):
                        e = rel_err(EC.oracle(scene, part, net, K, T, mode)[0], tr["costs"])
                        for k in np.nonzero(e > TOL64)[0]:
                            cls = min(margins, key=lambda c: margins[c][k] / EDGE_SCALE[c])
                            n_bad[cls] += 1
                            if margins[cls][k] > worst[cls][0]:
                                worst[cls] = (float(margins[cls][k]), (scene, part, net, K, T, mode, int(k), float(e[k])))
                    print("%s/%s net=%s K=%d T=%d: %d undecided" % (scene, part, net, K, T, int(K - tr["decided"].sum())), flush=True)
    print("%d rollouts x 2 modes" % n_roll)
    for c in EDGE_SCALE:
        print("EDGE DELTA %s: largest margin of an oracle rollout beyond TOL64 %.3g (%d such rollouts) at %s" % (c, worst[c][0], n_bad[c], worst[c][1]))


if __name__ == "__main__":
    import sys
    if len(sys.argv) > 1 and sys.argv[1] == "edge":
        measure_edge(sys.argv[2:] or None)
    else:
        measure()
