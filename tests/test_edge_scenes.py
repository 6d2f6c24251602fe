"""The edge scenes (tests/scenes.py: border, crawl, cap, stiff) on the CPU, for every case tests/test_edge_rollouts_gpu.py runs:
  * the scenes' own conditions: the border map and its transform, the quadrants of the start headings, the stiff network's
    pre-activations and its flip-freedom;
  * the cap on undecided rollouts (at most UNDECIDED_CAP of K) from ref64 alone;
  * coverage: a stated least share of the decided rollouts leaves the map across the case's border or corner, comes back, passes
    under 0.001 m/s, reverses, crosses the slip limit both ways, is capped on some steps but not all;
  * the fp32 oracle in modes 1 and 0 on every decided rollout, within 0.2 TOL64 of ref64;
  * mutants of ref64, one branch each: the GPU file's bar (edge_cases.hold, edge_cases.hold_start_state) rejects every one.
Everything here reads ref64 and the oracle only."""
import numpy as np
import pytest

from tests import edge_cases as EC
from tests import ref64 as R
from tests import scenes as SC
from tests.helpers import rel_err
from tests.scenes import TOL64

CASES = [(scene, net, K, T) for scene in EC.SCENES for net in EC.NET_LAYERS for K, T in EC.shapes(scene)]


def _id(v):
    return str(v)


def test_the_border_map_and_its_transform():
    cfg = EC.problem("border", "ne", "64x2", 1984, 37)[0]
    m = cfg["map_rgba"][:, :, 0].astype(np.float64)
    assert m.shape == (SC.BORDER_H, SC.BORDER_W) and SC.BORDER_W != SC.BORDER_H
    thr, slop = float(np.float32(cfg["cost"]["boundary_threshold"])), float(np.float32(cfg["cost"]["track_slop"]))
    v = np.unique(m)
    assert np.all(np.abs(v - thr) >= 0.01)
    avg = (v[:, None] + v[None, :]) / 2.0
    for s in (slop, 0.045):   # the second handle of a shared launch has another slop
        assert np.all(np.abs(avg - float(np.float32(s))) >= 1e-3)
    assert np.all(np.abs(np.diff(m, axis=0)) >= SC.PATCH_NEIGHBOUR_MIN - 1e-6) and np.all(np.abs(np.diff(m, axis=1)) >= SC.PATCH_NEIGHBOUR_MIN - 1e-6)
    for name, line in (("w", m[:, 0]), ("e", m[:, -1]), ("s", m[0, :]), ("n", m[-1, :])):
        assert np.all(np.abs(np.diff(line)) >= SC.PATCH_NEIGHBOUR_MIN - 1e-6), name
        assert line.min() < slop < line.max() and line.min() < thr < line.max(), (name, line.min(), line.max())
    # a clamp with the sizes swapped, to the last texel but one, or none at all reads another value on every border texel
    assert np.all(np.abs(m[:, -1] - m[:, -2]) >= 0.03 - 1e-6) and np.all(np.abs(m[-1, :] - m[-2, :]) >= 0.03 - 1e-6)
    # the projective third row stays, w > 0 over everything a rollout can reach: 15 m beyond every border (w is linear)
    assert tuple(np.float32([cfg["r_c1"][2], cfg["r_c2"][2]]).tolist()) == tuple(np.float32(SC.PROJ).tolist())
    hx, hy = SC.BORDER_W * SC.PATCH_TEXEL_M / 2 + 15.0, SC.BORDER_H * SC.PATCH_TEXEL_M / 2 + 15.0
    for x in (-hx, hx):
        for y in (-hy, hy):
            assert cfg["r_c1"][2] * x + cfg["r_c2"][2] * y + cfg["trs"][2] > 0.9


def test_the_start_headings_reach_negative_and_high_quadrants():
    """sincos_fast's quadrant number q = rint(heading x 2 / pi) of the border poses (verified there: 2 m texels) and of the
    stiff headings (exercised there: on the ramp a wrong quadrant moves a cost by less than the bar)."""
    q = {int(np.rint(SC.border_pose(b, **st)[2] * 2.0 / np.pi)) for (fam, T, b), st in SC.BORDER_START.items()}
    print("EDGE quadrants of the border poses: %s" % sorted(q))
    assert min(q) <= -3 and max(q) >= 3 and {-1, -2} & q
    qs = [int(np.rint(float(np.float32(h)) * 2.0 / np.pi)) for h in SC.STIFF_HEADINGS]
    assert qs == [-1, -2, 3, 4000], qs


def _check_border(ev, part, T, tag):
    """Across the case's border or corner: MIN_LEAVE of the decided rollouts; up to T = 37 MIN_STAY do not cross it; at T = 100
    MIN_BACK of them are back on the map with both car points (the four borders; past a corner a car is 12 m out)."""
    assert ev["across"] >= EC.MIN_LEAVE, (tag, ev)
    if T <= 37:
        assert 1.0 - ev["across"] >= EC.MIN_STAY, (tag, ev)
    elif len(part) == 1:
        assert ev["back"] >= EC.MIN_BACK, (tag, ev)


def _check_stiff(scene, part, net, K, T):
    """Flip-free as tests/test_ref64.py holds the ramp: u_x > 1, no crash flag, RAMP_FLIP_BOUND; and the pre-activations of the
    scaled-up hidden units over the K rollouts: beyond +- STIFF_SPAN and inside (-2, 2)."""
    cfg, U0, eps = EC.problem(scene, part, net, K, T)
    tr = EC.trace(scene, part, net, K, T)
    assert SC.RAMP_FLIP_BOUND <= 1e-6 and cfg["cost"]["max_slip_ang"] >= np.pi / 2 and cfg["cost"]["track_slop"] == 0.0
    assert float(tr["min_ux"].min()) > 1.0 and not tr["crash"].any() and tr["decided"].all()
    assert float(tr["m_slip"][:, 1:].min()) > 0.5 and float(tr["m_roll"][:, 1:].min()) > 1.0
    if net == "bf":
        return None
    r = R.Ref64(cfg)
    r.pre_probe = []
    r.rollouts(cfg["start_state"], U0, eps[0])
    pre = np.stack(r.pre_probe)[:, :, :min(3, cfg["layers"][1])]   # [T, K, units]
    lo, hi, mid = float(pre.min()), float(pre.max()), int(np.sum(np.abs(pre) < 2.0))
    assert lo <= -SC.STIFF_SPAN and hi >= SC.STIFF_SPAN and mid > 0, (lo, hi, mid)
    return lo, hi, mid


@pytest.mark.parametrize("scene,net,K,T", CASES, ids=_id)
def test_cap_coverage_and_oracle_on_every_decided_rollout(scene, net, K, T):
    for part in EC.parts(scene, net):
        tag = (scene, part, net, K, T)
        tr = EC.trace(scene, part, net, K, T)
        dec = tr["decided"]
        n_und = int(K - dec.sum())
        assert n_und <= SC.UNDECIDED_CAP * K, (tag, n_und)
        assert np.all(np.isfinite(tr["costs"]))
        ev = EC.events(scene, part, tr)
        worst = 0.0
        for mode in (1, 0):
            costs, V = EC.oracle(scene, part, net, K, T, mode)
            assert np.all(np.isfinite(costs))
            assert float(np.max(np.abs(V - tr["V"]))) <= 1.2e-7
            if EC.held_to_ref64(scene, part):
                err = rel_err(costs, tr["costs"])
                worst = max(worst, float(err[dec].max()))
                assert float(err[dec].max()) <= 0.2 * TOL64, (tag, mode, int(np.argmax(np.where(dec, err, 0))), float(err[dec].max()))
        extra = ""
        if scene == "border":
            _check_border(ev, part, T, tag)
        elif scene == "crawl":
            assert ev["slow"] >= (EC.MIN_SLOW if K > 64 else EC.MIN_SLOW_64) and ev["reversed"] >= EC.MIN_REVERSED, (tag, ev)
            if K > 64:   # among 64 rollouts over 17 steps the shares of two crossings are a handful of rollouts
                assert min(ev["slip_up"], ev["slip_down"]) >= EC.MIN_SLIP_BOTH_WAYS, (tag, ev)
            else:
                assert min(ev["slip_up"], ev["slip_down"]) > 0, (tag, ev)
            if net == "bf":
                assert ev["bf_down"] >= EC.MIN_SLOW and ev["bf_up"] > 0, (tag, ev)   # u_x through .1 both ways
        elif scene == "cap":
            want = {"over": ("part_capped", EC.MIN_PART_CAPPED), "on": ("all_capped", 0.9)}.get(part)
            if want:
                assert ev[want[0]] >= want[1], (tag, ev)
            else:
                assert ev["part_capped"] == 0 and ev["all_capped"] == 0 and ev["crashed"] >= EC.MIN_PART_CAPPED, (tag, ev)
                assert float(tr["m_cap"][:, 1:].min()) >= 1e-3 and float(tr["costs"].max()) > 1e10
        else:
            extra = "; pre-activations %s" % (_check_stiff(scene, part, net, K, T),)
        print("EDGE %s/%s net=%s K=%d T=%d: %d undecided (cap %d), oracle on the decided max %.2e (bar %.0e), shares %s%s" % (
            scene, part, net, K, T, n_und, int(SC.UNDECIDED_CAP * K), worst, 0.2 * TOL64, {k: round(v, 3) for k, v in ev.items() if v}, extra))


@pytest.mark.parametrize("scene,part,net,K,T,inst", EC.OTHER_LAUNCH_CASES, ids=_id)
def test_cap_and_oracle_on_the_other_launch_paths(scene, part, net, K, T, inst):
    """The capacity K and the second handle of a shared launch of the GPU file."""
    tr = EC.trace(scene, part, net, K, T, inst)
    dec = tr["decided"]
    assert int(K - dec.sum()) <= SC.UNDECIDED_CAP * K
    ev = EC.events(scene, part, tr)
    if scene == "border":
        assert ev["across"] >= EC.MIN_LEAVE, ev
    else:
        assert ev["slow"] >= EC.MIN_SLOW and ev["reversed"] >= EC.MIN_REVERSED, ev
    for mode in (1, 0):
        err = rel_err(EC.oracle(scene, part, net, K, T, mode, inst)[0], tr["costs"])
        assert float(err[dec].max()) <= 0.2 * TOL64, (mode, float(err[dec].max()))
    print("EDGE other %s/%s net=%s K=%d T=%d inst=%d: %d undecided, shares %s" % (scene, part, net, K, T, inst, int(K - dec.sum()),
                                                                               {k: round(v, 3) for k, v in ev.items() if v}))


# ------------------------------------------------------------------------------------------------------------------ mutants
class ClampToLastButOne(R.Ref64):
    """the upper clamp at W - 2 / H - 2"""
    def clamp_index(self, f, n):
        return super().clamp_index(f, n - 1)


class ClampSizesSwapped(R.Ref64):
    """W and H swapped in the clamp"""
    def clamp_sizes(self):
        W, H = super().clamp_sizes()
        return H, W

    def fetch(self, fi, fj):
        return self.map0[np.minimum(fj, self.map0.shape[0] - 1), fi]


class NoLowerClamp(R.Ref64):
    """no lower clamp: a column -1 is the last texel of the row before (the flat index wraps at the map's start)"""
    def clamp_index(self, f, n):
        return np.minimum(np.where(np.isnan(f), 0.0, np.maximum(f, -1.0)), n - 1).astype(np.int64)

    def fetch(self, fi, fj):
        return self.map0.reshape(-1)[(fj * self.map0.shape[1] + fi) % self.map0.size]


class NaNToTheLastTexel(R.Ref64):
    """a NaN coordinate clamped to the last texel (fminf(fmaxf(..)) in the other order)"""
    def clamp_index(self, f, n):
        return np.where(np.isnan(f), n - 1, super().clamp_index(f, n))


class NoSpeedGuard(R.Ref64):
    """the stabilizing cost without its |u_x| > 0.001 guard"""
    def moving(self, ux):
        return np.ones(ux.shape, bool)


class SignedSpeedGuard(R.Ref64):
    """the guard on the signed u_x"""
    def moving(self, ux):
        return ux > 0.001


class BfSwitchAtZero(R.Ref64):
    """the basis functions' switch at u_x >= 0"""
    def bf_big(self, ux):
        return ux >= 0.0


class NoCap(R.Ref64):
    """no 1e12 cap"""
    def cap(self, cost):
        return cost


class CapOnTheMean(R.Ref64):
    """the cap on the running mean, not on the step"""
    def cap(self, cost):
        return cost

    def accumulate(self, running, cost, t):
        return super().cap(super().accumulate(running, cost, t))


class CapValueIsTheThreshold(R.Ref64):
    """a capped step set to the float the compare uses (the next float above 1e12), not to (float)1e12"""
    def cap(self, cost):
        return np.where((cost > 1e12) | np.isnan(cost), 1000000061440.0, cost)


# mutant -> the (scene, part, net) it is shown; atan(u_y / u_x) in place of atan(u_y / |u_x|) is no mutant: the slip angle
# enters the cost as slip^2 and |slip| only, and atan is odd, so the two are the same function of the state.
MUTANTS = {ClampToLastButOne: [("border", "ne", "32x2"), ("border", "e", "64x2")],
           ClampSizesSwapped: [("border", "ne", "32x2"), ("border", "e", "64x2")],
           NoLowerClamp: [("border", "sw", "32x2"), ("border", "w", "64x2")],
           NaNToTheLastTexel: [("start", "heading_nan", "32x2")],
           NoSpeedGuard: [("crawl", "0.03", "32x2")], SignedSpeedGuard: [("crawl", "-0.05", "32x2")],
           BfSwitchAtZero: [("crawl", "0.13", "bf")],
           NoCap: [("cap", "over", "32x2")], CapOnTheMean: [("cap", "over", "32x2")], CapValueIsTheThreshold: [("cap", "on", "32x2")]}


@pytest.mark.parametrize("K,T", EC.SHAPES)
def test_the_bar_rejects_every_mutant(K, T):
    """The bar of the GPU file on each mutant's costs (as floats, named as an order-exact form) -- at BOTH shapes every form is
    run at; ref64's own costs pass it."""
    rows = []
    quiet = lambda *a: None
    for M, where in MUTANTS.items():
        for scene, part, net in where:
            if scene == "start":
                cfg, U0, eps, state = EC.start_state_problem(net, K, part)
                ok = EC.hold_start_state("ref64", net, K, part, dict(costs=EC.start_state_trace(net, K, part)["costs"].astype(np.float32),
                                                                    variant="valu_lds"), out=quiet)
                with np.errstate(all="ignore"):
                    costs = M(cfg).rollouts(state, U0, eps[0])[0]
                hold = lambda got: EC.hold_start_state("mutant", net, K, part, got, out=quiet)
            else:
                cfg, U0, eps = EC.problem(scene, part, net, K, T)
                EC.hold("ref64", scene, part, net, K, T, dict(costs=EC.trace(scene, part, net, K, T)["costs"].astype(np.float32),
                                                              variant="valu_lds"), out=quiet)
                costs = M(cfg).rollouts(cfg["start_state"], U0, eps[0])[0]
                hold = lambda got: EC.hold("mutant", scene, part, net, K, T, got, out=quiet)
            try:
                hold(dict(costs=costs.astype(np.float32), variant="valu_lds"))
                rejected = ""
            except AssertionError as e:
                rejected = str(e).splitlines()[0][:90]
            rows.append((M.__name__, scene, part, net, rejected))
    for row in rows:
        print("EDGE MUTANT K=%d T=%d  %-24s %s/%s net=%s: %s" % ((K, T) + row[:4] + ("rejected " + row[4] if row[4] else "ACCEPTED",)))
    accepted = sorted({r[0] for r in rows} - {r[0] for r in rows if r[4]})
    assert not accepted, accepted
