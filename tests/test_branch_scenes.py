"""The branch scenes (tests/scenes.py: patchwork, tilt-slide) on the CPU, for every case tests/test_branch_rollouts_gpu.py runs:
  * the patchwork map's conditions, the cap on undecided rollouts (at most UNDECIDED_CAP of K), u_x > 1;
  * the fp32 oracle in modes 1 and 0 against ref64 on every DECIDED rollout (tests/scenes.py: decided), within 0.2 TOL64;
  * coverage: the branches fire among the decided rollouts, at the steps and from the sources where a kernel can go wrong;
  * mutants of ref64, one deviation each: the decided-rollout bar rejects every one of them, the statistical bars of the
    parity and fuzz tests accept some (the table is printed).
Everything here reads ref64 and the oracle only."""
import numpy as np
import pytest

from tests import branch_cases as BC
from tests import ref64 as R
from tests import scenes as SC
from tests.helpers import rel_err
from tests.scenes import TOL64

MI355X_CUS = 256   # the GPU file's capacity case: 2 groups of 16 rollouts per CU and one 64-block more
CASES = [(scene, net, K, T, 0) for scene in BC.SCENES for net in BC.NET_LAYERS for K, T in BC.SHAPES]
CASES += [("patchwork", net, 2 * MI355X_CUS * 16 + 64, 17, 0) for net in ("32x2", "64x2", "32x3", "128x2")]
CASES += [("patchwork", net, K, 100, inst) for net in ("64x2", "32x3", "128x2") for inst, K in ((0, 1984), (1, 1920))]
CASES = sorted(set(CASES), key=CASES.index)


def _id(v):
    return str(v)


def test_the_patchwork_map_leaves_the_compares_to_the_texel():
    for inst in (0, 1):
        cfg = BC.problem("patchwork", "64x2", 1920 if inst else 1984, 100, inst)[0]
        SC.check_patchwork_map(cfg)
        assert 1.0 <= SC.PATCH_TEXEL_M <= 2.0 and cfg["map_rgba"].shape[0] * SC.PATCH_TEXEL_M == 2 * SC.MAP_HALF
        assert abs(cfg["cost"]["track_slop"] - 0.05) <= 0.01 and cfg["opt_stride"] == 2
        assert cfg["cost"]["steering_coeff"] > 0 and cfg["cost"]["throttle_coeff"] > 0
        assert tuple(np.float32(cfg["r_c1"][2:]).tolist() + np.float32(cfg["r_c2"][2:]).tolist()) == tuple(np.float32(SC.PROJ).tolist())


def test_the_tilt_slide_settings():
    for variant in SC.TILT_COSTS:
        cfg = SC.tilt_slide_config(64, 17, variant=variant)
        assert cfg["cost"]["discount"] != 0.1 and 0.2 <= cfg["cost"]["max_slip_ang"] <= 0.3
        assert np.array_equal(cfg["map_rgba"], SC.ramp_map())
    assert SC.TILT_COSTS["l1"]["l1_cost"] and not SC.TILT_COSTS["l2"]["l1_cost"]


@pytest.mark.parametrize("scene,net,K,T,inst", CASES, ids=_id)
def test_cap_and_oracle_against_ref64_on_every_decided_rollout(scene, net, K, T, inst):
    """At most UNDECIDED_CAP of the rollouts are undecided; on every decided one the oracle's cost, with and without fused
    multiply-adds, is within 0.2 TOL64 of ref64 (as test_ref64.py holds it on the ramp); every cost is finite, every applied
    control within an ulp; u_x > 1 on every step (the 0.001 and .1 switches stay out of reach), the map's border too."""
    tr = BC.trace(scene, net, K, T, inst)
    dec = tr["decided"]
    n_und = int(K - dec.sum())
    assert n_und <= SC.UNDECIDED_CAP * K, (n_und, K)
    assert float(tr["min_ux"].min()) > 1.0, float(tr["min_ux"].min())
    assert np.all(np.isfinite(tr["costs"])) and float(tr["costs"].max()) < 1e6
    worst = 0.0
    for mode in (1, 0):
        costs, V = BC.oracle(scene, net, K, T, mode, inst)
        assert np.all(np.isfinite(costs))
        assert float(np.max(np.abs(V - tr["V"]))) <= 1.2e-7
        err = rel_err(costs, tr["costs"])
        worst = max(worst, float(err[dec].max()))
        assert float(err[dec].max()) <= 0.2 * TOL64, (mode, int(np.argmax(np.where(dec, err, 0))), float(err[dec].max()))
    print("BRANCH %s net=%s K=%d T=%d inst=%d: %d undecided (cap %d), oracle on the decided max %.2e (bar %.0e), on the "
          "undecided max %.2e" % (scene, net, K, T, inst, n_und, int(SC.UNDECIDED_CAP * K), worst, 0.2 * TOL64,
                                  float(err[~dec].max()) if n_und else 0.0))


COVER_NETS = list(BC.NET_LAYERS)


PATCH_CASES = [c[1:] for c in CASES if c[0] == "patchwork"]


@pytest.mark.parametrize("net,K,T,inst", PATCH_CASES, ids=_id)
def test_the_track_branches_fire_on_the_patchwork(net, K, T, inst):
    """Among the decided rollouts of EVERY patchwork case of the GPU file -- the capacity K and the second handle of a shared
    launch included: 20-80 % crash on the boundary, at least 10 % never crash.
      T = 37, 100: the first crashes fall on steps of all four residues mod 4 (the row kernels hand over per chunk of four
        steps), beyond the 16-step ring and on the last step T-1; at least 5 % of the rollouts have a step whose track cost the
        slop zeroes and one it does not.
      T = 100, where the fan of rollouts is metres wide: the first crash is set by the front point alone and by the back point
        alone, and crashed rollouts have steps with BOTH points on the boundary.  A first crash set by both points in one step
        (source 3) needs the two points, 1 m apart on the line the car moves along, to enter boundary texels in the same
        0.12 m step out of texels that are off the boundary: with 2 m texels the texel one point would have to enter is the
        one the other is leaving, unless the car slides sideways.  The basis-function model does slide: its case asserts
        source 3 too; the network cases print the count.  At T = 37 the fan is a metre wide and the front point leads it
        into every texel; the shared launches of the GPU file therefore run at T = 100.
      T = 17: the fan is 0.2 m wide and long; a boundary texel's edge cuts it during its last three steps: first crashes on
        at least two residues mod 4 (the basis-function case: set by the back point)."""
    tr = BC.trace("patchwork", net, K, T, inst)
    dec = tr["decided"]
    n = int(dec.sum())
    first, src = tr["first"], tr["source"]
    crashed = dec & (first >= 0)
    assert not np.any(src & 4), "the roll flag stays out of this scene"
    share = crashed.sum() / n
    z = tr["zeroed"][:, 1:]
    mixed = float(np.mean((z.any(axis=1) & (~z).any(axis=1))[dec]))
    res = np.bincount(first[crashed] % 4, minlength=4)
    both_on = (tr["front"] & tr["back"]).any(axis=1)
    counts = dict(front=int(np.sum(crashed & (src == 1))), back=int(np.sum(crashed & (src == 2))), both_on=int(np.sum(crashed & both_on)),
                  both_first=int(np.sum(crashed & (src == 3))))
    print("BRANCH cover patchwork net=%s K=%d T=%d inst=%d: %d decided, %.3f crash (first steps mod 4: %s, %d .. %d, %d at T-1), "
          "sources %s, %.3f slop-mixed" % (net, K, T, inst, n, share, res.tolist(), int(first[crashed].min()), int(first[crashed].max()),
                                         int(np.sum(first[crashed] == T - 1)), counts, mixed))
    assert 0.2 <= share <= 0.8 and 1.0 - share >= 0.1
    if T == 17:
        assert np.sum(res > 0) >= 2
        return
    assert np.all(res > 0) and int(first[crashed].max()) > 16 and np.any(first[crashed] == T - 1)
    assert mixed >= 0.05
    if T == 100:
        assert min(counts["front"], counts["back"], counts["both_on"]) > 0, counts
        assert net != "bf" or counts["both_first"] > 0, counts


@pytest.mark.parametrize("K,T", BC.SHAPES)
@pytest.mark.parametrize("net", COVER_NETS)
@pytest.mark.parametrize("scene", ["tilt_l2", "tilt_l1"])
def test_the_state_branches_fire_on_the_tilt_slide(scene, net, K, T):
    """Among the decided rollouts: 20-80 % get the roll flag, first after at least T / 4 distinct updates, one of them the final
    update -- whose flag no cost sees; at least 10 % go over the slip limit and come back under it; each control is cut at
    each limit on at least 5 % of the (k, t); more than K / 2 distinct costs; the boundary never fires."""
    tr = BC.trace(scene, net, K, T)
    dec = tr["decided"]
    n = int(dec.sum())
    rf = tr["roll_first"]
    fired = dec & (rf >= 0)
    over = tr["over"][:, 1:]
    back = (over[:, :-1] & ~over[:, 1:]).any(axis=1)
    cl = tr["clamp"]
    cuts = [float(np.mean(cl[:, :, j] == v)) for j in (0, 1) for v in (-1, 1)]
    last = fired & (rf == T - 1)
    print("BRANCH cover %s net=%s K=%d T=%d: %d decided, %.3f tip over (%d distinct updates, %d at the final one), %.3f over the "
          "slip limit and back, cuts %s" % (scene, net, K, T, n, fired.sum() / n, len(np.unique(rf[fired])), int(last.sum()),
                                            float(np.mean(back[dec])), np.round(cuts, 3).tolist()))
    assert not tr["front"].any() and not tr["back"].any()
    assert 0.2 <= fired.sum() / n <= 0.8
    assert len(np.unique(rf[fired])) >= T / 4.0
    assert last.any() and np.all(tr["first"][last] == -1) and np.all(tr["crash"][last] == 1)
    assert np.all(tr["first"][fired & ~last] == rf[fired & ~last] + 1) and np.all(tr["source"][fired & ~last] == 4)
    assert float(np.mean(back[dec])) >= 0.1
    assert min(cuts) >= 0.05, cuts
    assert len(np.unique(tr["costs"])) > K // 2


# ------------------------------------------------------------------------------------------------------------------ mutants
class RollEarly(R.Ref64):
    """the roll flag seen one step early: step t's cost takes the flag of the state AFTER update t"""
    def compute_cost(self, s, u, du, crash, v=None, out=None):
        crash |= self.rolled(s + self.state_deriv(s, u) * self.dt).astype(crash.dtype)
        return super().compute_cost(s, u, du, crash, v, out)


class RollLate(R.Ref64):
    """the roll flag seen one step late"""
    def trace(self, state, U, eps):
        self._pending = None
        return super().trace(state, U, eps)

    def after_update(self, s, crash):
        if self._pending is not None:
            crash |= self._pending
        self._pending = self.rolled(s).astype(crash.dtype)


class NotSticky(R.Ref64):
    """the flag recomputed per step from this step's roll and texels"""
    def compute_cost(self, s, u, du, crash, v=None, out=None):
        crash[:] = self.rolled(s).astype(crash.dtype)
        return super().compute_cost(s, u, du, crash, v, out)


class FrontOnly(R.Ref64):
    """only the front point tested against the boundary"""
    def on_boundary(self, tf, tb):
        return tf >= self.cost["boundary_threshold"]


class SlipSigned(R.Ref64):
    """the slip test on the signed angle"""
    def slip_over(self, slip):
        return slip > self.cost["max_slip_ang"]


class RoundLookup(R.Ref64):
    """round for floor in the texel lookup"""
    def nearest(self, g):
        return np.floor(g + 0.5)


class NoDivision(R.Ref64):
    """the division by w dropped"""
    def grid(self, x, y):
        H, W = self.map0.shape
        return (self.r_c1[0] * x + self.r_c2[0] * y + self.trs[0]) * W, (self.r_c1[1] * x + self.r_c2[1] * y + self.trs[1]) * H


class UnclampedControlCost(R.Ref64):
    """the control cost with the unclamped u"""
    def control_cost(self, u, du, v):
        return super().control_cost(v, du, v)


class SlopOnScaled(R.Ref64):
    """the slop compare on track_coeff x track"""
    def slop_zeroed(self, track):
        return np.abs(self.cost["track_coeff"] * track) < self.cost["track_slop"]


MUTANTS = [RollEarly, RollLate, NotSticky, FrontOnly, SlipSigned, RoundLookup, NoDivision, UnclampedControlCost, SlopOnScaled]
RARE = dict(roll_below=2.9)   # a tilt-slide on which one or two rollouts in a hundred tip over


def _mutant_scene(name):
    K, T, net = 1984, 100, "32x2"
    if name == "tilt_rare":
        cfg = BC.config("tilt_l2", net, K, T, **RARE)
        from tests.helpers import noise_for
        U0, eps = SC.ramp_U(cfg, seed=K % 31 + T), noise_for(cfg, BC.noise_seed(T))
        tr = R.Ref64(cfg).trace(cfg["start_state"], U0, eps[0])
        tr["decided"] = SC.decided(cfg, tr)
        return cfg, U0, eps, tr
    return BC.problem(name, net, K, T) + (BC.trace(name, net, K, T),)


def _statistical_bars(r, costs, ref):
    """The two statistical bars on `costs` against the reference solve `ref` (costs, V): the parity tests' (at most K / 200
    rollouts beyond 1e-4, p99 < 5e-6, |dU| <= 1e-4) and the fuzz tests' (at most 3 % flipped, |dU| <= 2e-4 + 4 x their weight)."""
    K = len(costs)
    err = rel_err(costs, ref["costs"])
    fl = err > 1e-4
    w0, _, eta0, _ = r.weights(ref["costs"])
    w1, _, eta1, _ = r.weights(costs)
    dU = float(np.max(np.abs(r.weighted_reduction(w1, eta1, ref["V"]) - r.weighted_reduction(w0, eta0, ref["V"]))))
    mass = float(np.sum(np.maximum(w0 / eta0, w1 / eta1)[fl]))
    parity = int(fl.sum()) <= max(K // 200, 1) and float(np.percentile(err, 99)) < 5e-6 and dU <= 1e-4
    fuzz = float(np.mean(fl)) <= 0.03 and dU <= 2e-4 + 4.0 * mass
    return parity, fuzz, int(fl.sum()), dU, mass


def test_the_decided_bar_rejects_every_mutant_and_the_statistical_bars_do_not():
    """Each mutant of ref64 deviates in ONE branch.  The bar of tests/test_branch_rollouts_gpu.py -- every DECIDED rollout within
    TOL64 of ref64 -- rejects every mutant on some scene.  The fuzz bar accepts four of them (asserted): the roll flag one step
    early, one step late and not sticky on the tilt-slide on which 1 to 2 % of the rollouts tip over (asserted) -- their weight
    is nil, so no |dU| criterion sees them -- and the front-point-only boundary test on the patchwork."""
    rows, rejected, gap = [], set(), set()
    for scene in ("patchwork", "tilt_l2", "tilt_rare"):
        cfg, U0, eps, tr = _mutant_scene(scene)
        dec = tr["decided"]
        r = R.Ref64(cfg)
        assert _statistical_bars(r, tr["costs"], tr)[:2] == (True, True)
        if scene == "tilt_rare":
            tip = float(np.mean(tr["roll_first"] >= 0))
            print("MUTANTS  tilt_rare: %.4f of the rollouts tip over" % tip)
            assert 0.01 <= tip <= 0.02, tip
        for M in MUTANTS:
            costs = M(cfg).rollouts(cfg["start_state"], U0, eps[0])[0]
            e = rel_err(costs, tr["costs"])
            n_bad = int(np.sum(dec & (e > TOL64)))
            parity, fuzz, n_fl, dU, mass = _statistical_bars(r, costs, tr)
            rows.append((M.__name__, scene, n_bad, int(np.sum(e > TOL64)), n_fl, dU, parity, fuzz))
            if n_bad:
                rejected.add(M.__name__)
                if parity or fuzz:
                    gap.add(M.__name__)
    print("MUTANTS  %-22s %-10s %9s %9s %9s %9s  %-7s %-7s" % ("mutant", "scene", "decided>", "all>", ">1e-4", "|dU|", "parity", "fuzz"))
    for name, scene, n_bad, n_all, n_fl, dU, parity, fuzz in rows:
        print("MUTANTS  %-22s %-10s %9d %9d %9d %9.1e  %-7s %-7s" % (name, scene, n_bad, n_all, n_fl, dU, "accepts" if parity else "rejects",
                                                                    "accepts" if fuzz else "rejects"))
    assert rejected == {M.__name__ for M in MUTANTS}, sorted({M.__name__ for M in MUTANTS} - rejected)
    print("MUTANTS  accepted by a statistical bar and rejected on a decided rollout: %s" % sorted(gap))
    assert gap >= {"RollEarly", "RollLate", "NotSticky", "FrontOnly"}, sorted(gap)
