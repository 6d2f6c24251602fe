"""The cases of the edge scenes (tests/scenes.py: border, crawl, cap, stiff) shared by tests/test_edge_scenes.py (CPU: scene
conditions, caps, coverage, the oracle against ref64, mutants) and tests/test_edge_rollouts_gpu.py (every kernel form): problems,
ref64 traces, decided sets and oracle results, each computed once, and the bar both files apply.

A scene has PARTS -- the six borders and corners, the three start speeds, the cap's settings, the four headings -- and a case
(scene, net, K, T) runs all of them, one solve each."""
import functools

import numpy as np

from oracle import oracle as O
from tests import branch_cases as BC
from tests import ref64 as R
from tests import scenes as SC
from tests.helpers import noise_for, oracle_mode_for, rel_err
from tests.scenes import TOL64, TOL_MODE

U32 = np.uint32
SCENES = ["border", "crawl", "cap", "stiff"]
SHAPES = [(64, 17), (1984, 37)]     # one 64-block; an odd number of 64-blocks
BORDER_LONG = (1984, 100)           # the border only: a rollout that left the map comes back
NET_LAYERS = BC.NET_LAYERS
CAP_EXACT = np.float32(1e12)
INSTANCES = (0, 1, "trace")   # the problem itself; the second handle of a shared launch; the problem as mppi_trace_rollouts takes it

# the least share of the DECIDED rollouts of a case that must do each thing (tests/test_edge_scenes.py)
MIN_LEAVE, MIN_STAY, MIN_BACK, MIN_SLOW, MIN_REVERSED, MIN_PART_CAPPED, MIN_SLIP_BOTH_WAYS = 0.10, 0.05, 0.02, 0.10, 0.10, 0.10, 0.10
MIN_SLOW_64 = 0.04   # at K = 64: three rollouts (a share of 64 rollouts carries a sampling error of 0.04)


def parts(scene, net):
    if scene == "border":
        return list(SC.BORDER_POSES)
    if scene == "crawl":
        return ["%g" % v for v in ((SC.CRAWL_BF_SPEED,) if net == "bf" else SC.CRAWL_SPEEDS)]
    if scene == "cap":
        return list(SC.CAP_SETTINGS)
    return ["%g" % h for h in SC.STIFF_HEADINGS]


def shapes(scene):
    return SHAPES + ([BORDER_LONG] if scene == "border" else [])


def held_to_ref64(scene, part):
    """The 1000-turn heading is held to the fp32 oracle only: ref64 carries the heading in float64, the kernels in fp32, whose
    ulp at 6283 rad is 4.9e-4 rad."""
    return not (scene == "stiff" and float(part) == SC.STIFF_FAR)


def config(scene, part, net, K, T):
    kw = dict(bf_W=BC.bf_W()) if net == "bf" else dict(layers=NET_LAYERS[net])
    if scene == "border":
        return SC.border_config(K, T, part, **kw)
    if scene == "crawl":
        return SC.crawl_config(K, T, float(part), **kw)
    if scene == "cap":
        return SC.cap_config(K, T, part, **kw)
    return SC.stiff_config(K, T, float(part), **kw)


def noise_seed(T, inst=0):
    return 3000 + T + 50 * INSTANCES.index(inst)


@functools.lru_cache(maxsize=None)
def problem(scene, part, net, K, T, inst=0):
    """(cfg, U0, eps).  Instance 1 (the second handle of a shared launch): other cost parameters, its own nominal sequence and
    noise; the caller gives it another part as well.  Instance "trace": the two control-cost coefficients 0, as
    tests/trace_cases.py has them (with a control cost the library refuses the trace's cost outputs); its own noise."""
    cfg = config(scene, part, net, K, T)
    if inst == 1:
        cfg["cost"] = dict(cfg["cost"], desired_speed=7.0, speed_coeff=5.0, steering_coeff=0.9, track_slop=0.045)
    elif inst == "trace":
        cfg["cost"] = dict(cfg["cost"], steering_coeff=0.0, throttle_coeff=0.0)
    U0 = {"crawl": SC.crawl_U, "border": SC.border_U}.get(scene, SC.ramp_U)(cfg, seed=K % 31 + T + 7 * INSTANCES.index(inst))
    return cfg, U0, noise_for(cfg, noise_seed(T, inst))


@functools.lru_cache(maxsize=None)
def trace(scene, part, net, K, T, inst=0):
    cfg, U0, eps = problem(scene, part, net, K, T, inst)
    tr = R.Ref64(cfg).trace(cfg["start_state"], U0, eps[0])
    tr["decided"] = SC.decided(cfg, tr)
    return tr


@functools.lru_cache(maxsize=None)
def oracle(scene, part, net, K, T, mode, inst=0):
    cfg, U0, eps = problem(scene, part, net, K, T, inst)
    costs, V, crash = O.Oracle(cfg, fma_mode=mode, nthreads=16).rollouts(cfg["start_state"], U0, eps[0])
    return costs, V


def events(scene, part, tr):
    """Shares of the decided rollouts of a ref64 trace that do what the scene is about (the coverage the CPU file asserts and
    both files print)."""
    dec = tr["decided"]
    n = max(int(dec.sum()), 1)
    share = lambda m: float(np.sum(m & dec)) / n
    anyout = (tr["out_w"] | tr["out_e"] | tr["out_s"] | tr["out_n"])[:, 1:]
    ins = tr["inside"][:, 1:]
    was_out = np.cumsum(anyout, axis=1) > 0
    cap = tr["capped"][:, 1:]
    over = tr["over"][:, 1:]
    ev = dict(left=share(anyout.any(axis=1)), stayed=share(~anyout.any(axis=1)), back=share((was_out & ins).any(axis=1)),
              slow=share(tr["slow"][:, 1:].any(axis=1)), reversed=share(tr["reversed"][:, 1:].any(axis=1)),
              part_capped=share(cap.any(axis=1) & ~cap.all(axis=1)), all_capped=share(cap.all(axis=1)),
              crashed=share(tr["crash"] > 0),
              slip_up=share((~over[:, :-1] & over[:, 1:]).any(axis=1)), slip_down=share((over[:, :-1] & ~over[:, 1:]).any(axis=1)))
    fast = tr["fast"][:, :-1]
    ev.update(bf_down=share((fast[:, :-1] & ~fast[:, 1:]).any(axis=1)), bf_up=share((~fast[:, :-1] & fast[:, 1:]).any(axis=1)))
    if scene == "border":
        ev["across"] = share(tr["out_" + part][:, 1:].any(axis=1))
    return ev


def hold(tag, scene, part, net, K, T, got, want_name=None, inst=0, out=print):
    """The bar of tests/test_edge_rollouts_gpu.py -- that of tests/test_branch_rollouts_gpu.py -- on one solve's results `got`
    (costs, V, variant): the form's name; V bit-equal to the oracle for all rollouts; every decided rollout within TOL64 of
    ref64 and TOL_MODE of the oracle in the form's own mode; undecided rollouts finite; a rollout whose every costed step ref64
    caps exactly (float)1e12.  The decided set and its cap come from ref64 on the host.  Raises AssertionError."""
    tr = trace(scene, part, net, K, T, inst)
    dec = tr["decided"]
    n_und = int(K - dec.sum())
    assert n_und <= SC.UNDECIDED_CAP * K, (n_und, K)
    if want_name is not None:
        assert got["variant"] == want_name, (got["variant"], want_name)
    mode = oracle_mode_for(got["variant"])
    costs_o, V_o = oracle(scene, part, net, K, T, mode, inst)
    if got.get("V") is not None:
        np.testing.assert_array_equal(np.asarray(got["V"], np.float32).view(U32), V_o.view(U32))
    costs = np.asarray(got["costs"])
    assert np.all(np.isfinite(costs)), "a cost is not finite"
    e64 = rel_err(costs, tr["costs"]) if held_to_ref64(scene, part) else np.zeros(K)
    eo = rel_err(costs, costs_o)
    d64, do = np.where(dec, e64, 0.0), np.where(dec, eo, 0.0)
    k64, ko = int(np.argmax(d64)), int(np.argmax(do))
    ev = events(scene, part, tr)
    out("EDGE_ROLLOUT %s %s/%s net=%s K=%d T=%d form=%s mode=%d: %d decided, %d undecided; decided: ref64 max %.2e (k=%d, margin "
        "x%.1f)  oracle max %.2e (k=%d, margin x%.1f); undecided: ref64 max %.2e; events %s" % (
            tag, scene, part, net, K, T, got["variant"], mode, int(dec.sum()), n_und, d64[k64], k64, TOL64 / max(d64[k64], 1e-30),
            do[ko], ko, TOL_MODE / max(do[ko], 1e-30), float(e64[~dec].max()) if n_und else 0.0,
            {k: round(v, 3) for k, v in ev.items() if v}))
    assert float(d64[k64]) <= TOL64, ("ref64", k64, float(d64[k64]), int(np.sum(d64 > TOL64)), int(tr["first"][k64]))
    assert float(do[ko]) <= TOL_MODE, ("oracle mode %d" % mode, ko, float(do[ko]), int(np.sum(do > TOL_MODE)))
    full = dec & tr["capped"][:, 1:].all(axis=1) if T > 1 else np.zeros(K, bool)
    assert np.all(costs[full].astype(np.float32) == CAP_EXACT), ("capped on every step, not (float)1e12", int(np.sum(costs[full] != CAP_EXACT)))
    return float(d64[k64]), float(do[ko])


# ------------------------------------------------------------------------------------------- the other launch paths
MI355X_CUS = 256   # the capacity case: 2 groups of 16 rollouts per CU and one 64-block more
CAPACITY_PARTS = ("ne", "sw")            # the two corners: both ends of the clamp of both axes
CAPACITY_NETS = ("32x2", "64x2", "32x3", "128x2")
SHARED_NETS = ("64x2", "32x3", "128x2")
SHARED = {"border": (100, ("ne", "sw")), "crawl": (37, ("0.03", "-0.05"))}   # scene -> (T, the parts of the two handles)
SHARED_KS = (1984, 1920)
OTHER_LAUNCH_CASES = [("border", p, net, 2 * MI355X_CUS * 16 + 64, 17, 0) for net in CAPACITY_NETS for p in CAPACITY_PARTS]
OTHER_LAUNCH_CASES += [(scene, SHARED[scene][1][i], net, SHARED_KS[i], SHARED[scene][0], i) for scene in SHARED for net in SHARED_NETS
                       for i in (0, 1)]
# the "bf_row" pair of the basis-function model, on the border only (the crawl's shared parts are network start speeds)
OTHER_LAUNCH_CASES += [("border", SHARED["border"][1][i], "bf", SHARED_KS[i], SHARED["border"][0], i) for i in (0, 1)]
# "lds16" at the K where its launcher's rule picks 512 threads (6-128-128-128-4: one workgroup per CU) and 1024 (6-64x6-4)
LDS16_THREADS = (("128x3", 128, 512), ("64x6", 256, 1024))   # (net, rollouts per CU, threads per workgroup)
OTHER_LAUNCH_CASES += [("border", p, net, per_cu * MI355X_CUS, 17, 0) for net, per_cu, threads in LDS16_THREADS for p in CAPACITY_PARTS]


# ------------------------------------------------------------------------------------------- non-finite and huge start states
START_STATES = {"speed_nan": (4, np.nan), "x_inf": (0, np.inf), "heading_nan": (2, np.nan), "yaw_rate_minus_inf": (6, -np.inf),
                "speed_1e30": (4, 1e30), "x_1e20": (0, 1e20)}
START_KS, START_T = (64, 1984), 17
START_HIST = np.array([0.01, 0.3, -0.02, 0.33], np.float32)


@functools.lru_cache(maxsize=None)
def start_state_problem(net, K, which):
    """(cfg, U0, eps, state): the ramp's problem (tests/test_every_rollout_gpu.py) with one entry of the measured state
    replaced."""
    kw = dict(bf_W=BC.bf_W()) if net == "bf" else dict(layers=NET_LAYERS[net])
    cfg = SC.ramp_config(K, START_T, **kw)
    state = cfg["start_state"].copy()
    i, v = START_STATES[which]
    state[i] = v
    return cfg, SC.ramp_U(cfg, seed=K % 31 + START_T), noise_for(cfg, noise_seed(START_T)), state


@functools.lru_cache(maxsize=None)
def start_state_trace(net, K, which):
    cfg, U0, eps, state = start_state_problem(net, K, which)
    with np.errstate(all="ignore"):
        return R.Ref64(cfg).trace(state, U0, eps[0])


@functools.lru_cache(maxsize=None)
def start_state_oracle(net, K, which, mode):
    cfg, U0, eps, state = start_state_problem(net, K, which)
    costs, V, crash = O.Oracle(cfg, fma_mode=mode, nthreads=16).rollouts(state, U0, eps[0])
    return costs, V


def hold_start_state(tag, net, K, which, got, want_name=None, out=print):
    """The bar on a solve from a non-finite or huge start state: where ref64 says every costed step is capped the cost is exactly
    (float)1e12; every other cost within TOL_MODE of the oracle in the form's mode; V bit-equal; U (if given) finite and within
    2e-6 of ref64's weighting, reduction and smoothing fed with the solve's OWN costs and V (tests/test_stream_tail_gpu.py's bar)."""
    cfg, U0, eps, state = start_state_problem(net, K, which)
    tr = start_state_trace(net, K, which)
    if want_name is not None:
        assert got["variant"] == want_name, (got["variant"], want_name)
    mode = oracle_mode_for(got["variant"])
    costs_o, V_o = start_state_oracle(net, K, which, mode)
    costs = np.asarray(got["costs"])
    assert np.all(np.isfinite(costs)), ("a cost is not finite", int(np.sum(~np.isfinite(costs))))
    full = tr["capped"][:, 1:].all(axis=1)
    n_bad = int(np.sum(costs[full].astype(np.float32) != CAP_EXACT))
    eo = np.where(full, 0.0, rel_err(costs, costs_o))
    ko = int(np.argmax(eo))
    dU = -1.0
    if got.get("V") is not None:
        np.testing.assert_array_equal(np.asarray(got["V"], np.float32).view(U32), V_o.view(U32))
    if got.get("U") is not None:
        r = R.Ref64(cfg)
        w, beta, eta, tc = r.weights(costs)
        dU = float(np.max(np.abs(r.savgol(r.weighted_reduction(w, eta, got["V"]), START_HIST) - got["U"])))
    out("EDGE_START %s %s net=%s K=%d form=%s mode=%d: %d rollouts capped on every step (%d not exactly 1e12), %d capped in part, "
        "the others: oracle max %.2e (k=%d, margin x%.1f); |dU| %.2e" % (
            tag, which, net, K, got["variant"], mode, int(full.sum()), n_bad, int(np.sum(tr["capped"][:, 1:].any(axis=1) & ~full)),
            eo[ko], ko, TOL_MODE / max(eo[ko], 1e-30), dU))
    assert n_bad == 0, ("capped on every step, not (float)1e12", n_bad)
    assert float(eo[ko]) <= TOL_MODE, ("oracle mode %d" % mode, ko, float(eo[ko]), int(np.sum(eo > TOL_MODE)))
    if got.get("U") is not None:
        assert np.all(np.isfinite(got["U"])) and dU <= 2e-6, dU
