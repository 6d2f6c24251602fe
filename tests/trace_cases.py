"""The cases of the rollout trace (mppi_trace_rollouts), shared by tests/test_trace_cpu.py (the reference side alone: TOL_STATE,
the cap of undecided rollouts) and tests/test_trace_gpu.py: problems, the fp32 oracle's applied controls, the float64 state
loop, ref64's branch record and the decided sets, each computed once.

K = 128 everywhere: rollout 0 is the noise-free one, rollout 127 a pure-noise one (k >= .99 K).  The scenes are the oval (affine
transform, the shipped launch file's cost with both control-cost coefficients 0) and tests/scenes.py's patchwork and tilt-slide
(projective transform; boundary, slop, slip and roll branches fire) with the two control-cost coefficients set to 0: with a
control cost the library refuses the cost outputs (du = eps nu is not recoverable from the applied controls), and the
coefficients move no state, no margin and no flag."""
import ctypes as C
import functools
import os

import numpy as np

from autorally_amd import params as P
from autorally_amd import synthetic as S
from oracle import oracle as O
from tests import ref64 as R
from tests import scenes as SC
from tests.helpers import noise_for, warm_U

K = 128
f64 = np.float64

# TOL_STATE: ten times the largest per-component |fp32 oracle (mode 1) - float64 loop| of a state, both stepped over the same
# applied controls, over every case below, every rollout and every step (tests/test_trace_cpu.py re-measures and asserts that
# the constant still covers it).  Ten is the factor tests/measure_branch_deltas.py gives the oracle's own deviation: it stands
# for the device's tanh / sincos forms against libm.
MEASURED_STATE_DEV = 5.13e-6   # y of patchwork-bf-T37-s1 (metres); measured on the CPU before any GPU run
TOL_STATE = 5.2e-5

NETS = {
    "32x2": None, "64x2": [6, 64, 64, 4], "16-24": [6, 16, 24, 4], "32x3": [6, 32, 32, 32, 4], "33-97-66": [6, 33, 97, 66, 4],
    # past every fast form ("valu_lds" only): three and four neurons per lane, ragged tails; an image beyond the LDS; no hidden
    # layer; a list of MPPI_MAX_LAYERS entries
    "129": [6, 129, 4], "256-7": [6, 256, 7, 4], "200-256": [6, 200, 256, 4], "256x2": [6, 256, 256, 4], "none": [6, 4],
    "8deep": [6, 20, 70, 9, 130, 33, 65, 4], "bf": None,
    # lists whose k-major image is beyond the trace kernel's LDS budget (its weights come from global memory) and which
    # "valu_lds" still serves: four neurons per lane with ragged tails, and two full halves
    "197-67": [6, 197, 67, 4], "128x2": [6, 128, 128, 4],
    # three and four chains per lane over MORE THAN ONE chunk of 8 inputs (the read-ahead of trace_layer<3> and <4> is taken),
    # on lists "valu_lds" can still hold (at most 160 KB of LDS): 6-16-256-4 (153 040 B there: four chains at the full width,
    # two chunks, trace image in LDS), 6-64-200-4 (159 408 B: four chains with a ragged last one, eight chunks, LDS),
    # 6-70-193-4 (four chains, one neuron in the last, eight chunks and a ragged end of six inputs, image in GLOBAL memory),
    # 6-24-150-4 (three chains, three chunks, LDS) and 6-100-140-4 (three chains, twelve chunks and a ragged end, global)
    "16-256": [6, 16, 256, 4], "64-200": [6, 64, 200, 4], "70-193": [6, 70, 193, 4], "24-150": [6, 24, 150, 4],
    "100-140": [6, 100, 140, 4],
}
# mppi_create accepts these, but no rollout kernel of the library runs them: "valu_lds", the only form for lists this wide,
# needs the packed parameters and two activation tiles of 64 x max width floats in 160 KB of LDS (346 KB and 407 KB here), so
# mppi_compute_control fails at its launch and there is no solve to trace.  tests/test_trace_gpu.py holds that refusal and,
# should a rollout form for them appear, the full bar; the CPU tests keep them as cases.
NO_ROLLOUT_KERNEL = ("200-256", "256x2")

# (scene, net, T, optimization stride, rollout variants)
CASES = [
    ("oval", "32x2", 37, 1, ["row_exact", "quad", "valu", "row_tree", "multi4_tree"]),
    ("patchwork", "32x2", 5, 3, ["row_exact", "valu"]),
    ("tilt_l2", "32x2", 2, 0, ["row_exact", "quad"]),
    ("tilt_l1", "32x2", 37, 1, ["row_exact", "row_tree"]),
    ("oval", "64x2", 37, 0, ["m44_chain", "oct", "m44"]),
    ("tilt_l1", "64x2", 5, 1, ["m44_chain", "oct"]),
    ("patchwork", "64x2", 37, 3, ["oct", "m44"]),
    ("patchwork", "16-24", 37, 3, ["lds44"]),
    ("tilt_l2", "32x3", 37, 1, ["lds44"]),
    ("oval", "32x3", 2, 0, ["lds44"]),
    ("patchwork", "33-97-66", 37, 0, ["lds128"]),
    ("oval", "33-97-66", 5, 1, ["lds128"]),
    ("tilt_l2", "129", 37, 1, ["valu_lds"]),
    ("patchwork", "256-7", 5, 0, ["valu_lds"]),
    ("oval", "200-256", 37, 3, ["valu_lds"]),
    ("patchwork", "256x2", 37, 1, ["valu_lds"]),
    ("oval", "256x2", 2, 1, ["valu_lds"]),
    ("tilt_l2", "197-67", 37, 1, ["valu_lds"]),
    ("patchwork", "128x2", 37, 3, ["valu_lds", "lds128"]),
    ("oval", "197-67", 5, 0, ["valu_lds"]),
    ("patchwork", "16-256", 37, 1, ["valu_lds"]),
    ("tilt_l2", "64-200", 37, 0, ["valu_lds"]),
    ("oval", "70-193", 37, 3, ["valu_lds"]),
    ("patchwork", "24-150", 5, 1, ["valu_lds"]),
    ("tilt_l1", "100-140", 37, 1, ["valu_lds"]),
    ("oval", "none", 37, 1, ["valu_lds"]),
    ("patchwork", "8deep", 37, 1, ["valu_lds"]),
    ("tilt_l1", "8deep", 5, 3, ["valu_lds"]),
    ("patchwork", "bf", 37, 1, ["bf3", "quad", "fused"]),
    ("tilt_l1", "bf", 5, 3, ["bf3", "quad"]),
    ("oval", "bf", 2, 0, ["bf3", "fused"]),
]
CASE_IDS = ["%s-%s-T%d-s%d" % c[:4] for c in CASES]


@functools.lru_cache(maxsize=None)
def bf_W():
    return P.load_bf_npz(os.path.join(os.path.dirname(__file__), "golden", "models", "basis_function_09_12_2018.npz"))


def config(scene, net, T, stride, **over):
    kw = dict(bf_W=bf_W()) if net == "bf" else dict(layers=NETS[net])
    if scene == "oval":
        cfg = S.make_config(K, T, track="oval", **kw)
    else:
        cfg = SC.patchwork_config(K, T, **kw) if scene == "patchwork" else SC.tilt_slide_config(K, T, variant=scene[5:], **kw)
        cfg["cost"] = dict(cfg["cost"], steering_coeff=0.0, throttle_coeff=0.0)
    cfg["opt_stride"] = int(stride)
    cfg.update(over)
    return cfg


@functools.lru_cache(maxsize=None)
def problem(scene, net, T, stride):
    """(cfg, U0, eps [1, K, T, 2])"""
    cfg = config(scene, net, T, stride)
    U0 = warm_U(cfg) if scene == "oval" else SC.ramp_U(cfg, seed=T + 3)
    return cfg, U0, noise_for(cfg, 2000 + 7 * T + stride)


@functools.lru_cache(maxsize=None)
def oracle_V(scene, net, T, stride):
    """The applied controls of the fp32 oracle (the existing bars hold every kernel form's V to them bit for bit)."""
    cfg, U0, eps = problem(scene, net, T, stride)
    return O.Oracle(cfg, fma_mode=1, nthreads=8).rollouts(cfg["start_state"], U0, eps[0])[1]


def loop64(cfg, V):
    """The float64 state loop over given applied controls V [K, T, 2]: clamp (ref64's limits), Ref64.state_deriv, Euler update.
    Returns the state BEFORE the update of every step, [K, T, 7]."""
    r = R.Ref64(cfg)
    V = np.asarray(V, np.float32).astype(f64)
    n, T = V.shape[0], V.shape[1]
    s = np.tile(np.asarray(cfg["start_state"], np.float32).astype(f64).reshape(1, 7), (n, 1))
    out = np.empty((n, T, 7), f64)
    with np.errstate(all="ignore"):
        for t in range(T):
            out[:, t] = s
            s = s + r.state_deriv(s, np.clip(V[:, t], r.u_lo, r.u_hi)) * r.dt
    return out


def loop32(cfg, V):
    """The same loop stepped by the fp32 oracle in the reference's arithmetic (orc_update_state, mode 1), [K, T, 7]."""
    orc = O.Oracle(cfg, fma_mode=1)
    V = np.ascontiguousarray(V, np.float32)
    n, T = V.shape[0], V.shape[1]
    out = np.empty((n, T, 7), np.float32)
    s, u = np.zeros(7, np.float32), np.zeros(2, np.float32)
    fp = C.POINTER(C.c_float)
    sp, up, pp = s.ctypes.data_as(fp), u.ctypes.data_as(fp), C.byref(orc.p)
    for k in range(n):
        s[:] = np.asarray(cfg["start_state"], np.float32)
        for t in range(T):
            out[k, t] = s
            u[:] = V[k, t]
            orc.L.orc_update_state(pp, sp, up)
    return out


@functools.lru_cache(maxsize=None)
def states64(scene, net, T, stride):
    return loop64(problem(scene, net, T, stride)[0], oracle_V(scene, net, T, stride))


def boundary_settled(cfg, st):
    """[K] bool: at every costed step the boundary test of both car points gives one answer anywhere within DELTA_TEXEL of the
    point along both map axes (the same texel, or a neighbour on the same side of boundary_threshold)."""
    r = R.Ref64(cfg)
    thr = r.cost["boundary_threshold"]
    ok = np.ones(st.shape[0], bool)
    with np.errstate(all="ignore"):
        for t in range(1, st.shape[1]):
            s = st[:, t]
            c, sn = np.cos(s[:, 2]), np.sin(s[:, 2])
            for sg in (0.5, -0.5):
                x, y = s[:, 0] + sg * c, s[:, 1] + sg * sn
                here = r.texel(x, y) >= thr
                for dx, dy in ((SC.DELTA_TEXEL, 0.0), (-SC.DELTA_TEXEL, 0.0), (0.0, SC.DELTA_TEXEL), (0.0, -SC.DELTA_TEXEL)):
                    ok &= (r.texel(x + dx, y + dy) >= thr) == here
    return ok


@functools.lru_cache(maxsize=None)
def trace64(scene, net, T, stride):
    """ref64's branch record of the case with tr["decided"]: tests/scenes.py's margins and its DELTA per class (slip, roll;
    texel on the patchwork).  On the oval, whose texels are 0.1 m and smooth, the texel class is the boundary test itself:
    settled where no point within DELTA_TEXEL gives another answer (boundary_settled)."""
    cfg, U0, eps = problem(scene, net, T, stride)
    tr = R.Ref64(cfg).trace(cfg["start_state"], U0, eps[0])
    dec = SC.decided(cfg, tr)
    if scene == "oval":
        dec &= boundary_settled(cfg, states64(scene, net, T, stride))
    tr["decided"] = dec
    return tr


def fold_step_costs(step_costs):
    """running_mean over the step costs [n, T] on the host: J += (double)(float)(c - J) / t in f64, rounded to float."""
    c = np.asarray(step_costs, np.float32)
    J = np.zeros(c.shape[0], np.float32)
    for t in range(1, c.shape[1]):
        d = (c[:, t] - J).astype(f64)   # the subtraction in float, as the kernels do it
        J = (J.astype(f64) + d / f64(t)).astype(np.float32)
    return J
