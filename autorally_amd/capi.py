"""ctypes binding of libmppi_hip.so (include/mppi_hip.h) -- plumbing for tests and bench.py.

The product is the shared library; this module only marshals numpy arrays across the C ABI.
It never computes anything itself and has no CPU fallback: if the library is missing or no
gfx950 device is usable, it raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# MPPI_LIB_PATH: developer override used for kernel A/B builds (scratch/), never a fallback
LIB_PATH = os.environ.get("MPPI_LIB_PATH") or os.path.join(HERE, "libmppi_hip.so")
MAX_LAYERS = 8

OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_STATE, ERR_UNSUPPORTED = range(6)


class Config(C.Structure):
    _fields_ = [
        ("device", C.c_int),
        ("num_rollouts", C.c_int),
        ("num_timesteps", C.c_int),
        ("hz", C.c_int),
        ("optimization_stride", C.c_int),
        ("gamma", C.c_float),
        ("num_iters", C.c_int),
        ("n_layers", C.c_int),
        ("layers", C.c_int * MAX_LAYERS),
        ("exploration_std", C.c_float * 2),
        ("init_control", C.c_float * 2),
        ("control_min", C.c_float * 2),
        ("control_max", C.c_float * 2),
        ("negate_yaw_der", C.c_int),
        ("seed", C.c_uint64),
    ]


class CostParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in (
        "desired_speed", "speed_coeff", "track_coeff", "max_slip_ang", "slip_penalty", "track_slop",
        "crash_coeff", "steering_coeff", "throttle_coeff", "boundary_threshold", "discount")] + [
        ("l1_cost", C.c_int)]


class StageTimes(C.Structure):
    _fields_ = [("n_solves", C.c_int), ("noise_ms", C.c_float), ("rollout_ms", C.c_float),
                ("weights_ms", C.c_float), ("reduction_ms", C.c_float), ("total_ms", C.c_float)]


# every symbol include/mppi_hip.h declares
SYMBOLS = [
    "mppi_abi_version", "mppi_strerror", "mppi_last_error", "mppi_device_count", "mppi_create",
    "mppi_destroy", "mppi_set_nn_params", "mppi_update_model", "mppi_set_control_limits",
    "mppi_set_costmap", "mppi_set_costmap_transform", "mppi_set_costmap_channel", "mppi_set_cost_params", "mppi_reset_controls",
    "mppi_set_control_seq", "mppi_get_control_seq", "mppi_set_control_hist", "mppi_get_control_hist",
    "mppi_savitsky_golay", "mppi_slide_control_seq", "mppi_seed", "mppi_set_noise", "mppi_generate_noise",
    "mppi_compute_control", "mppi_control_ticks", "mppi_compute_control_async", "mppi_synchronize",
    "mppi_compute_control_batch_async", "mppi_compute_control_batch", "mppi_control_ticks_batch", "mppi_get_results",
    "mppi_get_applied_controls", "mppi_rollout_only", "mppi_nominal_traj", "mppi_nominal_traj_pair",
    "mppi_set_bf_params", "mppi_set_ddp_weights", "mppi_debug_cost_raster", "mppi_compute_feedback_gains", "mppi_get_feedback_gains",
    "mppi_enable_stage_timing", "mppi_reset_stage_times", "mppi_get_stage_times",
    "mppi_rollout_variant", "mppi_set_rollout_variant", "mppi_debug_dynamics",
    "mppi_debug_inject_handover_fault", "mppi_compute_feedback_gains_pair", "mppi_set_host_threads",
    "mppi_debug_capture_iterations", "mppi_debug_get_iterations", "mppi_set_wait_timeout", "mppi_debug_form_candidates",
    "mppi_debug_set_chained_ticks", "mppi_debug_min_cost",
    "mppi_arm", "mppi_arm_batch", "mppi_disarm", "mppi_is_armed", "mppi_debug_launch_info",
    "mppi_trace_rollouts", "mppi_top_rollouts",
    "mppi_compute_feedback_gains_batch", "mppi_debug_ddp_info", "mppi_debug_device_tanhf",
    "mppi_nominal_traj_batch", "mppi_debug_nominal_info",
    "mppi_trace_rollouts_batch", "mppi_debug_trace_info",
    "mppi_nominal_and_gains_batch", "mppi_debug_nominal_and_gains_info",
    "mppi_closed_loop_ticks_batch", "mppi_debug_closed_loop_info", "mppi_debug_closed_loop_check",
    "mppi_set_plant_model", "mppi_debug_plant_model_info", "mppi_plant_drive_batch", "mppi_debug_plant_drive_info",
    "mppi_debug_plant_drive_host", "mppi_closed_loop_sim_batch",
]

ABI2_SYMBOLS = ("mppi_debug_inject_handover_fault", "mppi_savitsky_golay", "mppi_set_costmap_transform",
                "mppi_compute_control_batch", "mppi_compute_control_batch_async", "mppi_control_ticks_batch",
                "mppi_nominal_traj_pair")
ABI3_SYMBOLS = ("mppi_compute_feedback_gains_pair", "mppi_set_host_threads")
ABI4_SYMBOLS = ("mppi_debug_capture_iterations", "mppi_debug_get_iterations", "mppi_set_wait_timeout", "mppi_debug_form_candidates")
ABI5_SYMBOLS = ("mppi_debug_set_chained_ticks", "mppi_debug_min_cost", "mppi_arm", "mppi_arm_batch", "mppi_disarm",
                "mppi_is_armed")

# added to version 5 as compatible additions: an older version-5 library (a kernel A/B through MPPI_LIB_PATH) lacks them
UNVERSIONED_SYMBOLS = ("mppi_debug_launch_info", "mppi_trace_rollouts", "mppi_top_rollouts",
                       "mppi_compute_feedback_gains_batch", "mppi_debug_ddp_info", "mppi_debug_device_tanhf",
                       "mppi_nominal_traj_batch", "mppi_debug_nominal_info",
                       "mppi_trace_rollouts_batch", "mppi_debug_trace_info",
                       "mppi_nominal_and_gains_batch", "mppi_debug_nominal_and_gains_info",
                       "mppi_closed_loop_ticks_batch", "mppi_debug_closed_loop_info", "mppi_debug_closed_loop_check",
                       "mppi_set_plant_model", "mppi_debug_plant_model_info", "mppi_plant_drive_batch", "mppi_debug_plant_drive_info",
                       "mppi_debug_plant_drive_host", "mppi_closed_loop_sim_batch")

_lib = None


class MppiError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("mppi status %d: %s" % (status, msg))
        self.status = status


def lib():
    """Loads libmppi_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libmppi_hip.so is missing: run `python -m autorally_amd.build` "
                               "or __graft_entry__.build() first")
        L = C.CDLL(LIB_PATH)
        fp = C.POINTER(C.c_float)
        hp = C.c_void_p
        L.mppi_abi_version.restype = C.c_int
        L.mppi_strerror.restype = C.c_char_p
        L.mppi_strerror.argtypes = [C.c_int]
        L.mppi_last_error.restype = C.c_char_p
        L.mppi_last_error.argtypes = [hp]
        L.mppi_device_count.restype = C.c_int
        L.mppi_create.argtypes = [C.POINTER(Config), C.POINTER(hp)]
        L.mppi_destroy.argtypes = [hp]
        L.mppi_set_nn_params.argtypes = [hp, fp, C.c_size_t]
        L.mppi_update_model.argtypes = [hp, C.POINTER(C.c_int), C.c_int, fp, C.c_size_t]
        L.mppi_set_control_limits.argtypes = [hp, fp, fp]
        L.mppi_set_costmap.argtypes = [hp, C.c_int, C.c_int, fp, fp, fp, fp]
        L.mppi_set_costmap_transform.argtypes = [hp, fp, fp, fp]
        L.mppi_set_costmap_channel.argtypes = [hp, C.c_int, fp, C.c_size_t]
        L.mppi_set_cost_params.argtypes = [hp, C.POINTER(CostParams)]
        L.mppi_reset_controls.argtypes = [hp]
        L.mppi_set_control_seq.argtypes = [hp, fp, C.c_size_t]
        L.mppi_get_control_seq.argtypes = [hp, fp, C.c_size_t]
        L.mppi_set_control_hist.argtypes = [hp, fp]
        L.mppi_get_control_hist.argtypes = [hp, fp]
        L.mppi_slide_control_seq.argtypes = [hp, C.c_int]
        L.mppi_seed.argtypes = [hp, C.c_uint64, C.c_uint64]
        L.mppi_set_noise.argtypes = [hp, fp, C.c_size_t]
        L.mppi_generate_noise.argtypes = [hp, fp, C.c_size_t]
        L.mppi_compute_control.argtypes = [hp, fp]
        L.mppi_compute_control_async.argtypes = [hp, fp]
        L.mppi_control_ticks.argtypes = [hp, fp, C.c_int, C.c_int]
        L.mppi_synchronize.argtypes = [hp]
        L.mppi_get_results.argtypes = [hp, fp, fp, fp, fp]
        L.mppi_get_applied_controls.argtypes = [hp, fp, C.c_size_t]
        L.mppi_rollout_only.argtypes = [hp, fp, fp]
        L.mppi_nominal_traj.argtypes = [hp, fp, fp, fp]
        L.mppi_set_bf_params.argtypes = [hp, fp, C.c_size_t]
        L.mppi_debug_cost_raster.argtypes = [hp, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, C.c_int, fp, C.c_size_t]
        L.mppi_set_ddp_weights.argtypes = [hp, fp, fp, fp]
        L.mppi_compute_feedback_gains.argtypes = [hp, fp, fp, fp]
        L.mppi_get_feedback_gains.argtypes = [hp, fp, fp, fp, fp, fp]
        L.mppi_enable_stage_timing.argtypes = [hp, C.c_int]
        L.mppi_reset_stage_times.argtypes = [hp]
        L.mppi_get_stage_times.argtypes = [hp, C.POINTER(StageTimes)]
        L.mppi_rollout_variant.restype = C.c_char_p
        L.mppi_rollout_variant.argtypes = [hp]
        L.mppi_set_rollout_variant.argtypes = [hp, C.c_char_p]
        L.mppi_debug_dynamics.argtypes = [hp, C.c_int, fp, fp, fp]
        # symbols added with ABI version 2 (include/mppi_hip.h): an older library (kernel A/B through
        # MPPI_LIB_PATH) reports version 1 and lacks them
        v2 = L.mppi_abi_version() >= 2
        if v2:
            L.mppi_debug_inject_handover_fault.argtypes = [hp, C.c_int, C.c_int]
            L.mppi_savitsky_golay.argtypes = [hp]
            L.mppi_compute_control_batch_async.argtypes = [C.POINTER(hp), fp, C.c_int]
            L.mppi_compute_control_batch.argtypes = [C.POINTER(hp), fp, C.c_int]
            L.mppi_control_ticks_batch.argtypes = [C.POINTER(hp), fp, C.c_int, C.c_int, C.c_int]
            L.mppi_nominal_traj_pair.argtypes = [hp, fp, fp, fp, hp, fp, fp, fp]
        v3 = L.mppi_abi_version() >= 3
        if v3:
            L.mppi_compute_feedback_gains_pair.argtypes = [hp, fp, fp, fp, hp, fp, fp, fp]
            L.mppi_set_host_threads.argtypes = [C.c_int]
        v4 = L.mppi_abi_version() >= 4
        if v4:
            L.mppi_debug_capture_iterations.argtypes = [hp, C.c_int]
            L.mppi_debug_get_iterations.argtypes = [hp, fp, fp, fp]
            L.mppi_set_wait_timeout.argtypes = [hp, C.c_double]
            L.mppi_debug_form_candidates.argtypes = [hp, C.POINTER(C.c_char_p), C.c_int]
        v5 = L.mppi_abi_version() >= 5
        if v5:
            L.mppi_debug_set_chained_ticks.argtypes = [hp, C.c_int]
            L.mppi_debug_min_cost.argtypes = [hp, C.c_int, C.POINTER(C.c_int)]
            L.mppi_arm.argtypes = [hp, C.c_double]
            L.mppi_arm_batch.argtypes = [C.POINTER(hp), C.c_int, C.c_double]
            L.mppi_disarm.argtypes = [hp]
            L.mppi_is_armed.argtypes = [hp]
        if hasattr(L, "mppi_debug_launch_info"):  # added without a version step: an older version-5 library lacks it
            L.mppi_debug_launch_info.argtypes = [hp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        if hasattr(L, "mppi_trace_rollouts"):  # added without a version step, like mppi_debug_launch_info
            ip = C.POINTER(C.c_int)
            L.mppi_trace_rollouts.argtypes = [hp, ip, C.c_int, fp, fp, fp, fp, ip]
            L.mppi_top_rollouts.argtypes = [hp, C.c_int, ip]
        if hasattr(L, "mppi_compute_feedback_gains_batch"):  # added without a version step, like mppi_debug_launch_info
            fpp = C.POINTER(fp)
            L.mppi_compute_feedback_gains_batch.argtypes = [C.POINTER(hp), fp, fpp, fpp, C.c_int]
            L.mppi_debug_ddp_info.argtypes = [hp, C.POINTER(C.c_int)]
            L.mppi_debug_device_tanhf.argtypes = [C.c_int, fp, fp, C.c_size_t]
        if hasattr(L, "mppi_nominal_traj_batch"):  # added without a version step, like mppi_debug_launch_info
            fpp = C.POINTER(fp)
            L.mppi_nominal_traj_batch.argtypes = [C.POINTER(hp), fp, fpp, fpp, C.c_int]
            L.mppi_debug_nominal_info.argtypes = [hp, C.POINTER(C.c_int)]
        if hasattr(L, "mppi_nominal_and_gains_batch"):  # added without a version step, like mppi_debug_launch_info
            fpp = C.POINTER(fp)
            L.mppi_nominal_and_gains_batch.argtypes = [C.POINTER(hp), fp, fpp, fpp, C.c_int]
            L.mppi_debug_nominal_and_gains_info.argtypes = [hp, C.POINTER(C.c_int)]
        if hasattr(L, "mppi_closed_loop_ticks_batch"):  # added without a version step, like mppi_debug_launch_info
            ip, fpp = C.POINTER(C.c_int), C.POINTER(fp)
            L.mppi_closed_loop_ticks_batch.argtypes = [C.POINTER(hp), fp, C.c_int, C.c_int, C.c_int, fpp, fpp, fpp]
            L.mppi_debug_closed_loop_info.argtypes = [hp, ip, ip]
            L.mppi_debug_closed_loop_check.argtypes = [fp, fp, C.c_int, C.c_int, ip]
        if hasattr(L, "mppi_plant_drive_batch"):  # added without a version step, like mppi_debug_launch_info
            ip, fpp = C.POINTER(C.c_int), C.POINTER(fp)
            L.mppi_set_plant_model.argtypes = [hp, ip, C.c_int, fp, C.c_size_t, C.c_int]
            L.mppi_debug_plant_model_info.argtypes = [hp, ip]
            L.mppi_plant_drive_batch.argtypes = [C.POINTER(hp), fp, fpp, fpp, C.c_int, C.c_int, C.c_int, C.c_int, fp, fpp]
            L.mppi_debug_plant_drive_info.argtypes = [hp, ip]
            L.mppi_debug_plant_drive_host.argtypes = [ip, C.c_int, fp, C.c_size_t, C.c_int, C.c_float, fp, fp, fp, fp, fp, fp,
                                                      C.c_int, C.c_int, C.c_int, fp, fp]
            L.mppi_closed_loop_sim_batch.argtypes = [C.POINTER(hp), fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, fpp, fpp, fpp]
        if hasattr(L, "mppi_trace_rollouts_batch"):  # added without a version step, like mppi_debug_launch_info
            ip, fpp = C.POINTER(C.c_int), C.POINTER(fp)
            ipp = C.POINTER(ip)
            L.mppi_trace_rollouts_batch.argtypes = [C.POINTER(hp), C.c_int, ip, ipp, ipp, fpp, fpp, fpp, fpp, ipp]
            L.mppi_debug_trace_info.argtypes = [hp, C.POINTER(C.c_int)]
        for s in SYMBOLS:  # every declared symbol of the library's ABI version must be there
            if (v2 or s not in ABI2_SYMBOLS) and (v3 or s not in ABI3_SYMBOLS) and (v4 or s not in ABI4_SYMBOLS) and \
                    (v5 or s not in ABI5_SYMBOLS) and s not in UNVERSIONED_SYMBOLS:
                getattr(L, s)
        _lib = L
    return _lib


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float32)
    if shape is not None:
        a = a.reshape(shape)
    return a


def make_config_struct(cfg, device=0):
    c = Config()
    c.device = int(device)
    c.num_rollouts = int(cfg["K"])
    c.num_timesteps = int(cfg["T"])
    c.hz = int(cfg["hz"])
    c.optimization_stride = int(cfg["opt_stride"])
    c.gamma = float(cfg["gamma"])
    c.num_iters = int(cfg.get("num_iters", 1))
    # cfg["bf_W"] selects the GeneralizedLinear basis-function dynamics (n_layers = 0)
    layers = [] if cfg.get("bf_W") is not None else [int(x) for x in cfg["layers"]]
    c.n_layers = len(layers)
    for i, v in enumerate(layers):
        c.layers[i] = v
    for i in range(2):
        c.exploration_std[i] = float(cfg["nu"][i])
        c.init_control[i] = float(cfg["init_u"][i])
        c.control_min[i] = float(cfg["u_lo"][i])
        c.control_max[i] = float(cfg["u_hi"][i])
    c.negate_yaw_der = int(bool(cfg["negate_yaw_der"]))
    c.seed = int(cfg.get("seed", 1234))
    return c


def make_cost_struct(cost):
    p = CostParams()
    for n, _ in CostParams._fields_[:-1]:
        setattr(p, n, float(cost[n]))
    p.l1_cost = int(bool(cost.get("l1_cost", False)))
    return p


class Solver:
    """One mppi_handle: a thin object wrapper over the C ABI (method names follow the ABI)."""

    def __init__(self, cfg, device=0):
        self.L = lib()
        self.cfg = cfg
        self.K, self.T = int(cfg["K"]), int(cfg["T"])
        self.num_iters = int(cfg.get("num_iters", 1))
        self.h = C.c_void_p()
        c = make_config_struct(cfg, device)
        rc = self.L.mppi_create(C.byref(c), C.byref(self.h))
        if rc != OK:
            self.h = C.c_void_p()
            raise MppiError(rc, self.L.mppi_strerror(rc).decode())
        if cfg.get("bf_W") is not None:
            W = _f32(cfg["bf_W"], (4, 25))
            self._ck(self.L.mppi_set_bf_params(self.h, _fp(W), W.size))
        else:
            theta = _f32(cfg["theta"])
            self._ck(self.L.mppi_set_nn_params(self.h, _fp(theta), theta.size))
        m = _f32(cfg["map_rgba"])
        H, W = m.shape[0], m.shape[1]
        self._ck(self.L.mppi_set_costmap(self.h, W, H, _fp(m), _fp(_f32(cfg["r_c1"])),
                                         _fp(_f32(cfg["r_c2"])), _fp(_f32(cfg["trs"]))))
        p = make_cost_struct(cfg["cost"])
        self._ck(self.L.mppi_set_cost_params(self.h, C.byref(p)))

    def _ck(self, rc):
        if rc != OK:
            raise MppiError(rc, "%s (%s)" % (self.L.mppi_strerror(rc).decode(),
                                             self.L.mppi_last_error(self.h).decode()))

    def close(self):
        if self.h:
            self.L.mppi_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- setters / getters ---
    def set_cost_params(self, cost):
        p = make_cost_struct(cost)
        self._ck(self.L.mppi_set_cost_params(self.h, C.byref(p)))

    def set_control_limits(self, lo, hi):
        self._ck(self.L.mppi_set_control_limits(self.h, _fp(_f32(lo)), _fp(_f32(hi))))

    def set_control_seq(self, U):
        U = _f32(U)
        self._ck(self.L.mppi_set_control_seq(self.h, _fp(U), U.size))

    def get_control_seq(self):
        U = np.zeros((self.T, 2), dtype=np.float32)
        self._ck(self.L.mppi_get_control_seq(self.h, _fp(U), U.size))
        return U

    def reset_controls(self):
        self._ck(self.L.mppi_reset_controls(self.h))

    def set_control_hist(self, hist):
        self._ck(self.L.mppi_set_control_hist(self.h, _fp(_f32(hist, (4,)))))

    def get_control_hist(self):
        h = np.zeros(4, dtype=np.float32)
        self._ck(self.L.mppi_get_control_hist(self.h, _fp(h)))
        return h

    def savitsky_golay(self):
        self._ck(self.L.mppi_savitsky_golay(self.h))

    def slide_control_seq(self, stride):
        self._ck(self.L.mppi_slide_control_seq(self.h, int(stride)))

    def seed(self, seed, offset=0):
        self._ck(self.L.mppi_seed(self.h, int(seed), int(offset)))

    def set_noise(self, eps):
        eps = _f32(eps)
        self._ck(self.L.mppi_set_noise(self.h, _fp(eps), eps.size))

    def generate_noise(self):
        e = np.zeros((self.K, self.T, 2), dtype=np.float32)
        self._ck(self.L.mppi_generate_noise(self.h, _fp(e), e.size))
        return e

    def set_nn_params(self, theta):
        """mppi_set_nn_params: the packed [W1|b1|W2|b2|..] of the handle's layer list, live."""
        theta = _f32(theta)
        self._ck(self.L.mppi_set_nn_params(self.h, _fp(theta), theta.size))

    def update_model(self, description, data):
        d = (C.c_int * len(description))(*[int(x) for x in description])
        data = _f32(data)
        self._ck(self.L.mppi_update_model(self.h, d, len(description), _fp(data), data.size))

    def set_costmap_transform(self, r_c1, r_c2, trs):
        self._ck(self.L.mppi_set_costmap_transform(self.h, _fp(_f32(r_c1, (3,))), _fp(_f32(r_c2, (3,))), _fp(_f32(trs, (3,)))))

    def set_costmap_channel(self, channel, data):
        data = _f32(data)
        self._ck(self.L.mppi_set_costmap_channel(self.h, int(channel), _fp(data), data.size))

    # --- compute ---
    def compute_control(self, state):
        self._ck(self.L.mppi_compute_control(self.h, _fp(_f32(state, (7,)))))

    def bind_state(self, state):
        """Returns a zero-argument callable running mppi_compute_control on a fixed state buffer
        (skips the per-call numpy/ctypes marshalling; used by bench.py's timed loop)."""
        buf = _f32(state, (7,)).copy()
        ptr = _fp(buf)
        fn, h, ck = self.L.mppi_compute_control, self.h, self._ck

        def run(_keep=buf):
            ck(fn(h, ptr))
        return run

    def control_ticks(self, state, n_ticks, stride=1):
        """n_ticks x (compute_control + slide_control_seq(stride)) inside one library call."""
        self._ck(self.L.mppi_control_ticks(self.h, _fp(_f32(state, (7,))), int(n_ticks), int(stride)))

    def debug_set_chained_ticks(self, on):
        self._ck(self.L.mppi_debug_set_chained_ticks(self.h, int(on)))

    def debug_min_cost(self, on=-1):
        """Switch beta-from-the-rollout-kernel on / off (on < 0: leave it); returns whether the LAST solve's tail kernel used it."""
        got = C.c_int(0)
        self._ck(self.L.mppi_debug_min_cost(self.h, int(on), C.byref(got)))
        return bool(got.value)

    def arm(self, max_wait_s=0.01):
        """mppi_arm: enqueue the next solve now, gated; the next compute_control[_async] opens it with its state.
        Raises MppiError (status ERR_UNSUPPORTED) where the handle's form / configuration has no gated form."""
        self._ck(self.L.mppi_arm(self.h, float(max_wait_s)))

    def disarm(self):
        """mppi_disarm: call the armed solve off (never blocks on the GPU)."""
        self._ck(self.L.mppi_disarm(self.h))

    def is_armed(self):
        return bool(self.L.mppi_is_armed(self.h))

    def debug_launch_info(self):
        """mppi_debug_launch_info: (instances, gated) of the rollout launch of the most recently enqueued solve (an armed one
        counts): instances 0 before any solve, 1 for a launch of its own, n for one shared by the n handles of a batch."""
        n, g = C.c_int(-1), C.c_int(-1)
        self._ck(self.L.mppi_debug_launch_info(self.h, C.byref(n), C.byref(g)))
        return n.value, g.value

    def compute_control_async(self, state):
        self._ck(self.L.mppi_compute_control_async(self.h, _fp(_f32(state, (7,)))))

    def synchronize(self):
        self._ck(self.L.mppi_synchronize(self.h))

    def get_results(self, with_vectors=True):
        U = np.zeros((self.T, 2), dtype=np.float32)
        tc = C.c_float()
        costs = np.zeros(self.K, dtype=np.float32) if with_vectors else None
        w = np.zeros(self.K, dtype=np.float32) if with_vectors else None
        self._ck(self.L.mppi_get_results(self.h, _fp(U), C.byref(tc),
                                         _fp(costs) if with_vectors else None,
                                         _fp(w) if with_vectors else None))
        return dict(U=U, traj_cost=tc.value, costs=costs, w=w)

    def get_applied_controls(self):
        V = np.zeros((self.K, self.T, 2), dtype=np.float32)
        self._ck(self.L.mppi_get_applied_controls(self.h, _fp(V), V.size))
        return V

    def trace_rollouts(self, ks, with_costs=True):
        """mppi_trace_rollouts: the rollouts ks of the last solve replayed on the device.  dict(states [n, T, 7] before the
        update of step t, controls [n, T, 2] after the clamp, first_crash [n]; with_costs: step_costs [n, T], costs [n]).
        With a control cost on the cost outputs are refused (ERR_UNSUPPORTED): pass with_costs=False."""
        ks = np.ascontiguousarray(ks, dtype=np.int32).reshape(-1)
        n = ks.size
        out = dict(states=np.zeros((n, self.T, 7), np.float32), controls=np.zeros((n, self.T, 2), np.float32),
                   first_crash=np.zeros(n, np.int32))
        if with_costs:
            out.update(step_costs=np.zeros((n, self.T), np.float32), costs=np.zeros(n, np.float32))
        ip = C.POINTER(C.c_int)
        self._ck(self.L.mppi_trace_rollouts(self.h, ks.ctypes.data_as(ip), n, _fp(out["states"]), _fp(out["controls"]),
                                            _fp(out["step_costs"]) if with_costs else None,
                                            _fp(out["costs"]) if with_costs else None, out["first_crash"].ctypes.data_as(ip)))
        return out

    def top_rollouts(self, n):
        """mppi_top_rollouts: indices of the n largest weights of the last solve, descending, ties to the lower index."""
        ks = np.zeros(int(n), np.int32)
        self._ck(self.L.mppi_top_rollouts(self.h, int(n), ks.ctypes.data_as(C.POINTER(C.c_int))))
        return ks

    def debug_trace_info(self):
        """mppi_debug_trace_info: 1 if the handle's last trace ran in the fleet's kernels, 0 if in a launch of its own."""
        on = C.c_int(-1)
        self._ck(self.L.mppi_debug_trace_info(self.h, C.byref(on)))
        return on.value

    def rollout_only(self, state):
        costs = np.zeros(self.K, dtype=np.float32)
        self._ck(self.L.mppi_rollout_only(self.h, _fp(_f32(state, (7,))), _fp(costs)))
        return costs

    def nominal_traj(self, state):
        ss = np.zeros((self.T, 7), dtype=np.float32)
        cs = np.zeros((self.T, 2), dtype=np.float32)
        self._ck(self.L.mppi_nominal_traj(self.h, _fp(_f32(state, (7,))), _fp(ss), _fp(cs)))
        return ss, cs

    def debug_nominal_info(self):
        """mppi_debug_nominal_info: 1 if the handle's last nominal replay ran in the fleet's kernel, 0 if on the host."""
        on = C.c_int(-1)
        self._ck(self.L.mppi_debug_nominal_info(self.h, C.byref(on)))
        return on.value

    def debug_closed_loop_info(self):
        """mppi_debug_closed_loop_info: (on_device, ticks) of the handle's last closed_loop_ticks_batch -- 1 if its ticks were
        enqueued on the device with the plant step in plant_fleet_kernel, 0 if it ran the loop of public calls; the ticks completed."""
        on, ticks = C.c_int(-1), C.c_int(-1)
        self._ck(self.L.mppi_debug_closed_loop_info(self.h, C.byref(on), C.byref(ticks)))
        return on.value, ticks.value

    def set_plant_model(self, layers=None, theta=None, negate_yaw_der=False):
        """mppi_set_plant_model: the network of the handle's plant (plant_drive_batch, closed_loop_sim_batch); layers=None and
        theta=None clear it -- the plant is then the handle's own network."""
        if layers is None and theta is None:
            self._ck(self.L.mppi_set_plant_model(self.h, None, 0, None, 0, 0))
            return
        ls = np.ascontiguousarray(layers, dtype=np.int32).reshape(-1)
        th = _f32(theta).ravel()
        self._ck(self.L.mppi_set_plant_model(self.h, ls.ctypes.data_as(C.POINTER(C.c_int)), ls.size, _fp(th), th.size,
                                             int(bool(negate_yaw_der))))

    def debug_plant_model_info(self):
        """mppi_debug_plant_model_info: the layer count of the handle's plant model, 0 without one."""
        nl = C.c_int(-1)
        self._ck(self.L.mppi_debug_plant_model_info(self.h, C.byref(nl)))
        return nl.value

    def debug_plant_drive_info(self):
        """mppi_debug_plant_drive_info: 1 if the handle's last plant_drive_batch ran in plant_drive_fleet_kernel, 0 if in the host text."""
        on = C.c_int(-1)
        self._ck(self.L.mppi_debug_plant_drive_info(self.h, C.byref(on)))
        return on.value

    def debug_nominal_and_gains_info(self):
        """mppi_debug_nominal_and_gains_info: 1 if the handle's last nominal_and_gains_batch ran in the one kernel, 0 if as the two calls."""
        fused = C.c_int(-1)
        self._ck(self.L.mppi_debug_nominal_and_gains_info(self.h, C.byref(fused)))
        return fused.value

    def set_ddp_weights(self, Q, R, Qf):
        self._ck(self.L.mppi_set_ddp_weights(self.h, _fp(_f32(Q, (7,))), _fp(_f32(R, (2,))), _fp(_f32(Qf, (7,)))))

    def compute_feedback_gains(self, state, target_x=None, target_u=None):
        """computeFeedbackGains + getFeedbackGains: dict(feedback[T,2,7], feedforward[T,2], x, u, total_cost).
        Targets default to the nominal trajectory of the current control sequence from `state`."""
        tx = _fp(_f32(target_x, (self.T, 7))) if target_x is not None else None
        tu = _fp(_f32(target_u, (self.T, 2))) if target_u is not None else None
        self._ck(self.L.mppi_compute_feedback_gains(self.h, _fp(_f32(state, (7,))), tx, tu))
        return self.feedback_gains()

    def feedback_gains(self):
        """getFeedbackGains of the last successful computeFeedbackGains."""
        fb = np.zeros((self.T, 2, 7), dtype=np.float32)
        ff = np.zeros((self.T, 2), dtype=np.float32)
        x = np.zeros((self.T, 7), dtype=np.float32)
        u = np.zeros((self.T, 2), dtype=np.float32)
        tc = np.zeros(1, dtype=np.float32)
        self._ck(self.L.mppi_get_feedback_gains(self.h, _fp(fb), _fp(ff), _fp(x), _fp(u), _fp(tc)))
        return dict(feedback=fb, feedforward=ff, x=x, u=u, total_cost=float(tc[0]))

    def debug_ddp_info(self):
        """mppi_debug_ddp_info: 1 if the handle's last DDP pass ran in the fleet's kernel, 0 if on the host."""
        on = C.c_int(-1)
        self._ck(self.L.mppi_debug_ddp_info(self.h, C.byref(on)))
        return on.value

    def debug_cost_raster(self, x, y, heading, width_m=10, height_m=10, ppm=50):
        out = np.zeros((height_m * ppm, width_m * ppm), dtype=np.float32)
        self._ck(self.L.mppi_debug_cost_raster(self.h, x, y, heading, width_m, height_m, ppm, _fp(out), out.size))
        return out

    def debug_dynamics(self, states, controls):
        states = _f32(states).reshape(-1, 7)
        controls = _f32(controls).reshape(-1, 2)
        out = np.zeros_like(states)
        self._ck(self.L.mppi_debug_dynamics(self.h, states.shape[0], _fp(states), _fp(controls), _fp(out)))
        return out

    def debug_capture_iterations(self, on=1):
        self._ck(self.L.mppi_debug_capture_iterations(self.h, int(on)))

    def debug_get_iterations(self, with_V=False):
        """{"U_raw": [iters][T][2], "costs": [iters][K], "V": [iters][K][T][2] (explicit-noise solves, with_V)}"""
        it, K, T = int(self.cfg.get("num_iters", 1)), self.cfg["K"], self.cfg["T"]
        U = np.zeros((it, T, 2), np.float32)
        c = np.zeros((it, K), np.float32)
        V = np.zeros((it, K, T, 2), np.float32) if with_V else None
        self._ck(self.L.mppi_debug_get_iterations(self.h, _fp(U), _fp(c), _fp(V) if with_V else None))
        out = {"U_raw": U, "costs": c}
        if with_V:
            out["V"] = V
        return out

    def form_candidates(self):
        """Names of the kernel forms the selection table knows for this model (mppi_debug_form_candidates)."""
        buf = (C.c_char_p * 16)()
        n = self.L.mppi_debug_form_candidates(self.h, buf, 16)
        return [buf[i].decode() for i in range(n)]

    def set_wait_timeout(self, seconds):
        self._ck(self.L.mppi_set_wait_timeout(self.h, float(seconds)))

    def debug_inject_handover_fault(self, wave, spin_budget):
        self._ck(self.L.mppi_debug_inject_handover_fault(self.h, int(wave), int(spin_budget)))

    # --- measurement ---
    def enable_stage_timing(self, on=1):
        """on = 1: every solve, N > 1: every Nth solve, 0: off."""
        self._ck(self.L.mppi_enable_stage_timing(self.h, int(on)))

    def reset_stage_times(self):
        self._ck(self.L.mppi_reset_stage_times(self.h))

    def get_stage_times(self):
        st = StageTimes()
        self._ck(self.L.mppi_get_stage_times(self.h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in StageTimes._fields_}

    def rollout_variant(self):
        return self.L.mppi_rollout_variant(self.h).decode()

    def set_rollout_variant(self, name):
        self._ck(self.L.mppi_set_rollout_variant(self.h, name.encode()))


def compute_control_batch(solvers, states, blocking=True):
    """mppi_compute_control_batch[_async]: the solves of several Solver objects enqueued together (one launch of
    the quad kernel + one of the tail kernel where the library can batch them)."""
    n = len(solvers)
    hs = (C.c_void_p * n)(*[s.h for s in solvers])
    st = np.ascontiguousarray(np.stack([_f32(x, (7,)) for x in states]), dtype=np.float32)
    L = solvers[0].L
    fn = L.mppi_compute_control_batch if blocking else L.mppi_compute_control_batch_async
    rc = fn(hs, _fp(st), n)
    if rc != OK:
        msgs = [s.L.mppi_last_error(s.h).decode() for s in solvers]
        raise MppiError(rc, "; ".join(m for m in msgs if m))


def arm_batch(solvers, max_wait_s=0.01):
    """mppi_arm_batch: arm the solves of the next compute_control_batch(solvers, ...) -- one gated launch where the batch is
    one launch, else each solver on its own.  Raises MppiError (ERR_UNSUPPORTED) if a solver could not be armed."""
    n = len(solvers)
    hs = (C.c_void_p * n)(*[s.h for s in solvers])
    rc = solvers[0].L.mppi_arm_batch(hs, n, float(max_wait_s))
    if rc != OK:
        raise MppiError(rc, "; ".join(m for m in (s.L.mppi_last_error(s.h).decode() for s in solvers) if m))


def control_ticks_batch(solvers, states, n_ticks, stride=1):
    """mppi_control_ticks_batch: n_ticks x (batched solve + slide of every controller) inside one library call."""
    n = len(solvers)
    hs = (C.c_void_p * n)(*[s.h for s in solvers])
    st = np.ascontiguousarray(np.stack([_f32(x, (7,)) for x in states]), dtype=np.float32)
    rc = solvers[0].L.mppi_control_ticks_batch(hs, _fp(st), n, int(n_ticks), int(stride))
    if rc != OK:
        raise MppiError(rc, "; ".join(s.L.mppi_last_error(s.h).decode() for s in solvers))


def set_host_threads(n):
    """mppi_set_host_threads: 1 = the caller's thread only, 2 = one helper thread for the paired host work of a tick."""
    rc = lib().mppi_set_host_threads(int(n))
    if rc != OK:
        raise MppiError(rc, "mppi_set_host_threads(%d)" % n)


def compute_feedback_gains_pair(sol_a, state_a, sol_b, state_b, targets_a=None, targets_b=None):
    """mppi_compute_feedback_gains_pair; targets_x = (state_seq [T][7], control_seq [T][2]) or None (the handle's own
    nominal replay from state_x)."""
    def tp(t):
        if t is None:
            return None, None
        return _fp(_f32(t[0], (sol_a.T, 7))), _fp(_f32(t[1], (sol_a.T, 2)))
    ta, tb = tp(targets_a), tp(targets_b)
    rc = sol_a.L.mppi_compute_feedback_gains_pair(sol_a.h, _fp(_f32(state_a, (7,))), ta[0], ta[1],
                                                  sol_b.h, _fp(_f32(state_b, (7,))), tb[0], tb[1])
    if rc != OK:
        raise MppiError(rc, sol_a.L.mppi_last_error(sol_a.h).decode() + " | " + sol_b.L.mppi_last_error(sol_b.h).decode())


def compute_feedback_gains_batch(solvers, states, targets=None):
    """mppi_compute_feedback_gains_batch: the DDP passes of several Solver objects in one call (one launch per 64 where the library
    can share it).  targets: None, or one entry per solver -- (state_seq [T][7], control_seq [T][2]) or None (that handle's own
    nominal replay).  Raises MppiError with every handle's message; the results are read with Solver.feedback_gains()."""
    n = len(solvers)
    hs = (C.c_void_p * n)(*[s.h for s in solvers])
    st = np.ascontiguousarray(np.stack([_f32(x, (7,)) for x in states]), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    txp = tup = None
    keep = []
    if targets is not None:
        txp, tup = (fp * n)(), (fp * n)()
        for i, (s, t) in enumerate(zip(solvers, targets)):
            if t is None:
                continue
            keep.append((_f32(t[0], (s.T, 7)), _f32(t[1], (s.T, 2))))
            txp[i], tup[i] = _fp(keep[-1][0]), _fp(keep[-1][1])
    L = solvers[0].L
    rc = L.mppi_compute_feedback_gains_batch(hs, _fp(st), txp, tup, n)
    if rc != OK:
        raise MppiError(rc, "; ".join(m for m in (s.L.mppi_last_error(s.h).decode() for s in solvers) if m))


def device_tanhf(x, device=0):
    """mppi_debug_device_tanhf: the DDP kernel's tanhf of every element of x, computed on the device."""
    x = _f32(x).ravel()
    out = np.zeros_like(x)
    rc = lib().mppi_debug_device_tanhf(int(device), _fp(x), _fp(out), x.size)
    if rc != OK:
        raise MppiError(rc, "mppi_debug_device_tanhf")
    return out


def nominal_traj_batch(solvers, states):
    """mppi_nominal_traj_batch: the nominal replays of several Solver objects in one call (one launch per 64 where the library can
    share it).  Returns [(state_seq [T][7], control_seq [T][2])] in the solvers' order; raises MppiError with every handle's
    message (an empty fleet: MPPI_ERR_INVALID, as the library answers n < 1)."""
    n = len(solvers)
    if n < 1 or len(states) != n:
        raise MppiError(ERR_INVALID, "nominal_traj_batch: %d solvers, %d states" % (n, len(states)))
    hs = (C.c_void_p * n)(*[s.h for s in solvers])
    st = np.ascontiguousarray(np.stack([_f32(x, (7,)) for x in states]), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    out = [(np.zeros((s.T, 7), np.float32), np.zeros((s.T, 2), np.float32)) for s in solvers]
    ssp, csp = (fp * n)(*[_fp(o[0]) for o in out]), (fp * n)(*[_fp(o[1]) for o in out])
    rc = solvers[0].L.mppi_nominal_traj_batch(hs, _fp(st), ssp, csp, n)
    if rc != OK:
        raise MppiError(rc, "; ".join(m for m in (s.L.mppi_last_error(s.h).decode() for s in solvers) if m))
    return out


def closed_loop_ticks_batch(solvers, states, n_ticks, stride):
    """mppi_closed_loop_ticks_batch: n_ticks closed-loop ticks (solve, plant step with the handle's own model, slide) of several
    Solver objects in one call; on the device without collecting in between where the library can (Solver.debug_closed_loop_info).
    Returns [(states [n_ticks + 1][7], controls [n_ticks][stride][2], costs [n_ticks])] in the solvers' order; the last row of a
    solver's states is its final state.  Raises MppiError with every handle's message."""
    n = len(solvers)
    if n < 1 or len(states) != n:
        raise MppiError(ERR_INVALID, "closed_loop_ticks_batch: %d solvers, %d states" % (n, len(states)))
    hs = (C.c_void_p * n)(*[s.h for s in solvers])
    nt, sd = max(int(n_ticks), 0), max(int(stride), 0)
    fp = C.POINTER(C.c_float)
    st = np.ascontiguousarray(np.stack([_f32(x, (7,)) for x in states]), dtype=np.float32)
    out = [(np.zeros((nt + 1, 7), np.float32), np.zeros((nt, sd, 2), np.float32), np.zeros((nt,), np.float32)) for _ in solvers]
    xl, ul, cl = ((fp * n)(*[_fp(o[k]) for o in out]) for k in range(3))
    rc = solvers[0].L.mppi_closed_loop_ticks_batch(hs, _fp(st), n, int(n_ticks), int(stride), xl, ul, cl)
    if rc != OK:
        raise MppiError(rc, "; ".join(m for m in (s.L.mppi_last_error(s.h).decode() for s in solvers) if m))
    return out


def plant_drive_batch(solvers, states, seqs, periods, substeps, feedback=False, outputs=None):
    """mppi_plant_drive_batch: `periods` control periods of `substeps` plant steps of several Solver objects' plants
    (Solver.set_plant_model; else the solver's own network) under the drive law, in one call (one launch per 64 where the library
    can share it: Solver.debug_plant_drive_info).  seqs[i]: (state_seq [T][7], control_seq [T][2]) as the nominal calls deliver
    them; with feedback the gains are each solver's current DDP result.  Returns (states_out [n][7], [applied [periods *
    substeps][2]]); outputs: that pair to fill (a caller that checks what a refused call wrote).  Raises MppiError with every
    handle's message."""
    n = len(solvers)
    if n < 1 or len(states) != n or len(seqs) != n:
        raise MppiError(ERR_INVALID, "plant_drive_batch: %d solvers, %d states, %d sequences" % (n, len(states), len(seqs)))
    hs = (C.c_void_p * n)(*[s.h for s in solvers])
    st = np.ascontiguousarray(np.stack([_f32(x, (7,)) for x in states]), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    keep = [(_f32(x, (s.T, 7)), _f32(u, (s.T, 2))) for s, (x, u) in zip(solvers, seqs)]
    xsp, usp = (fp * n)(*[_fp(k[0]) for k in keep]), (fp * n)(*[_fp(k[1]) for k in keep])
    steps = max(int(periods), 0) * max(int(substeps), 0)
    if outputs is None:
        outputs = (np.zeros((n, 7), np.float32), [np.zeros((steps, 2), np.float32) for _ in solvers])
    app = (fp * n)(*[_fp(a) for a in outputs[1]])
    rc = solvers[0].L.mppi_plant_drive_batch(hs, _fp(st), xsp, usp, n, int(periods), int(substeps), int(bool(feedback)), _fp(outputs[0]), app)
    if rc != OK:
        raise MppiError(rc, "; ".join(m for m in (s.L.mppi_last_error(s.h).decode() for s in solvers) if m))
    return outputs


def debug_plant_drive_host(layers, theta, negate_yaw_der, dt, u_lo, u_hi, x, state_seq, control_seq, feedback, periods, substeps):
    """mppi_debug_plant_drive_host: the host text of the drive law for a network given by value: (state_out [7], applied
    [periods * substeps][2]).  feedback: [T][2][7] or None.  Needs no device."""
    ls = np.ascontiguousarray(layers, dtype=np.int32).reshape(-1)
    th = _f32(theta).ravel()
    us = _f32(control_seq)
    T = us.shape[0]
    us = us.reshape(T, 2)
    xs = _f32(state_seq, (T, 7)) if state_seq is not None else None
    K = _f32(feedback, (T, 2, 7)) if feedback is not None else None
    out = np.zeros(7, np.float32)
    app = np.zeros((max(int(periods), 0) * max(int(substeps), 0), 2), np.float32)
    rc = lib().mppi_debug_plant_drive_host(ls.ctypes.data_as(C.POINTER(C.c_int)), ls.size, _fp(th), th.size, int(bool(negate_yaw_der)),
                                           float(np.float32(dt)), _fp(_f32(u_lo, (2,))), _fp(_f32(u_hi, (2,))), _fp(_f32(x, (7,))),
                                           _fp(xs) if xs is not None else None, _fp(us), _fp(K) if K is not None else None, T,
                                           int(periods), int(substeps), _fp(out), _fp(app))
    if rc != OK:
        raise MppiError(rc, "mppi_debug_plant_drive_host")
    return out, app


def closed_loop_sim_batch(solvers, states, n_ticks, stride, substeps, feedback=False):
    """mppi_closed_loop_sim_batch: n_ticks closed-loop ticks of several Solver objects against their plants (Solver.set_plant_model)
    under the drive law -- solve, nominal replay (with the gains where feedback is on), `stride` periods of `substeps` plant steps,
    slide -- in one call; on the device without collecting in between where the library can (Solver.debug_closed_loop_info).
    Returns [(states [n_ticks + 1][7], controls [n_ticks][stride * substeps][2], costs [n_ticks])] in the solvers' order.  Raises
    MppiError with every handle's message."""
    n = len(solvers)
    if n < 1 or len(states) != n:
        raise MppiError(ERR_INVALID, "closed_loop_sim_batch: %d solvers, %d states" % (n, len(states)))
    hs = (C.c_void_p * n)(*[s.h for s in solvers])
    nt, per = max(int(n_ticks), 0), max(int(stride), 0) * max(int(substeps), 0)
    fp = C.POINTER(C.c_float)
    st = np.ascontiguousarray(np.stack([_f32(x, (7,)) for x in states]), dtype=np.float32)
    out = [(np.zeros((nt + 1, 7), np.float32), np.zeros((nt, per, 2), np.float32), np.zeros((nt,), np.float32)) for _ in solvers]
    xl, ul, cl = ((fp * n)(*[_fp(o[k]) for o in out]) for k in range(3))
    rc = solvers[0].L.mppi_closed_loop_sim_batch(hs, _fp(st), n, int(n_ticks), int(stride), int(substeps), int(bool(feedback)), xl, ul, cl)
    if rc != OK:
        raise MppiError(rc, "; ".join(m for m in (s.L.mppi_last_error(s.h).decode() for s in solvers) if m))
    return out


def debug_closed_loop_check(etas, controls, stride):
    """mppi_debug_closed_loop_check: the first tick of a device run's logs (etas [n_ticks], controls [n_ticks][stride][2]) whose eta
    is below 1 or not finite or whose controls are not finite; -1: none.  Needs no device."""
    etas = np.ascontiguousarray(etas, dtype=np.float32).ravel()
    controls = np.ascontiguousarray(controls, dtype=np.float32).ravel()
    if controls.size != etas.size * 2 * int(stride):
        raise MppiError(ERR_INVALID, "debug_closed_loop_check: controls must be [n_ticks][stride][2]")
    bad = C.c_int(-2)
    rc = lib().mppi_debug_closed_loop_check(_fp(etas), _fp(controls), etas.size, int(stride), C.byref(bad))
    if rc != OK:
        raise MppiError(rc, "mppi_debug_closed_loop_check")
    return bad.value


def nominal_and_gains_batch(solvers, states, outputs=None):
    """mppi_nominal_and_gains_batch: the nominal replays of several Solver objects and the DDP passes that track them in one call
    (one launch per 64 where the library can share it).  Returns [(state_seq [T][7], control_seq [T][2])] in the solvers' order; the
    gains are read with Solver.feedback_gains().  outputs: the arrays to fill (a caller that checks what a refused or a partly
    failed call wrote); raises MppiError with every handle's message (an empty fleet: MPPI_ERR_INVALID, as the library answers
    n < 1)."""
    n = len(solvers)
    if n < 1 or len(states) != n:
        raise MppiError(ERR_INVALID, "nominal_and_gains_batch: %d solvers, %d states" % (n, len(states)))
    hs = (C.c_void_p * n)(*[s.h for s in solvers])
    st = np.ascontiguousarray(np.stack([_f32(x, (7,)) for x in states]), dtype=np.float32)
    fp = C.POINTER(C.c_float)
    out = outputs if outputs is not None else [(np.zeros((s.T, 7), np.float32), np.zeros((s.T, 2), np.float32)) for s in solvers]
    ssp, csp = (fp * n)(*[_fp(o[0]) for o in out]), (fp * n)(*[_fp(o[1]) for o in out])
    rc = solvers[0].L.mppi_nominal_and_gains_batch(hs, _fp(st), ssp, csp, n)
    if rc != OK:
        raise MppiError(rc, "; ".join(m for m in (s.L.mppi_last_error(s.h).decode() for s in solvers) if m))
    return out


def trace_rollouts_batch(solvers, counts, ks=None, with_costs=True, outputs=None):
    """mppi_trace_rollouts_batch: the traces of several Solver objects in one call (one launch per 64 where the library can share
    it).  counts[i]: rollouts of solver i; ks: None, or one entry per solver -- its indices, or None for its counts[i] largest
    weights (mppi_top_rollouts' order).  Returns one dict per solver as Solver.trace_rollouts does, plus ks [counts[i]]: the
    indices that were traced.  outputs: the dicts to fill (a caller that checks what a refused call wrote); raises MppiError with
    every handle's message (an empty fleet: MPPI_ERR_INVALID, as the library answers n_handles < 1)."""
    n = len(solvers)
    if n < 1 or len(counts) != n or (ks is not None and len(ks) != n):
        raise MppiError(ERR_INVALID, "trace_rollouts_batch: %d solvers, %d counts" % (n, len(counts)))
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    cn = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
    if outputs is None:
        outputs = []
        for s, c in zip(solvers, cn):
            c = max(int(c), 0)
            o = dict(ks=np.zeros(c, np.int32), states=np.zeros((c, s.T, 7), np.float32), controls=np.zeros((c, s.T, 2), np.float32),
                     first_crash=np.zeros(c, np.int32))
            if with_costs:
                o.update(step_costs=np.zeros((c, s.T), np.float32), costs=np.zeros(c, np.float32))
            outputs.append(o)
    keep, ksp = [], None
    if ks is not None:
        ksp = (ip * n)()
        for i, k in enumerate(ks):
            if k is not None:
                keep.append(np.ascontiguousarray(k, dtype=np.int32).reshape(-1))
                ksp[i] = keep[-1].ctypes.data_as(ip)

    def arr(key, ptr):
        if key not in outputs[0]:
            return None
        return (ptr * n)(*[o[key].ctypes.data_as(ptr) for o in outputs])
    hs = (C.c_void_p * n)(*[s.h for s in solvers])
    rc = solvers[0].L.mppi_trace_rollouts_batch(hs, n, cn.ctypes.data_as(ip), ksp, arr("ks", ip), arr("states", fp), arr("controls", fp),
                                                arr("step_costs", fp), arr("costs", fp), arr("first_crash", ip))
    if rc != OK:
        raise MppiError(rc, "; ".join(m for m in (s.L.mppi_last_error(s.h).decode() for s in solvers) if m))
    return outputs


def nominal_traj_pair(sol_a, state_a, sol_b, state_b):
    """mppi_nominal_traj_pair: ((state_seq_a, control_seq_a), (state_seq_b, control_seq_b))."""
    out = []
    for s in (sol_a, sol_b):
        out.append((np.zeros((s.T, 7), np.float32), np.zeros((s.T, 2), np.float32)))
    rc = sol_a.L.mppi_nominal_traj_pair(sol_a.h, _fp(_f32(state_a, (7,))), _fp(out[0][0]), _fp(out[0][1]),
                                        sol_b.h, _fp(_f32(state_b, (7,))), _fp(out[1][0]), _fp(out[1][1]))
    if rc != OK:
        raise MppiError(rc, sol_a.L.mppi_last_error(sol_a.h).decode() + " | " + sol_b.L.mppi_last_error(sol_b.h).decode())
    return out

