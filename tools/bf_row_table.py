"""The "bf_row" form of the basis-function model beside "bf3" (DESIGN 4.15), both measured in this run on this box:
  1. rollout stage, K in {256, 1024, 2560, 4096, 8192, 16384}, T = 100: the kernel's own dispatch time (mppi_get_stage_times,
     every 2nd solve timed), median of 50 samples per form, the forms alternating in blocks inside one process;
  2. K = 2560: ms per tick with a new state every tick, as tools/tick_time.py measures them -- one handle fresh / armed, the
     pair fresh / armed (mppi_compute_control_batch, mppi_arm_batch); "bf3" has no gated form: its armed entries say so;
  3. the control loop of path_integral_bf (tools/loop_time.sh's row) as it is and with --rollout-variant bf_row --solve-ahead.
    python tools/bf_row_table.py [--k 256,2560] [--ticks 200] [--loop-iters 2000] [> profiles/<round>_bf_row_times.txt]
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autorally_amd import build as B  # noqa: E402
from autorally_amd import capi  # noqa: E402
from autorally_amd import params as P  # noqa: E402
from autorally_amd import synthetic as S  # noqa: E402

T = 100
KS = [256, 1024, 2560, 4096, 8192, 16384]
FORMS = ["bf3", "bf_row"]
BF_NPZ = os.path.join(ROOT, "autorally_amd", "data", "models", "basis_function_09_12_2018.npz")


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def sample(sol, st, every=2):
    sol.enable_stage_timing(every)
    sol.reset_stage_times()
    for _ in range(every):
        sol.compute_control(st)
        sol.slide_control_seq(1)
    t = sol.get_stage_times()
    sol.enable_stage_timing(0)
    return 1e3 * t["rollout_ms"] / max(1, t["n_solves"])


def rollout_table(bf_W, ks):
    print("rollout stage, T = %d, us (median of 50 samples, min .. max)" % T, flush=True)
    for K in ks:
        cfg = S.make_config(K, T, track="oval", bf_W=bf_W)
        st = cfg["start_state"]
        sols = {}
        for v in FORMS:
            sols[v] = capi.Solver(cfg)
            sols[v].set_rollout_variant(v)
            for _ in range(20):  # clocks up, code objects loaded, every buffer touched
                sols[v].compute_control(st)
        got = {v: [] for v in sols}
        for _ in range(5):
            for v, sol in sols.items():
                got[v] += [sample(sol, st) for _ in range(10)]
        line = ["K = %-6d" % K]
        for v, x in got.items():
            line.append("%s (%s) %.1f (%.1f .. %.1f)" % (v, sols[v].rollout_variant(), np.median(x), min(x), max(x)))
        line.append("bf3 / bf_row = %.2f" % (np.median(got["bf3"]) / np.median(got["bf_row"])))
        print("  ".join(line), flush=True)
        for sol in sols.values():
            sol.close()


def tick_table(bf_W, K, ticks, repeats=7, max_wait=0.01):
    """tools/tick_time.py's fresh / armed / batch_fresh / batch_armed on the basis-function model"""
    cfg = S.make_config(K, T, track="oval", bf_W=bf_W)
    opt = int(cfg["opt_stride"])
    st = cfg["start_state"]
    rec = capi.Solver(cfg)
    seq, s_ = [], st.copy()
    for _ in range(ticks):
        ss, _ = rec.nominal_traj(s_)
        seq.append(np.ascontiguousarray(np.stack([s_, ss[1]]), dtype=np.float32))
        rec.compute_control(s_)
        rec.slide_control_seq(opt)
        s_ = rec.nominal_traj(s_)[0][min(opt, T - 1)].copy()
    rec.close()
    fp = C.POINTER(C.c_float)
    ptrs = [x.ctypes.data_as(fp) for x in seq]
    L = capi.lib()
    print("ms per tick, K = %d, T = %d, a new state every tick, median of %d blocks of %d ticks (min .. max); [instances of the last "
          "rollout launch, gated]" % (K, T, repeats, ticks), flush=True)
    for v in FORMS:
        for mode in ("fresh", "armed", "batch_fresh", "batch_armed"):
            pair = mode.startswith("batch")
            sols = []
            for _ in range(2 if pair else 1):
                sols.append(capi.Solver(cfg))
                sols[-1].set_rollout_variant(v)
            hs = (C.c_void_p * len(sols))(*[x.h for x in sols])

            def ck(rc):
                if rc != capi.OK:
                    raise capi.MppiError(rc, L.mppi_last_error(sols[0].h).decode())

            def block():
                if not pair:
                    h = sols[0].h
                    ck(L.mppi_compute_control_async(h, ptrs[0]))
                    for i in range(1, ticks + 1):
                        if mode == "armed":
                            ck(L.mppi_arm(h, max_wait))
                        ck(L.mppi_synchronize(h))
                        ck(L.mppi_slide_control_seq(h, opt))
                        if i < ticks:
                            ck(L.mppi_compute_control_async(h, ptrs[i]))
                    if mode == "armed":
                        ck(L.mppi_disarm(h))
                else:
                    ck(L.mppi_compute_control_batch_async(hs, ptrs[0], 2))
                    for i in range(1, ticks + 1):
                        if mode == "batch_armed":
                            ck(L.mppi_arm_batch(hs, 2, max_wait))
                        for x in sols:
                            ck(L.mppi_synchronize(x.h))
                        for x in sols:
                            ck(L.mppi_slide_control_seq(x.h, opt))
                        if i < ticks:
                            ck(L.mppi_compute_control_batch_async(hs, ptrs[i], 2))
                    if mode == "batch_armed":
                        for x in sols:
                            ck(L.mppi_disarm(x.h))
            try:
                for _ in range(2):
                    block()
                ts = []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    block()
                    ts.append(1e3 * (time.perf_counter() - t0) / ticks)
                print("  %-7s %-12s %.4f (%.4f .. %.4f)  %s" % (v, mode, np.median(ts), min(ts), max(ts), list(sols[0].debug_launch_info())), flush=True)
            except capi.MppiError as e:
                if e.status != capi.ERR_UNSUPPORTED:
                    raise
                print("  %-7s %-12s no gated form (MPPI_ERR_UNSUPPORTED)" % (v, mode), flush=True)
            for s in sols:
                s.close()


def loop_rows(iters):
    """path_integral_bf's control loop (two controllers of K = 2560, self-simulation, no sleep) on the synthetic oval"""
    B.build_host()
    exe = os.path.join(ROOT, "autorally_amd", "bin", "path_integral_bf")
    launch = os.path.join(ROOT, "autorally_amd", "host", "launch", "path_integral_bf.launch")
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "models"))
        os.makedirs(os.path.join(d, "maps"))
        for f in os.listdir(S.MODELS_DIR):
            with open(os.path.join(S.MODELS_DIR, f), "rb") as src, open(os.path.join(d, "models", f), "wb") as dst:
                dst.write(src.read())
        ch0, xb, yb, ppm = S.oval_track_map()
        for m in ("ccrf_costmap_09_29_2017.npz", "marietta_costmap_09_08_2018.npz"):
            P.save_costmap_npz(os.path.join(d, "maps", m), ch0, xb, yb, ppm)
        env = dict(os.environ, AR_MPPI_PARAMS_PATH=d)
        base = [exe, launch, "--rollouts", "2560", "--max-iter", str(iters), "--no-sleep", "--set", "x_pos=0.0", "--set", "y_pos=-10.0",
                "--set", "heading=0.0", "--set", "use_feedback_gains=false"]
        for extra in ([], ["--rollout-variant", "bf_row"], ["--rollout-variant", "bf_row", "--solve-ahead"]):
            r = subprocess.run(base + extra, env=env, capture_output=True, text=True, timeout=300)
            last = r.stdout.strip().split("\n")[-1] if r.stdout.strip() else r.stderr[-300:]
            print("path_integral_bf K=2560 use_feedback_gains=false %s (exit %d)\n  %s" % (" ".join(extra), r.returncode, last[:330]), flush=True)


def main():
    B.build()
    bf_W = P.load_bf_npz(BF_NPZ)
    ks = [int(x) for x in arg("--k", ",".join(map(str, KS))).split(",")]
    rollout_table(bf_W, ks)
    tick_table(bf_W, 2560, int(arg("--ticks", "200")))
    loop_rows(int(arg("--loop-iters", "2000")))


if __name__ == "__main__":
    main()
