#!/usr/bin/env python3
"""tools/tick_time.py: what the two controllers of runControlLoop (run_control_loop.cuh:218-219; K = 1920 each by
default, the reference's rollout count) cost per tick on this GPU:
  one     -- one controller alone: solve + slide
  streams -- both controllers, each solve on its own handle's stream, enqueued before either is waited for (round 2)
  batch   -- both controllers in one launch (mppi_compute_control_batch)
and with a DIFFERENT state every tick (the nominal trajectory's state at the optimization stride, recorded once beforehand,
fed through the per-tick calls a control loop makes: compute_async -> [arm] -> synchronize -> slide):
  fresh        -- one controller, unarmed
  armed        -- one controller, its next solve armed (mppi_arm) while this one runs
  batch_fresh  -- both controllers in one launch, unarmed (the predicted state: the actual one's nominal state one step on)
  batch_armed  -- both controllers, the next pair armed in one gated launch (mppi_arm_batch)
Times are per tick (both solves + both slides), median of --repeats blocks of --ticks ticks, inside one library call
per block where the library has one (one, batch).
The network is the shipped 6-32-32-4 model, or --model FILE.npz (e.g. tests/golden/models/wider_deeper_network_08_20_2020.npz),
or a synthetic model of --layers 6,64,64,4; --variant forces a rollout form by name (e.g. lds44) on every handle.  Every mode's
entry says how many instances its last rollout launch served (mppi_debug_launch_info): 2 where the pair shared a launch."""
import ctypes as C
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autorally_amd import capi, params as P, synthetic as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=int, default=1920)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--modes", type=str, default="one,streams,batch")
    ap.add_argument("--max-wait", type=float, default=0.01, help="armed modes: mppi_arm's max_wait_s")
    ap.add_argument("--layers", type=str, default=None, help="a synthetic model of this layer list, e.g. 6,64,64,4")
    ap.add_argument("--model", type=str, default=None, help="a model file (.npz) instead of the shipped 6-32-32-4 one")
    ap.add_argument("--variant", type=str, default=None, help="rollout form forced by name on every handle, e.g. lds44")
    a = ap.parse_args()
    if a.model:
        layers, theta = P.load_model_npz(a.model)
        cfg = S.make_config(a.K, a.T, layers=list(layers), theta=theta, track="oval")
    elif a.layers:
        cfg = S.make_config(a.K, a.T, layers=[int(x) for x in a.layers.split(",")], track="oval")
    else:
        cfg = S.make_config(a.K, a.T, track="oval")

    def solver():
        s = capi.Solver(cfg)
        if a.variant:
            s.set_rollout_variant(a.variant)
        return s
    st = cfg["start_state"]
    st2 = st.copy()
    st2[0] += 0.3
    out = {"K": a.K, "T": a.T, "ticks": a.ticks, "layers": list(cfg["layers"])}
    opt = int(cfg["opt_stride"])
    # the states of a control loop: each tick's state is the nominal trajectory's state at the optimization stride of the
    # tick before (recorded once; the timed blocks feed them again and again)
    rec = solver()
    seq, s_ = [], st.copy()
    for _ in range(a.ticks):
        ss, _ = rec.nominal_traj(s_)
        seq.append(np.ascontiguousarray(np.stack([s_, ss[1]]), dtype=np.float32))
        rec.compute_control(s_)
        rec.slide_control_seq(opt)
        s_ = rec.nominal_traj(s_)[0][min(opt, a.T - 1)].copy()
    rec.close()
    fp = C.POINTER(C.c_float)
    ptrs = [x.ctypes.data_as(fp) for x in seq]
    L = capi.lib()
    for mode in a.modes.split(","):
        sols = [solver() for _ in range(1 if mode in ("one", "fresh", "armed") else 2)]
        hs = (C.c_void_p * len(sols))(*[x.h for x in sols])

        def ck(rc):
            if rc != capi.OK:
                raise capi.MppiError(rc, L.mppi_last_error(sols[0].h).decode())

        def block():
            if mode in ("fresh", "armed"):
                h = sols[0].h
                ck(L.mppi_compute_control_async(h, ptrs[0]))
                for i in range(1, a.ticks + 1):
                    if mode == "armed":
                        ck(L.mppi_arm(h, a.max_wait))
                    ck(L.mppi_synchronize(h))
                    ck(L.mppi_slide_control_seq(h, opt))
                    if i < a.ticks:
                        ck(L.mppi_compute_control_async(h, ptrs[i]))
                if mode == "armed":
                    ck(L.mppi_disarm(h))
            elif mode in ("batch_fresh", "batch_armed"):
                ck(L.mppi_compute_control_batch_async(hs, ptrs[0], 2))
                for i in range(1, a.ticks + 1):
                    if mode == "batch_armed":
                        ck(L.mppi_arm_batch(hs, 2, a.max_wait))
                    for x in sols:
                        ck(L.mppi_synchronize(x.h))
                    for x in sols:
                        ck(L.mppi_slide_control_seq(x.h, opt))
                    if i < a.ticks:
                        ck(L.mppi_compute_control_batch_async(hs, ptrs[i], 2))
                if mode == "batch_armed":
                    ck(L.mppi_disarm(sols[0].h))
            elif mode == "one":
                sols[0].control_ticks(st, a.ticks, 1)
            elif mode == "batch":
                capi.control_ticks_batch(sols, [st, st2], a.ticks, 1)
            else:
                for _ in range(a.ticks):
                    sols[0].compute_control_async(st)
                    sols[1].compute_control_async(st2)
                    sols[0].synchronize()
                    sols[1].synchronize()
                    sols[0].slide_control_seq(1)
                    sols[1].slide_control_seq(1)
        for _ in range(3):
            block()
        ts = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            block()
            ts.append(1e3 * (time.perf_counter() - t0) / a.ticks)
        out[mode] = {"ms_per_tick_median": float(np.median(ts)), "min": float(min(ts)), "max": float(max(ts)),
                     "variant": sols[0].rollout_variant(), "launch_instances": sols[0].debug_launch_info()[0]}
        if mode in ("armed", "batch_armed"):  # the armed path ran (every compute opened a gate): same results as unarmed
            out[mode]["U0"] = float(sols[0].get_control_seq()[0, 0])
        elif mode in ("fresh", "batch_fresh"):
            out[mode]["U0"] = float(sols[0].get_control_seq()[0, 0])
        for s in sols:
            s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
