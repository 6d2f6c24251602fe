"""Tick time of a fleet of controllers on one GPU: the "fleet16" rollout form (one generator, one rollout and one tail launch per
tick for the whole fleet) against the same handles solved one by one.

    python tools/fleet_time.py [--n 16] [--K 1920] [--T 100] [--ticks 200] [--warm 20] [--ways abc] [--net 6-32-32-4 ...]

n distinct oval instances with generator noise; the median wall time of a tick (mppi_control_ticks_batch, one tick, stride 1) over
`ticks` ticks after `warm` warm ones, three ways: (a) every handle forced to "fleet16"; (b) forced to "lds16" -- the same
wavefront, handle by handle; (c) "auto" (row_tree / m44, handle by handle).  Prints one line per network and a JSON line.

With "d" among --ways: (d) every handle forced to "fleet_multi4" -- the register MFMA group of "multi4_tree_gen" as a fleet form
(6-32x2-4, 6-32x4-4 and 6-64x2-4; any other list: not available) -- and with "A": "fleet16" a second time, the A/A spread of the
visit beside the ratios (--ways dabcA).

    python tools/fleet_time.py --model bf [--n 16] [--K 2560] [--T 100] [--ticks 200] [--warm 20] [--ways f123cF]

The basis-function model (the golden W of tests/golden/models) instead of a network: (f) every handle forced to "fleet_bf" -- the
model's own workgroups as a fleet form, the wave count per 64 rollouts chosen by fleet_bf_plan --, (1) (2) (3) "fleet_bf_w1" /
"_w2" / "_w3", that count forced, (c) "auto" (up to 4 handles in one launch of the three-wave kernel, beyond that handle by
handle), (F) "fleet_bf" a second time: the A/A spread of the visit; and, handle by handle, the single-handle forms the wave
counts match: (p) "fused" (one wave), (q) "quad" (two), (r) "bf3" (three).

    python tools/fleet_time.py --ddp [--T 100] [--ticks 200] [--net ...]

The DDP feedback gains of the fleet instead (n = 2, 4, 16, 64): mppi_compute_feedback_gains_batch -- one launch of ddp_fleet_kernel --
against n single calls on one host thread and against the pair entry with mppi_set_host_threads(2); median of `ticks` calls.

    python tools/fleet_time.py --nominal [--T 100] [--ticks 200] [--net ...]

The nominal trajectories of the fleet (n = 2, 4, 16, 64): mppi_nominal_traj_batch -- one launch of nominal_fleet_kernel -- against
n mppi_nominal_traj calls on one host thread and n / 2 mppi_nominal_traj_pair calls with mppi_set_host_threads(2).

    python tools/fleet_time.py --finish [--n 2 4 16 64] [--T 100] [--ticks 200] [--net ...]

The two closing stages of the fleet's tick (n = 2, 4, 16, 64): mppi_nominal_and_gains_batch -- one launch of
nominal_gains_fleet_kernel -- against mppi_nominal_traj_batch followed by mppi_compute_feedback_gains_batch on its outputs, the two
sides alternating call by call within the run; both sides fill the same caller buffers, as the host layer's state_solution_ /
control_solution_ are filled, so each includes the copies between those buffers and the staging memory.  The kernel times come from a
run of their own:  rocprofv3 --kernel-trace --stats -- python tools/fleet_time.py --finish --n 64 --ticks 20

    python tools/fleet_time.py --mixed 6-32-32-4 6-64-64-64-64-4 6-129-4 6-256-256-4 [--n 4 16 64] [--K 1920] [--T 100] [--ways abcdA]

A fleet whose handles cycle through the given layer lists (handle i has list i mod the number of lists), one row per n, every
column of a row in one process: (a) every handle forced to "fleet_glb16" -- one launch for the mixed fleet --, (b) the same handles
forced to "glb16", handle by handle, (c) "auto", (d) "fleet16" (one list of hidden widths up to 128 only; else not available),
(A) "fleet_glb16" a second time: the A/A spread of the visit.

    python tools/fleet_time.py --trace [--n 4 16 64] [--K 1920] [--T 100] [--ticks 100] [--net ...]

The 64 best sampled trajectories of every handle of a solved fleet: mppi_trace_rollouts_batch -- the largest weights chosen on the
device, one trace launch, one result copy -- against the same handles one by one (mppi_top_rollouts + mppi_trace_rollouts); the
batch entry is timed twice, interleaved with the per-handle calls: the A/A spread of the visit.

    python tools/fleet_time.py --closed-loop [--n 64] [--K 1920] [--T 100] [--ticks 200] [--net ...] [--variant fleet_multi4]

Closed-loop ticks of the fleet (solve, plant step, slide): mppi_closed_loop_ticks_batch with all ticks enqueued on the device against
(r) the reference loop inside the library (the same entry with MPPI_CLOSED_LOOP_DEVICE=0) and (p) the reference loop driven from
Python; every run from the same start (controls reset, generator reseeded), the ways alternating, the median of three runs each.

    python tools/fleet_time.py --closed-loop-sim [--n 64] [--K 1920] [--T 100] [--ticks 100] [--net ...] [--variant fleet_multi4]

Closed-loop ticks against a plant of its own (the controller's weights scaled by 1.05) under the drive law: for m in {1, 4} and
feedback off / on, mppi_closed_loop_sim_batch's first way (the device loop where it has one) against the loop of public calls inside
the library (MPPI_CLOSED_LOOP_DEVICE=0), alternating in one process, the median of three runs each.

    python tools/fleet_time.py --plant-drive [--n 64] [--T 100] [--ticks 200] [--net ...]

mppi_plant_drive_batch with feedback, the plant's image copied to LDS against the image read from global memory
(MPPI_PLANT_DRIVE_LDS = 1 / 0), alternating call by call, for one step, one period of four and two periods of four."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WAYS = (("d", "fleet_multi4"), ("a", "fleet16"), ("b", "lds16"), ("c", "auto"), ("A", "fleet16"))
BF_WAYS = (("f", "fleet_bf"), ("1", "fleet_bf_w1"), ("2", "fleet_bf_w2"), ("3", "fleet_bf_w3"), ("c", "auto"), ("F", "fleet_bf"),
           ("p", "fused"), ("q", "quad"), ("r", "bf3"))
MIXED_WAYS = (("a", "fleet_glb16"), ("b", "glb16"), ("c", "auto"), ("d", "fleet16"), ("A", "fleet_glb16"))
BF = "bf"  # in place of a layer list: the basis-function model


def bf_W():
    from autorally_amd import params as P
    return P.load_bf_npz(os.path.join(ROOT, "tests", "golden", "models", "basis_function_09_12_2018.npz"))


def fleet(net, variant, n, K, T):
    """n solvers on n distinct oval instances (one map: the instances differ in the start state, the model's scale, the cost
    parameters and the seed), forced to `variant`, and their states.  net: one layer list, BF, or a tuple of layer lists the
    handles cycle through (--mixed)."""
    from autorally_amd import capi
    from autorally_amd import synthetic as S
    mixed = net != BF and isinstance(net[0], (list, tuple))
    if net == BF:
        bases = [S.make_config(K, T, track="oval", opt_stride=1, bf_W=bf_W())]
    else:
        bases = [S.make_config(K, T, layers=list(l), track="oval", opt_stride=1) for l in (net if mixed else [net])]
    sols, states = [], []
    for i in range(n):
        base = bases[i % len(bases)]
        st = np.array(base["start_state"], np.float32)
        st[0] += np.float32(0.4 * i)
        st[4] += np.float32(0.1 * (i % 5))
        cfg = dict(base, cost=dict(base["cost"], desired_speed=6.0 + 0.25 * i), start_state=st)
        if net == BF:
            cfg["bf_W"] = np.asarray(base["bf_W"], np.float32) * np.float32(1.0 + 0.005 * i)
        else:
            cfg["theta"] = np.asarray(base["theta"], np.float32) * np.float32(1.0 + 0.005 * i)
        sol = capi.Solver(cfg)
        if variant != "auto":
            try:
                sol.set_rollout_variant(variant)
            except capi.MppiError:
                for s in sols + [sol]:
                    s.close()
                raise
        sol.seed(1000 + i, 0)
        sols.append(sol)
        states.append(st)
    return sols, states


def tick_ms(net, variant, n=16, K=1920, T=100, ticks=200, warm=20):
    """-> (median ms per tick, instances per rollout launch, the form's name)"""
    from autorally_amd import capi
    try:
        sols, states = fleet(net, variant, n, K, T)
    except capi.MppiError as e:
        if e.status != capi.ERR_UNSUPPORTED:
            raise
        return None, 0, "not available"  # a list the form does not take ("fleet_multi4")
    try:
        capi.control_ticks_batch(sols, states, warm, 1)
        dt = []
        for _ in range(ticks):
            t0 = time.perf_counter()
            capi.control_ticks_batch(sols, states, 1, 1)
            dt.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(dt)), sols[0].debug_launch_info()[0], sols[0].rollout_variant()
    finally:
        for s in sols:
            s.close()


def table(nets, n=16, K=1920, T=100, ticks=200, warm=20, ways="abc"):
    rows = []
    for net in nets:
        row = {"net": "-".join(map(str, net)), "n": n, "K": K, "T": T}
        for key, variant in WAYS:
            if key not in ways:
                continue
            ms, inst, name = tick_ms(net, variant, n, K, T, ticks, warm)
            row[key + "_ms"], row[key + "_instances"], row[key + "_form"] = ms, inst, name
        rows.append(row)
        if set(ways) != set("abc"):
            print("FLEET n=%d K=%d T=%d net=%s: %s" % (n, K, T, row["net"], "  ".join(
                "(%s) %s %s [%d per launch]" % (key, variant, "n/a" if row[key + "_ms"] is None else "%.4f ms" % row[key + "_ms"], row[key + "_instances"])
                for key, variant in WAYS if key + "_ms" in row)), flush=True)
            continue
        print("FLEET n=%d K=%d T=%d net=%s: (a) fleet16 %.4f ms [%d per launch]  (b) lds16 %.4f ms  (c) auto (%s) %.4f ms;  b/a %.2f  c/a %.2f" % (
            n, K, T, row["net"], row["a_ms"], row["a_instances"], row["b_ms"], row["c_form"], row["c_ms"], row["b_ms"] / row["a_ms"],
            row["c_ms"] / row["a_ms"]), flush=True)
    return rows


def mixed_table(nets, ns=(4, 16, 64), K=1920, T=100, ticks=200, warm=20, ways="abcdA"):
    """One row per fleet size for handles that cycle through `nets`: every way of MIXED_WAYS named in `ways`, in one process."""
    rows = []
    for n in ns:
        row = {"nets": ["-".join(map(str, l)) for l in nets], "n": n, "K": K, "T": T}
        for key, variant in MIXED_WAYS:
            if key not in ways:
                continue
            if variant == "fleet16" and len(nets) != 1:  # a form of one layer list
                ms, inst, name = None, 0, "not available"
            else:
                ms, inst, name = tick_ms(tuple(tuple(l) for l in nets), variant, n, K, T, ticks, warm)
            row[key + "_ms"], row[key + "_instances"], row[key + "_form"] = ms, inst, name
        rows.append(row)
        print("FLEET MIXED n=%d K=%d T=%d nets=%s: %s" % (n, K, T, ",".join(row["nets"]), "  ".join(
            "(%s) %s %s [%d per launch]" % (key, variant, "n/a" if row[key + "_ms"] is None else "%.4f ms" % row[key + "_ms"], row[key + "_instances"])
            for key, variant in MIXED_WAYS if key + "_ms" in row)), flush=True)
    return rows


def table_bf(n=16, K=2560, T=100, ticks=200, warm=20, ways="f123cF"):
    """One row for the basis-function model: every way of BF_WAYS named in `ways`, in BF_WAYS' order, in one process."""
    row = {"net": BF, "n": n, "K": K, "T": T}
    for key, variant in BF_WAYS:
        if key not in ways:
            continue
        ms, inst, name = tick_ms(BF, variant, n, K, T, ticks, warm)
        row[key + "_ms"], row[key + "_instances"], row[key + "_form"] = ms, inst, name
    print("FLEET n=%d K=%d T=%d model=bf: %s" % (n, K, T, "  ".join(
        "(%s) %s %.4f ms [%s, %d per launch]" % (key, variant, row[key + "_ms"], row[key + "_form"], row[key + "_instances"])
        for key, variant in BF_WAYS if key + "_ms" in row)), flush=True)
    return [row]


def ddp_ms(net, n, K=64, T=100, calls=200, warm=10):
    """The DDP feedback gains of n handles, three ways, each the median wall time of `calls` calls after `warm` warm ones: the batch
    entry (one launch for the fleet), n single calls on one host thread, n / 2 pair calls with mppi_set_host_threads(2).  Every way
    tracks the same given targets (each handle's nominal trajectory), so the time is the DDP pass's alone."""
    from autorally_amd import capi
    sols, states = fleet(net, "auto", n, K, T)
    try:
        targets = [s.nominal_traj(st) for s, st in zip(sols, states)]

        def median(fn):
            for _ in range(warm):
                fn()
            dt = []
            for _ in range(calls):
                t0 = time.perf_counter()
                fn()
                dt.append(time.perf_counter() - t0)
            return 1e3 * float(np.median(dt))

        def single():
            for s, st, (tx, tu) in zip(sols, states, targets):
                s.L.mppi_compute_feedback_gains(s.h, capi._fp(st), capi._fp(tx), capi._fp(tu))

        def pairs():
            for i in range(0, n - 1, 2):
                capi.compute_feedback_gains_pair(sols[i], states[i], sols[i + 1], states[i + 1], targets[i], targets[i + 1])
            if n % 2:
                sols[-1].L.mppi_compute_feedback_gains(sols[-1].h, capi._fp(states[-1]), capi._fp(targets[-1][0]), capi._fp(targets[-1][1]))

        row = {"net": "-".join(map(str, net)), "n": n, "T": T}
        row["batch_ms"] = median(lambda: capi.compute_feedback_gains_batch(sols, states, targets))
        row["on_device"] = sols[0].debug_ddp_info()
        capi.set_host_threads(1)
        row["host1_ms"] = median(single)
        capi.set_host_threads(2)
        try:
            row["host2_ms"] = median(pairs)
        finally:
            capi.set_host_threads(1)
        return row
    finally:
        for s in sols:
            s.close()


def ddp_table(nets, ns=(2, 4, 16, 64), T=100, calls=200):
    rows = []
    for net in nets:
        for n in ns:
            row = ddp_ms(net, n, T=T, calls=calls)
            rows.append(row)
            print("FLEET DDP n=%d T=%d net=%s: batch %.4f ms (on_device %d)  host, 1 thread %.4f ms  host, 2 threads (pairs) %.4f ms;  "
                  "host1/batch %.2f  host2/batch %.2f" % (n, T, row["net"], row["batch_ms"], row["on_device"], row["host1_ms"],
                                                         row["host2_ms"], row["host1_ms"] / row["batch_ms"], row["host2_ms"] / row["batch_ms"]),
                  flush=True)
    return rows


def nominal_ms(net, n, K=64, T=100, calls=200, warm=10):
    """The nominal replays of n handles, three ways, each the median wall time of `calls` calls after `warm` warm ones: the batch
    entry (one launch for the fleet), n single calls on one host thread, n / 2 pair calls with mppi_set_host_threads(2).  Every
    handle replays a warm control sequence from its own state into buffers allocated once."""
    from autorally_amd import capi
    sols, states = fleet(net, "auto", n, K, T)
    try:
        rng = np.random.RandomState(5)
        for s in sols:
            s.set_control_seq(np.stack([rng.uniform(-0.5, 0.5, T), rng.uniform(-0.2, 0.6, T)], axis=1).astype(np.float32))
        out = [(np.zeros((T, 7), np.float32), np.zeros((T, 2), np.float32)) for _ in sols]
        fp = capi.C.POINTER(capi.C.c_float)
        hs = (capi.C.c_void_p * n)(*[s.h for s in sols])
        st = np.ascontiguousarray(np.stack(states), np.float32)
        ssp, csp = (fp * n)(*[capi._fp(o[0]) for o in out]), (fp * n)(*[capi._fp(o[1]) for o in out])
        L = sols[0].L

        def median(fn):
            for _ in range(warm):
                fn()
            dt = []
            for _ in range(calls):
                t0 = time.perf_counter()
                fn()
                dt.append(time.perf_counter() - t0)
            return 1e3 * float(np.median(dt))

        def batch():
            assert L.mppi_nominal_traj_batch(hs, capi._fp(st), ssp, csp, n) == capi.OK

        def single():
            for s, x, o in zip(sols, states, out):
                assert L.mppi_nominal_traj(s.h, capi._fp(x), capi._fp(o[0]), capi._fp(o[1])) == capi.OK

        def pairs():
            for i in range(0, n - 1, 2):
                assert L.mppi_nominal_traj_pair(sols[i].h, capi._fp(states[i]), capi._fp(out[i][0]), capi._fp(out[i][1]), sols[i + 1].h,
                                                capi._fp(states[i + 1]), capi._fp(out[i + 1][0]), capi._fp(out[i + 1][1])) == capi.OK
            if n % 2:
                assert L.mppi_nominal_traj(sols[-1].h, capi._fp(states[-1]), capi._fp(out[-1][0]), capi._fp(out[-1][1])) == capi.OK

        row = {"net": "-".join(map(str, net)), "n": n, "T": T}
        row["batch_ms"] = median(batch)
        row["on_device"] = sols[0].debug_nominal_info()
        capi.set_host_threads(1)
        row["host1_ms"] = median(single)
        capi.set_host_threads(2)
        try:
            row["host2_ms"] = median(pairs)
        finally:
            capi.set_host_threads(1)
        return row
    finally:
        for s in sols:
            s.close()


def nominal_table(nets, ns=(2, 4, 16, 64), T=100, calls=200):
    rows = []
    for net in nets:
        for n in ns:
            row = nominal_ms(net, n, T=T, calls=calls)
            rows.append(row)
            print("FLEET NOMINAL n=%d T=%d net=%s: batch %.4f ms (on_device %d)  host, 1 thread %.4f ms  host, 2 threads (pairs) %.4f ms;  "
                  "host1/batch %.2f  host2/batch %.2f" % (n, T, row["net"], row["batch_ms"], row["on_device"], row["host1_ms"],
                                                         row["host2_ms"], row["host1_ms"] / row["batch_ms"], row["host2_ms"] / row["batch_ms"]),
                  flush=True)
    return rows


def finish_ms(net, n, K=64, T=100, calls=200, warm=10):
    """The closing stages of n handles' tick, two ways, each the median wall time of `calls` calls after `warm` warm ones, the two
    alternating call by call: the fused entry (one launch for the fleet), and the batched replay followed by the batched DDP pass
    that tracks its outputs.  Every handle replays a warm control sequence from its own state into buffers allocated once."""
    from autorally_amd import capi
    sols, states = fleet(net, "auto", n, K, T)
    try:
        rng = np.random.RandomState(5)
        for s in sols:
            s.set_control_seq(np.stack([rng.uniform(-0.5, 0.5, T), rng.uniform(-0.2, 0.6, T)], axis=1).astype(np.float32))
        out = [(np.zeros((T, 7), np.float32), np.zeros((T, 2), np.float32)) for _ in sols]
        fp = capi.C.POINTER(capi.C.c_float)
        hs = (capi.C.c_void_p * n)(*[s.h for s in sols])
        st = np.ascontiguousarray(np.stack(states), np.float32)
        ssp, csp = (fp * n)(*[capi._fp(o[0]) for o in out]), (fp * n)(*[capi._fp(o[1]) for o in out])
        L = sols[0].L

        def fused():
            assert L.mppi_nominal_and_gains_batch(hs, capi._fp(st), ssp, csp, n) == capi.OK

        def two():
            assert L.mppi_nominal_traj_batch(hs, capi._fp(st), ssp, csp, n) == capi.OK
            assert L.mppi_compute_feedback_gains_batch(hs, capi._fp(st), ssp, csp, n) == capi.OK

        def clock(fn):
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0
        for _ in range(warm):
            fused()
            two()
        tf, tt, tf2 = [], [], []
        for _ in range(calls):
            tf.append(clock(fused))
            tt.append(clock(two))
            tf2.append(clock(fused))
        row = {"net": "-".join(map(str, net)), "n": n, "T": T}
        row["fused_ms"], row["two_ms"], row["fused_again_ms"] = (1e3 * float(np.median(t)) for t in (tf, tt, tf2))
        fused()
        row["fused"] = sols[0].debug_nominal_and_gains_info()
        return row
    finally:
        for s in sols:
            s.close()


def finish_table(nets, ns=(2, 4, 16, 64), T=100, calls=200):
    rows = []
    for net in nets:
        for n in ns:
            row = finish_ms(net, n, T=T, calls=calls)
            rows.append(row)
            print("FLEET FINISH n=%d T=%d net=%s: one call %.4f ms (fused %d; again %.4f ms: A/A %.4f ms)  replay + gains, two calls %.4f ms;  "
                  "two/one %.2f" % (n, T, row["net"], row["fused_ms"], row["fused"], row["fused_again_ms"],
                                    abs(row["fused_ms"] - row["fused_again_ms"]), row["two_ms"], row["two_ms"] / row["fused_ms"]), flush=True)
    return rows


def trace_ms(net, n, K=1920, T=100, rollouts=64, calls=100, warm=5):
    """The 64 best sampled trajectories of each of n solved handles, each the median wall time of `calls` calls after `warm` warm
    ones: the batch entry (the largest weights chosen on the device, one trace launch for the fleet) twice -- interleaved, their
    difference is the A/A spread of the visit -- against the same handles one by one (mppi_top_rollouts + mppi_trace_rollouts).
    Every call fills buffers allocated once."""
    from autorally_amd import capi
    sols, states = fleet(net, "auto", n, K, T)
    try:
        for s, st in zip(sols, states):
            s.compute_control(st)
        C = capi.C
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
        c = rollouts
        bufs = [dict(ks=np.zeros(c, np.int32), states=np.zeros((c, T, 7), np.float32), controls=np.zeros((c, T, 2), np.float32),
                     step_costs=np.zeros((c, T), np.float32), costs=np.zeros(c, np.float32), first_crash=np.zeros(c, np.int32)) for _ in sols]
        arr = lambda key, ptr: (ptr * n)(*[b[key].ctypes.data_as(ptr) for b in bufs])  # noqa: E731
        hs = (C.c_void_p * n)(*[s.h for s in sols])
        counts = (C.c_int * n)(*([c] * n))
        args = (arr("ks", ip), arr("states", fp), arr("controls", fp), arr("step_costs", fp), arr("costs", fp), arr("first_crash", ip))
        L = sols[0].L

        def batch():
            assert L.mppi_trace_rollouts_batch(hs, n, counts, None, *args) == capi.OK

        def single():
            for s, b in zip(sols, bufs):
                assert L.mppi_top_rollouts(s.h, c, b["ks"].ctypes.data_as(ip)) == capi.OK
                assert L.mppi_trace_rollouts(s.h, b["ks"].ctypes.data_as(ip), c, capi._fp(b["states"]), capi._fp(b["controls"]),
                                             capi._fp(b["step_costs"]), capi._fp(b["costs"]), b["first_crash"].ctypes.data_as(ip)) == capi.OK

        def clock(fn):
            t0 = time.perf_counter()
            fn()
            return time.perf_counter() - t0
        for _ in range(warm):
            batch()
            single()
        ta, tb, ts = [], [], []
        for _ in range(calls):
            ta.append(clock(batch))
            ts.append(clock(single))
            tb.append(clock(batch))
        row = {"net": "-".join(map(str, net)), "n": n, "K": K, "T": T, "rollouts": c}
        row["batch_ms"], row["batch_again_ms"], row["single_ms"] = (1e3 * float(np.median(t)) for t in (ta, tb, ts))
        batch()
        row["on_device"] = sols[0].debug_trace_info()
        return row
    finally:
        for s in sols:
            s.close()


def trace_table(nets, ns=(4, 16, 64), K=1920, T=100, calls=100):
    rows = []
    for net in nets:
        for n in ns:
            row = trace_ms(net, n, K=K, T=T, calls=calls)
            rows.append(row)
            print("FLEET TRACE n=%d K=%d T=%d net=%s, %d rollouts each: batch %.4f ms (on_device %d; again %.4f ms: A/A %.4f ms)  handle by handle "
                  "%.4f ms;  single/batch %.2f" % (n, K, T, row["net"], row["rollouts"], row["batch_ms"], row["on_device"], row["batch_again_ms"],
                                                    abs(row["batch_ms"] - row["batch_again_ms"]), row["single_ms"], row["single_ms"] / row["batch_ms"]),
                  flush=True)
    return rows


def closed_loop_ms(net, variant, n=64, K=1920, T=100, ticks=200, stride=1, runs=3, warm=20):
    """-> a row: ms per tick of the device loop, of the reference loop inside the library and of the reference loop from Python
    (the median of `runs` runs each, alternating), and what mppi_debug_closed_loop_info says of the first two."""
    from autorally_amd import capi
    sols, states = fleet(net, variant, n, K, T)
    try:
        def restart():
            for i, s in enumerate(sols):
                s.reset_controls()
                s.seed(1000 + i, 0)
            return [st.copy() for st in states]

        def library(device):
            st = restart()
            os.environ["MPPI_CLOSED_LOOP_DEVICE"] = "1" if device else "0"
            try:
                t0 = time.perf_counter()
                capi.closed_loop_ticks_batch(sols, st, ticks, stride)
                return (time.perf_counter() - t0) / ticks, sols[0].debug_closed_loop_info()
            finally:
                os.environ.pop("MPPI_CLOSED_LOOP_DEVICE", None)

        def python():
            st = restart()
            t0 = time.perf_counter()
            for _ in range(ticks):
                capi.compute_control_batch(sols, st)
                seqs = capi.nominal_traj_batch(sols, st)
                st = [x[0][stride].copy() for x in seqs]
                for s in sols:
                    s.slide_control_seq(stride)
            return (time.perf_counter() - t0) / ticks

        capi.closed_loop_ticks_batch(sols, restart(), warm, stride)
        td, tr, tp, info_d, info_r = [], [], [], None, None
        for _ in range(runs):
            d, info_d = library(True)
            r, info_r = library(False)
            td.append(d)
            tr.append(r)
            tp.append(python())
        row = {"net": "-".join(map(str, net)), "variant": variant, "n": n, "K": K, "T": T, "ticks": ticks, "stride": stride}
        row["device_ms"], row["reference_ms"], row["python_ms"] = (1e3 * float(np.median(t)) for t in (td, tr, tp))
        row["device_runs_ms"], row["reference_runs_ms"] = [1e3 * t for t in td], [1e3 * t for t in tr]
        row["on_device"], row["reference_on_device"] = info_d[0], info_r[0]
        return row
    finally:
        for s in sols:
            s.close()


def closed_loop_table(nets, variant=None, n=64, K=1920, T=100, ticks=200):
    rows = []
    for net in nets:
        v = variant or ("fleet_multi4" if net == [6, 32, 32, 4] else "fleet16")
        row = closed_loop_ms(net, v, n, K, T, ticks)
        rows.append(row)
        print("FLEET CLOSED LOOP n=%d K=%d T=%d net=%s %s, %d ticks: device loop %.4f ms per tick (on_device %d)  reference loop in the library "
              "%.4f ms  from Python %.4f ms;  reference/device %.2f" % (n, K, T, row["net"], v, ticks, row["device_ms"], row["on_device"],
                                                                      row["reference_ms"], row["python_ms"], row["reference_ms"] / row["device_ms"]),
              flush=True)
    return rows


def _with_plants(sols, net):
    """every handle's plant: its own layer list with the weights of a perturbed copy (scaled by 1.05)"""
    for s in sols:
        s.set_plant_model(net, np.asarray(s.cfg["theta"], np.float32) * np.float32(1.05), s.cfg["negate_yaw_der"])


def closed_loop_sim_ms(net, variant, substeps, feedback, n=64, K=1920, T=100, ticks=100, stride=1, runs=3, warm=10):
    """-> a row: ms per tick of mppi_closed_loop_sim_batch's device loop and of the loop of public calls inside the library
    (MPPI_CLOSED_LOOP_DEVICE=0), the median of `runs` runs each, alternating in one process, and what mppi_debug_closed_loop_info says
    of each.  The plant is the controller's network with its weights scaled by 1.05."""
    from autorally_amd import capi
    sols, states = fleet(net, variant, n, K, T)
    try:
        _with_plants(sols, net)

        def library(device, count):
            for i, s in enumerate(sols):
                s.reset_controls()
                s.seed(1000 + i, 0)
            st = [x.copy() for x in states]
            os.environ["MPPI_CLOSED_LOOP_DEVICE"] = "1" if device else "0"
            try:
                t0 = time.perf_counter()
                capi.closed_loop_sim_batch(sols, st, count, stride, substeps, feedback)
                return (time.perf_counter() - t0) / count, sols[0].debug_closed_loop_info()
            finally:
                os.environ.pop("MPPI_CLOSED_LOOP_DEVICE", None)

        library(True, warm)
        td, tr, info_d, info_r = [], [], None, None
        for _ in range(runs):
            d, info_d = library(True, ticks)
            r, info_r = library(False, ticks)
            td.append(d)
            tr.append(r)
        row = {"net": "-".join(map(str, net)), "variant": variant, "n": n, "K": K, "T": T, "ticks": ticks, "stride": stride,
               "substeps": substeps, "feedback": int(bool(feedback))}
        row["device_ms"], row["reference_ms"] = (1e3 * float(np.median(t)) for t in (td, tr))
        row["device_runs_ms"], row["reference_runs_ms"] = [1e3 * t for t in td], [1e3 * t for t in tr]
        row["on_device"], row["reference_on_device"] = info_d[0], info_r[0]
        return row
    finally:
        for s in sols:
            s.close()


def closed_loop_sim_table(nets, variant=None, n=64, K=1920, T=100, ticks=100):
    rows = []
    for net in nets:
        v = variant or ("fleet_multi4" if net == [6, 32, 32, 4] else "fleet16")
        for substeps in (1, 4):
            for feedback in (False, True):
                row = closed_loop_sim_ms(net, v, substeps, feedback, n, K, T, ticks)
                rows.append(row)
                print("FLEET CLOSED LOOP SIM n=%d K=%d T=%d net=%s %s m=%d feedback=%d, %d ticks: first way %.4f ms per tick (on_device %d)  loop "
                      "of public calls in the library %.4f ms;  ratio %.2f" % (n, K, T, row["net"], v, substeps, feedback, ticks, row["device_ms"],
                                                                              row["on_device"], row["reference_ms"], row["reference_ms"] / row["device_ms"]),
                      flush=True)
    return rows


def plant_drive_ms(net, n=64, T=100, periods=1, substeps=4, feedback=True, calls=200, warm=10):
    """-> a row: ms per call of mppi_plant_drive_batch with every image copied to LDS and with every image in global memory
    (MPPI_PLANT_DRIVE_LDS = 1 / 0), the median of `calls` calls each, alternating in blocks of ten."""
    from autorally_amd import capi
    sols, states = fleet(net, "auto", n, 64, T)
    try:
        _with_plants(sols, net)
        seqs = capi.nominal_and_gains_batch(sols, states)
        out = None
        times = {"1": [], "0": []}
        for c in range(warm + calls):
            for sw in ("1", "0"):
                os.environ["MPPI_PLANT_DRIVE_LDS"] = sw
                t0 = time.perf_counter()
                out = capi.plant_drive_batch(sols, states, seqs, periods, substeps, feedback, outputs=out)
                if c >= warm:
                    times[sw].append(time.perf_counter() - t0)
        os.environ.pop("MPPI_PLANT_DRIVE_LDS", None)
        return {"net": "-".join(map(str, net)), "n": n, "T": T, "periods": periods, "substeps": substeps, "feedback": int(bool(feedback)),
                "lds_ms": 1e3 * float(np.median(times["1"])), "global_ms": 1e3 * float(np.median(times["0"])),
                "on_device": sols[0].debug_plant_drive_info()}
    finally:
        os.environ.pop("MPPI_PLANT_DRIVE_LDS", None)
        for s in sols:
            s.close()


def plant_drive_table(nets, n=64, T=100, calls=200):
    rows = []
    for net in nets:
        for periods, substeps in ((1, 1), (1, 4), (2, 4)):
            row = plant_drive_ms(net, n, T, periods, substeps, True, calls)
            rows.append(row)
            print("FLEET PLANT DRIVE n=%d T=%d net=%s P=%d m=%d feedback=1 (on_device %d): image in LDS %.4f ms per call, in global memory %.4f ms" % (
                n, T, row["net"], periods, substeps, row["on_device"], row["lds_ms"], row["global_ms"]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=None, help="handles (default 16; --mixed: 4 16 64, one row each)")
    ap.add_argument("--mixed", nargs="+", default=None, help="the layer lists the handles of a \"fleet_glb16\" fleet cycle through, ways abcdA")
    ap.add_argument("--K", type=int, default=None, help="rollouts per handle (default 1920; --model bf: 2560)")
    ap.add_argument("--model", default="nn", choices=["nn", "bf"], help="bf: the basis-function model, ways f123cF (and p, q, r)")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--ways", default=None, help="(default abc; --model bf: f123cF) which of (a) fleet16, (b) lds16, (c) auto, (d) fleet_multi4, (A) fleet16 again to run")
    ap.add_argument("--net", nargs="*", default=["6-32-32-4", "6-64-64-64-64-4"])
    ap.add_argument("--ddp", action="store_true", help="the DDP feedback gains of the fleet instead: the batch entry against the host "
                    "passes, n = 2, 4, 16, 64 (mppi_compute_feedback_gains_batch)")
    ap.add_argument("--nominal", action="store_true", help="the nominal trajectories of the fleet instead: the batch entry against the "
                    "host replays, n = 2, 4, 16, 64 (mppi_nominal_traj_batch)")
    ap.add_argument("--trace", action="store_true", help="the best 64 sampled trajectories of every handle instead: the batch entry against "
                    "the per-handle calls, n = 4, 16, 64 (mppi_trace_rollouts_batch)")
    ap.add_argument("--finish", action="store_true", help="the closing stages of the fleet's tick instead: the fused entry against the "
                    "batched replay followed by the batched gains, n = 2, 4, 16, 64 (mppi_nominal_and_gains_batch)")
    ap.add_argument("--closed-loop", action="store_true", help="closed-loop ticks of the fleet instead: all ticks enqueued on the device "
                    "against the reference loop inside the library and from Python (mppi_closed_loop_ticks_batch)")
    ap.add_argument("--variant", default=None, help="--closed-loop: the fleet form (default fleet_multi4 for 6-32-32-4, else fleet16)")
    ap.add_argument("--closed-loop-sim", action="store_true", help="closed-loop ticks against a plant of its own instead: the device loop "
                    "against the loop of public calls inside the library, m in {1, 4}, feedback off / on (mppi_closed_loop_sim_batch)")
    ap.add_argument("--plant-drive", action="store_true", help="the batched plant drive instead: the plant's image in LDS against the image "
                    "in global memory (mppi_plant_drive_batch)")
    a = ap.parse_args()
    from autorally_amd import build as B
    B.build()
    parse = lambda names: [[int(x) for x in s.split("-")] for s in names]  # noqa: E731
    if a.closed_loop_sim:
        print(json.dumps(closed_loop_sim_table(parse(a.net), a.variant, a.n[0] if a.n else 64, a.K or 1920, a.T, min(a.ticks, 100))))
        return
    if a.plant_drive:
        print(json.dumps(plant_drive_table(parse(a.net), a.n[0] if a.n else 64, a.T, a.ticks)))
        return
    if a.closed_loop:
        print(json.dumps(closed_loop_table(parse(a.net), a.variant, a.n[0] if a.n else 64, a.K or 1920, a.T, a.ticks)))
        return
    if a.mixed:
        print(json.dumps(mixed_table(parse(a.mixed), a.n or (4, 16, 64), a.K or 1920, a.T, a.ticks, a.warm, a.ways or "abcdA")))
        return
    if a.trace:
        print(json.dumps(trace_table(parse(a.net), a.n or (4, 16, 64), a.K or 1920, a.T, min(a.ticks, 100))))
        return
    if a.finish:
        print(json.dumps(finish_table(parse(a.net), a.n or (2, 4, 16, 64), a.T, a.ticks)))
        return
    a.n = a.n[0] if a.n else 16
    if a.nominal:
        print(json.dumps(nominal_table([[int(x) for x in s.split("-")] for s in a.net], T=a.T, calls=a.ticks)))
        return
    if a.ddp:
        print(json.dumps(ddp_table([[int(x) for x in s.split("-")] for s in a.net], T=a.T, calls=a.ticks)))
        return
    if a.model == "bf":
        print(json.dumps(table_bf(a.n, a.K or 2560, a.T, a.ticks, a.warm, a.ways or "f123cF")))
        return
    rows = table([[int(x) for x in s.split("-")] for s in a.net], a.n, a.K or 1920, a.T, a.ticks, a.warm, a.ways or "abc")
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
