"""Rollout-stage times of the "glb16" form: "glb16", "glb16_r0" (every block of the stream from global memory) and
"valu_lds" on the lists only "valu_lds" served, "glb16", "glb16_r0" and "lds16" on lists "lds16" serves.  K in {1920, 16 384,
65 536}, T = 100: the kernel's own dispatch time (mppi_get_stage_times, every 2nd solve timed), median of the samples of each form,
the forms alternating in blocks inside one process.  A form whose solve takes more than 50 ms gets fewer samples; the count is
printed beside every median.
    python tools/glb16_table.py [--k 1920,16384] [--lists 6-129-4,6-256-256-4] [> profiles/<round>_glb16_rollout_times.txt]
The read-ahead depth (kGlb16Ahead, csrc/mppi_kernels.hpp) is a constant of the library, so its comparison is between two
libraries and therefore between processes: --depth-ab OTHER.so runs this build and OTHER.so (tools/build_variant.sh) in child
processes in turn, A B A B, and prints the median over both rounds.
    python tools/glb16_table.py --depth-ab tools/variants/glb16_a4.so [>> profiles/<round>_glb16_rollout_times.txt]
"""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autorally_amd import build as B  # noqa: E402
from autorally_amd import capi  # noqa: E402
from autorally_amd import synthetic as S  # noqa: E402

T = 100
KS = [1920, 16384, 65536]
WIDE = [[6, 129, 4], [6, 200, 256, 4], [6, 256, 256, 4], [6, 128, 128, 128, 128, 4], [6, 256, 256, 256, 256, 256, 256, 4]]
SHARED = [[6, 64, 64, 4], [6, 128, 128, 4], [6, 128, 128, 128, 4]]
DEPTH_LISTS = [[6, 256, 256, 4], [6, 128, 128, 128, 128, 4]]


def forms_for(layers):
    return ["glb16", "glb16_r0", "lds16" if layers in SHARED else "valu_lds"]


def sample(sol, st, every=2):
    sol.enable_stage_timing(every)
    sol.reset_stage_times()
    for _ in range(every):
        sol.compute_control(st)
        sol.slide_control_seq(1)
    t = sol.get_stage_times()
    sol.enable_stage_timing(0)
    return 1e3 * t["rollout_ms"] / max(1, t["n_solves"])


def arg(name, default):
    a = sys.argv[1:]
    return a[a.index(name) + 1] if name in a else default


def measure(layers, K, forms):
    """{form: samples in us}: warm-up, then blocks of samples, the forms in turn"""
    cfg = S.make_config(K, T, layers=layers, track="oval")
    st = cfg["start_state"]
    sols, per_block, names = {}, {}, {}
    for v in forms:
        sol = capi.Solver(cfg)
        sol.set_rollout_variant(v)
        sols[v], names[v] = sol, sol.rollout_variant()
        t0 = time.time()
        sol.compute_control(st)  # code object loaded, every buffer touched
        slow = time.time() - t0
        if slow < 0.05:
            for _ in range(19):
                sol.compute_control(st)
        per_block[v] = 10 if slow < 0.05 else 2 if slow < 1.0 else 1
    got = {v: [] for v in sols}
    for block in range(5 if all(n > 2 for n in per_block.values()) else 3):
        for v, sol in sols.items():
            if per_block[v] <= 2 and block > 0:
                continue
            got[v] += [sample(sol, st) for _ in range(per_block[v])]
    for sol in sols.values():
        sol.close()
    return got, names


def table():
    ks = [int(x) for x in arg("--k", ",".join(map(str, KS))).split(",")]
    want = arg("--lists", None)
    lists = [l for l in WIDE + SHARED if want is None or "-".join(map(str, l)) in want.split(",")]
    for K in ks:
        print("rollout stage, K = %d, T = %d, us: median (min .. max, samples)" % (K, T), flush=True)
        for layers in lists:
            got, names = measure(layers, K, forms_for(layers))
            line = ["%-26s" % "-".join(map(str, layers))]
            for v, x in got.items():
                line.append("%s (%s) %.1f (%.1f .. %.1f, %d)" % (v, names[v], np.median(x), min(x), max(x), len(x)))
            print("  ".join(line), flush=True)


def depth_child():
    out = {}
    for layers in DEPTH_LISTS:
        for K in (1920, 16384):
            got, _ = measure(layers, K, ["glb16", "glb16_r0"])
            out["%s K=%d" % ("-".join(map(str, layers)), K)] = got
    print("DEPTH " + json.dumps(out), flush=True)


def depth_ab(other):
    libs = {"this build": capi.LIB_PATH, os.path.relpath(other, ROOT): os.path.abspath(other)}
    acc = {name: {} for name in libs}
    for rnd in range(2):
        for name, path in libs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--depth-child"], env=dict(os.environ, MPPI_LIB_PATH=path),
                               capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise RuntimeError("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
            res = json.loads([l for l in r.stdout.split("\n") if l.startswith("DEPTH ")][-1][6:])
            for case, forms in res.items():
                for v, x in forms.items():
                    acc[name].setdefault((case, v), []).extend(x)
    print("read-ahead depth, rollout stage, T = %d, us: median (min .. max, samples) over two rounds of child processes, A B A B" % T)
    for case, v in sorted(next(iter(acc.values()))):
        line = ["%-34s %-9s" % (case, v)]
        for name in libs:
            x = acc[name][(case, v)]
            line.append("%s: %.1f (%.1f .. %.1f, %d)" % (name, np.median(x), min(x), max(x), len(x)))
        print("  ".join(line), flush=True)


if __name__ == "__main__":
    if "--depth-child" in sys.argv:
        depth_child()
    elif "--depth-ab" in sys.argv:
        B.build()
        depth_ab(arg("--depth-ab", None))
    else:
        B.build()
        table()
