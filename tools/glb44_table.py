"""Rollout-stage times of the "glb44" form: "glb44", "glb44_r0" (every quad of the stream from global memory) and
"glb16" on every list, "lds128" and "lds16" beside them where they serve the list.  K in {1920, 4096, 16 384}, T = 100: the
kernel's own dispatch time (mppi_get_stage_times, every 2nd solve timed), median of the samples of each form, the forms
alternating in blocks inside one process.  The count of samples is printed beside every median.
    python tools/glb44_table.py [--k 1920,4096] [--lists 6-129-4,6-256-256-4] [> profiles/<round>_glb44_rollout_times.txt]
The read-ahead depth (kGlb44Ahead, csrc/mppi_kernels.hpp) is a constant of the library, so its comparison is between two
libraries and therefore between processes: --depth-ab OTHER.so[,OTHER2.so] runs this build and the others (tools/build_variant.sh)
in child processes in turn, A B A B, and prints the median over both rounds.  kGlb44AheadLds (resident quads) likewise.
    tools/build_variant.sh glb44_a4 rollout_glb44.hip -DMPPI_GLB44_AHEAD=4
    python tools/glb44_table.py --depth-ab tools/variants/glb44_a4.so [>> profiles/<round>_glb44_rollout_times.txt]
"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from autorally_amd import build as B  # noqa: E402
from autorally_amd import capi  # noqa: E402
from autorally_amd import synthetic as S  # noqa: E402

T = 100
KS = [1920, 4096, 16384]
LISTS = [[6, 129, 4], [6, 128, 128, 128, 4], [6, 128, 128, 128, 128, 4], [6, 200, 256, 4], [6, 256, 256, 4],
         [6, 256, 256, 256, 256, 256, 256, 4], [6, 128, 128, 4]]
FORMS = ["glb44", "glb44_r0", "glb16", "lds128", "lds16"]
DEPTH_LISTS = [[6, 128, 128, 128, 4], [6, 256, 256, 4], [6, 128, 128, 4]]


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


def measure(layers, K, forms, blocks=5, per_block=10):
    """{form: samples in us} of the forms that serve the list: warm-up, then blocks of samples, the forms in turn"""
    cfg = S.make_config(K, T, layers=layers, track="oval")
    st = cfg["start_state"]
    sols, names = {}, {}
    for v in forms:
        sol = capi.Solver(cfg)
        try:
            sol.set_rollout_variant(v)
        except capi.MppiError:  # the form does not serve this list
            sol.close()
            continue
        sols[v], names[v] = sol, sol.rollout_variant()
        for _ in range(10):  # code object loaded, every buffer touched
            sol.compute_control(st)
    got = {v: [] for v in sols}
    for block in range(blocks):
        for v, sol in sols.items():
            got[v] += [sample(sol, st) for _ in range(per_block)]
    for sol in sols.values():
        sol.close()
    return got, names


def table():
    ks = [int(x) for x in arg("--k", ",".join(map(str, KS))).split(",")]
    want = arg("--lists", None)
    lists = [l for l in LISTS if want is None or "-".join(map(str, l)) in want.split(",")]
    for K in ks:
        print("rollout stage, K = %d, T = %d, us: median (min .. max, samples)" % (K, T), flush=True)
        for layers in lists:
            got, names = measure(layers, K, FORMS)
            line = ["%-26s" % "-".join(map(str, layers))]
            for v, x in got.items():
                line.append("%s (%s) %.1f (%.1f .. %.1f, %d)" % (v, names[v], np.median(x), min(x), max(x), len(x)))
            print("  ".join(line), flush=True)


def depth_child():
    out = {}
    for layers in DEPTH_LISTS:
        got, _ = measure(layers, 1920, ["glb44", "glb44_r0"], blocks=3)
        out["%s K=1920" % "-".join(map(str, layers))] = got
    print("DEPTH " + json.dumps(out), flush=True)


def depth_ab(other):
    libs = {"this build": capi.LIB_PATH}
    libs.update({os.path.relpath(o, ROOT): os.path.abspath(o) for o in other.split(",")})
    acc = {name: {} for name in libs}
    for rnd in range(2):
        for name, path in libs.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--depth-child"], env=dict(os.environ, MPPI_LIB_PATH=path),
                               capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise RuntimeError("child failed (%d): %s" % (r.returncode, r.stderr[-2000:]))
            res = json.loads([l for l in r.stdout.split("\n") if l.startswith("DEPTH ")][-1][6:])
            for case, forms in res.items():
                for v, x in forms.items():
                    acc[name].setdefault((case, v), []).extend(x)
    print("read-ahead depth, rollout stage, T = %d, us: median (min .. max, samples) over two rounds of child processes, A B A B" % T)
    for case, v in sorted(next(iter(acc.values()))):
        line = ["%-28s %-9s" % (case, v)]
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
