"""Rollout-stage times of the "lds16" form against the forms it stands beside: "valu_lds" on every list, "lds44" on
lists up to 64 wide, "lds128" where its image fits, and on 6-64-64-4 the forms that keep the weights in registers ("multi4_gen",
"fused": what the LDS operand costs).  K in {1920, 16 384, 65 536}, T = 100: the kernel's own dispatch time
(mppi_get_stage_times, every 2nd solve timed), median of 50 samples per form, the forms alternating in blocks inside one process.
    python tools/lds16_table.py [--k 1920,16384] [--lists 6-48-48-4,6-128-128-4] [> profiles/<round>_lds16_rollout_times.txt]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autorally_amd import build as B  # noqa: E402
from autorally_amd import capi  # noqa: E402
from autorally_amd import synthetic as S  # noqa: E402

T = 100
KS = [1920, 16384, 65536]
LISTS = [[6, 32, 32, 32, 4], [6, 48, 48, 4], [6, 64, 64, 64, 4], [6, 96, 96, 4], [6, 128, 128, 4], [6, 128, 128, 128, 4], [6, 64, 64, 4]]
REGISTER_FORMS = {(6, 64, 64, 4): ["multi4_gen", "fused"]}


def forms_for(layers):
    out = ["lds16", "valu_lds"]
    if max(layers[1:-1]) <= 64:
        out.append("lds44")
    out.append("lds128")  # left out below where the handle refuses it (its image does not fit)
    return out + REGISTER_FORMS.get(tuple(layers), [])


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


def main():
    B.build()
    ks = [int(x) for x in arg("--k", ",".join(map(str, KS))).split(",")]
    want = arg("--lists", None)
    lists = [l for l in LISTS if want is None or "-".join(map(str, l)) in want.split(",")]
    for K in ks:
        print("rollout stage, K = %d, T = %d, us (median of 50 samples, min .. max)" % (K, T), flush=True)
        for layers in lists:
            cfg = S.make_config(K, T, layers=layers, track="oval")
            st = cfg["start_state"]
            sols, refused = {}, []
            for v in forms_for(layers):
                sol = capi.Solver(cfg)
                try:
                    sol.set_rollout_variant(v)
                except capi.MppiError as e:
                    if e.status != capi.ERR_UNSUPPORTED:
                        raise
                    refused.append(v)
                    sol.close()
                    continue
                sols[v] = sol
                for _ in range(20):  # clocks up, code objects loaded, every buffer touched
                    sol.compute_control(st)
            got = {v: [] for v in sols}
            for _ in range(5):
                for v, sol in sols.items():
                    got[v] += [sample(sol, st) for _ in range(10)]
            line = ["%-18s" % "-".join(map(str, layers))]
            for v, x in got.items():
                line.append("%s (%s) %.1f (%.1f .. %.1f)" % (v, sols[v].rollout_variant(), np.median(x), min(x), max(x)))
            line += ["%s refused" % v for v in refused]
            print("  ".join(line), flush=True)
            for sol in sols.values():
                sol.close()


if __name__ == "__main__":
    main()
