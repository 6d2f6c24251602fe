"""Rollout-stage times of the "lds44" form against the forms it stands beside, K = 1920, T = 100:
the kernel's own dispatch time (mppi_get_stage_times, every 8th solve timed), median of 50 samples per form, the forms
alternating in blocks inside one process.
    python tools/lds44_table.py [> profiles/<round>_lds44_rollout_times.txt]
--wide: the same for the "lds128" form on lists up to 128 wide against "valu_lds" -- every 2nd solve timed, the
generic kernel takes milliseconds per solve there -- and, for information, against "lds44" on a list both serve.
    python tools/lds44_table.py --wide [> profiles/<round>_lds128_rollout_times.txt]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autorally_amd import build as B  # noqa: E402
from autorally_amd import capi  # noqa: E402
from autorally_amd import synthetic as S  # noqa: E402

K, T = 1920, 100
ROWS = [([6, 32, 32, 32, 4], []), ([6, 64, 64, 64, 4], []), ([6, 48, 48, 4], []), ([6, 16, 24, 4], []),
        ([6, 32, 32, 32, 32, 32, 32, 4], []), ([6, 64, 64, 4], ["m44_chain", "m44"]), ([6, 64, 64, 64, 64, 4], ["m44_chain", "m44"]),
        ([6, 32, 32, 4], ["row_exact", "row_tree"])]
WIDE_ROWS = [([6, 96, 96, 4], ["lds128", "valu_lds"]), ([6, 128, 128, 4], ["lds128", "valu_lds"]), ([6, 128, 64, 4], ["lds128", "valu_lds"]),
             ([6, 64, 128, 4], ["lds128", "valu_lds"]), ([6, 100, 72, 4], ["lds128", "valu_lds"]), ([6, 64, 64, 64, 4], ["lds128", "lds44"])]


def sample(sol, st, every=8):
    sol.enable_stage_timing(every)
    sol.reset_stage_times()
    for _ in range(every):
        sol.compute_control(st)
        sol.slide_control_seq(1)
    t = sol.get_stage_times()
    sol.enable_stage_timing(0)
    return 1e3 * t["rollout_ms"] / max(1, t["n_solves"])


def main():
    B.build()
    wide = "--wide" in sys.argv[1:]
    every = 2 if wide else 8
    print("rollout stage, K = %d, T = %d, us (median of 50 samples, min .. max)" % (K, T))
    for layers, forms in (WIDE_ROWS if wide else [(l, ["lds44", "valu_lds"] + extra) for l, extra in ROWS]):
        cfg = S.make_config(K, T, layers=layers, track="oval")
        st = cfg["start_state"]
        sols = {}
        for v in forms:
            sols[v] = capi.Solver(cfg)
            sols[v].set_rollout_variant(v)
            for _ in range(6 if wide else 20):
                sols[v].compute_control(st)
        got = {v: [] for v in sols}
        for _ in range(5):
            for v, sol in sols.items():
                got[v] += [sample(sol, st, every) for _ in range(10)]
        line = ["%-22s" % "-".join(map(str, layers))]
        for v, x in got.items():
            line.append("%s (%s) %.1f (%.1f .. %.1f)" % (v, sols[v].rollout_variant(), np.median(x), min(x), max(x)))
        print("  ".join(line), flush=True)
        for sol in sols.values():
            sol.close()


if __name__ == "__main__":
    main()
