"""Times of mppi_trace_rollouts (csrc/rollout_trace.hip) on one GPU: n rollouts of a finished solve at K = 1920, T = 100 traced
with every output, median of 9 calls after one warm-up, wall clock of the whole call (launches, device-to-host copies of the
records, one synchronisation per chunk of 1024).  Beside it one mppi_rollout_only of the same handle on its automatic form.

  python tools/trace_time.py [--n 64,1024] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autorally_amd import capi, params as P, synthetic as S  # noqa: E402

MODELS = [("6-32-32-4", None, None), ("6-64-64-64-64-4", [6, 64, 64, 64, 64, 4], None), ("basis functions", None, "bf"),
          ("6-128-128-4 (image in global memory)", [6, 128, 128, 4], None)]


def median_ms(fn, reps=9):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="64,1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ns = [int(x) for x in a.n.split(",")]
    K, T = 1920, 100
    rows = []
    for name, layers, kind in MODELS:
        kw = {}
        if kind == "bf":
            kw["bf_W"] = P.load_bf_npz(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                                                    "models", "basis_function_09_12_2018.npz"))
        elif layers is not None:
            kw["layers"] = layers
        cfg = S.make_config(K, T, track="oval", **kw)
        sol = capi.Solver(cfg)
        sol.seed(7, 0)
        sol.compute_control(cfg["start_state"])
        row = dict(model=name, form=sol.rollout_variant(), K=K, T=T)
        for n in ns:
            ks = np.linspace(0, K - 1, n).astype(np.int32)
            row["trace_%d_ms" % n] = median_ms(lambda: sol.trace_rollouts(ks))
        row["rollout_only_ms"] = median_ms(lambda: sol.rollout_only(cfg["start_state"]))
        sol.close()
        rows.append(row)
        print(json.dumps(row))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
