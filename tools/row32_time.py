#!/usr/bin/env python3
"""Rollout stage of the "row32" / "row32_tree" forms beside "lds44" and "auto" (DESIGN 4.27's table): per layer list and K one line
of medians in us, T = 100 -- the kernel's own dispatch time sampled every 8th solve, 30 samples per column, the columns
alternating in blocks of 10 inside one process, the new forms run twice (A ... A').

    python3 tools/row32_time.py [--K 1920,4096] [--layers 6,32,4/6,32,32,32,4]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from autorally_amd import synthetic as S  # noqa: E402
from tests.test_row32_gpu import _medians  # noqa: E402

NETS = "6,32,4/6,32,32,4/6,32,32,32,4/6,32,32,32,32,4/6,16,24,4"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--K", type=str, default="1920,4096")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--layers", type=str, default=NETS, help="layer lists, '/' between them")
    a = ap.parse_args()
    for K in [int(x) for x in a.K.split(",")]:
        for net in [[int(x) for x in l.split(",")] for l in a.layers.split("/")]:
            forms = (["row32"] if len(net) <= 5 else []) + ["row32_tree"]  # "row32": at most three hidden layers
            variants = forms + ["lds44", "auto"] + forms
            med, names = _medians(S.make_config(K, a.T, layers=net, track="oval"), variants, blocks=3)
            print("K=%d T=%d net=%s: " % (K, a.T, "-".join(map(str, net))) +
                  "  ".join("%s[%s] %.1f" % (v, n, m) for v, n, m in zip(variants, names, med)), flush=True)


if __name__ == "__main__":
    main()
