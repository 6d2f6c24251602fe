"""tools/record_row_chunked_golden.py <out.json>: SHA-256 of V, costs and U of the "row_tree" form for every shape of
tests/test_row_chunked_gpu.py, on that test's inputs -- run ONCE with the library of the commit before a change that must
keep the bits (MPPI_LIB_PATH=<that build>), committed as tests/golden/row_chunked_parent.json."""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import test_row_chunked_gpu as R  # noqa: E402

out = {}
for T in R.TS:
    for K in R.KS:
        cfg, U0, eps = R.inputs(K, T)
        got = R.solve(cfg, U0, eps, "row_tree")
        assert "row8w_tree" in got["variant"]
        out["K%d_T%d" % (K, T)] = {k: R.sha(got[k]) for k in ("V", "costs", "U")}
        print("K=%d T=%d %s" % (K, T, out["K%d_T%d" % (K, T)]["costs"][:16]), flush=True)
with open(sys.argv[1], "w") as f:
    json.dump(out, f, indent=0, sort_keys=True)
