"""tools/record_variant_requests.py <out.json> <commit>: what mppi_set_rollout_variant answers to every case of
tests/test_variant_requests_gpu.py (return code, message, reported variant, form candidates, whether mppi_arm is accepted) --
run ONCE with the library of the commit before a change that must keep them (<commit>: its full hash, written into the file),
committed as tests/golden/variant_requests.json."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests import test_variant_requests_gpu as V  # noqa: E402

out = {}
for model in V.MODELS:
    for phase in V.PHASES:
        got = V.run_model(model, phase)
        out.update(got)
        print("%s %s: %d cases, %d requests refused" % (model, phase, len(got), sum(r[0] != 0 for recs in got.values() for r in recs)),
              flush=True)
V.dump_golden(out, sys.argv[2], sys.argv[1])
