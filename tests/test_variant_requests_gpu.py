"""mppi_set_rollout_variant, request by request: every spelling the parser accepts, malformed ones and a few two-request
sequences, on every kind of model, before and after the parameters are set.  After each request: the return code, the text of
mppi_last_error when the call failed, mppi_rollout_variant, the list of mppi_debug_form_candidates and -- on the handles with
parameters, costmap and cost parameters -- whether mppi_arm(h, 0.05) is MPPI_OK or MPPI_ERR_UNSUPPORTED (mppi_disarm at once).
All of it equals tests/golden/variant_requests.json, recorded by tools/record_variant_requests.py at the commit the file names,
with ==.  Every case runs on a handle of its own (K = 64, T = 4): what a request leaves behind reaches only the second request
of its own sequence.  No solve runs; an accepted mppi_arm enqueues one gated launch of that size, called off at once."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from autorally_amd import capi
from autorally_amd import synthetic as S
from tests import branch_cases as BC

pytestmark = pytest.mark.gpu

K, T = 64, 4  # the smallest mppi_create accepts with the slide stride (1) inside T
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "variant_requests.json")
# the layer lists of tests/branch_cases.py, the too_big list of tests/test_lds16_gpu.py, one of tests/test_glb16_gpu.py's lists
# with a hidden width above 128, and the basis-function model
MODELS = {"32x2": None, "32x4": BC.NET_LAYERS["32x4"], "64x2": BC.NET_LAYERS["64x2"], "64x4": BC.NET_LAYERS["64x4"],
          "16-8": BC.NET_LAYERS["16-8"], "65": BC.NET_LAYERS["65"], "128x4": [6, 128, 128, 128, 128, 4],
          "200-256": [6, 200, 256, 4], "bf": "bf"}
PHASES = ["bare", "ready"]  # before mppi_set_nn_params / mppi_set_bf_params; with parameters, costmap and cost parameters
SPELLINGS = ["auto", "mfma", "valu", "valu_lds", "quad", "bf3", "bf_row", "row", "row_exact", "row_tree", "m44", "m44_chain",
             "lds44", "lds128", "lds16", "fleet16", "fleet_multi4", "glb16", "glb16_r0", "glb16_r3", "glb44", "glb44_r0",
             "glb44_r3", "row64", "row64_r16", "oct", "oct_gen", "multi2", "multi2_gen", "multi4", "multi4_gen", "multi4_tree",
             "multi4_tree_gen", "fused", "block256", "block64"]
MALFORMED = ["", "glb16_r", "glb16_rx", "glb44_r1234567890", "multi3", "multi2_ge", "m44x", "row64_r8", "lds"]
SEQUENCES = [("oct_gen", "oct"), ("fleet_multi4", "multi4_tree"), ("row_tree", "mfma"), ("glb16_r3", "glb16"), ("lds16", "auto")]
CASES = [(r,) for r in SPELLINGS + MALFORMED] + SEQUENCES


def case_key(model, phase, reqs):
    return "%s/%s/%s" % (model, phase, "+".join(reqs))


def _config(model):
    if MODELS[model] == "bf":
        return S.make_config(K, T, track="oval", bf_W=BC.bf_W())
    return S.make_config(K, T, layers=MODELS[model], track="oval")


def run_case(cfg, ready, reqs):
    """The requests `reqs` in turn on a fresh handle: [[rc, message or None, variant, candidates, arm rc or None]]."""
    L = capi.lib()
    h = C.c_void_p()
    c = capi.make_config_struct(cfg)
    assert L.mppi_create(C.byref(c), C.byref(h)) == capi.OK
    try:
        if ready:
            if cfg.get("bf_W") is not None:
                W = capi._f32(cfg["bf_W"], (4, 25))
                assert L.mppi_set_bf_params(h, capi._fp(W), W.size) == capi.OK
            else:
                theta = capi._f32(cfg["theta"])
                assert L.mppi_set_nn_params(h, capi._fp(theta), theta.size) == capi.OK
            m = capi._f32(cfg["map_rgba"][:8, :8])  # a corner of the map: nothing here samples it
            assert L.mppi_set_costmap(h, m.shape[1], m.shape[0], capi._fp(m), capi._fp(capi._f32(cfg["r_c1"])),
                                      capi._fp(capi._f32(cfg["r_c2"])), capi._fp(capi._f32(cfg["trs"]))) == capi.OK
            p = capi.make_cost_struct(cfg["cost"])
            assert L.mppi_set_cost_params(h, C.byref(p)) == capi.OK
        out = []
        for name in reqs:
            rc = L.mppi_set_rollout_variant(h, name.encode())
            msg = L.mppi_last_error(h).decode() if rc != capi.OK else None
            variant = L.mppi_rollout_variant(h).decode()
            buf = (C.c_char_p * 16)()
            cands = [buf[i].decode() for i in range(L.mppi_debug_form_candidates(h, buf, 16))]
            arm = None
            if ready:
                arm = L.mppi_arm(h, C.c_double(0.05))
                assert L.mppi_disarm(h) == capi.OK
            out.append([rc, msg, variant, cands, arm])
        return out
    finally:
        L.mppi_destroy(h)


def run_model(model, phase):
    cfg = _config(model)
    return {case_key(model, phase, reqs): run_case(cfg, phase == "ready", reqs) for reqs in CASES}


def load_golden():
    """{case key: records as run_case gives them}, and the commit they were recorded at.  The file holds every distinct message,
    variant name and candidate list once ("strings") and the records as indices into that list (-1: none)."""
    with open(GOLDEN) as f:
        g = json.load(f)
    s = g["strings"]
    cases = {}
    for key, recs in g["cases"].items():
        cases[key] = [[rc, None if m < 0 else s[m], s[v], [x for x in s[c].split(",") if x], None if arm < 0 else arm]
                      for rc, m, v, c, arm in recs]
    return cases, g["recorded_at"]


def dump_golden(cases, commit, path):
    strings, index = [], {}

    def ref(x):
        if x is None:
            return -1
        if x not in index:
            index[x] = len(strings)
            strings.append(x)
        return index[x]

    lines = []
    for key in sorted(cases):
        recs = [[rc, ref(m), ref(v), ref(",".join(c)), -1 if arm is None else arm] for rc, m, v, c, arm in cases[key]]
        lines.append("%s:%s" % (json.dumps(key), json.dumps(recs, separators=(",", ":"))))
    with open(path, "w") as f:
        f.write('{"recorded_at":%s,\n"strings":%s,\n"cases":{\n%s\n}}\n' % (
            json.dumps(commit), json.dumps(strings, indent=0), ",\n".join(lines)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from autorally_amd import build as B
    B.build()
    assert capi.lib().mppi_device_count() >= 1, "no gfx950 device: the HIP path cannot run"


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def test_the_recording_holds_every_case(golden):
    cases, commit = golden
    assert len(commit) == 40 and int(commit, 16) >= 0, commit
    want = {case_key(m, ph, reqs) for m in MODELS for ph in PHASES for reqs in CASES}
    assert set(cases) == want
    assert all(len(cases[case_key(m, ph, reqs)]) == len(reqs) for m in MODELS for ph in PHASES for reqs in CASES)
    assert any(rec[4] == capi.OK for recs in cases.values() for rec in recs), "no request of the recording could be armed"
    assert any(rec[4] == capi.ERR_UNSUPPORTED for recs in cases.values() for rec in recs)


@pytest.mark.parametrize("phase", PHASES)
@pytest.mark.parametrize("model", list(MODELS))
def test_every_request_answers_as_recorded(model, phase, golden):
    cases, commit = golden
    got = run_model(model, phase)
    diff = [(k, got[k], cases[k]) for k in got if got[k] != cases[k]]
    print("VARIANT REQUESTS %s %s: %d cases, %d differ from the recording of %s" % (model, phase, len(got), len(diff), commit[:7]))
    for k, g, w in diff[:10]:
        print("  %s\n    got      %s\n    recorded %s" % (k, g, w))
    assert not diff, [d[0] for d in diff]
    assert {k: got[k] for k in got} == {k: cases[k] for k in got}
