"""CPU: the depth-cut policy of `HipViewCompute` (engine._DepthCut behind `_cut_flag`) against a recorded run of the
single-method `_cut_flag` it was split from (tests/golden/depth_cut_policy.json, written by
tests/golden/make_depth_cut_golden.py at the commit named in the file).

The script in the file is replayed through the generator's own stand-ins for the rasterizer context, the workspace and the
library.  Per forward the returned debug bits, the arguments of the mgr_raster_set_cut_* calls, the views named in the
workspace, its cut_block flag and the bytes of the two hint regions must EQUAL the record: floats bit for bit (float.hex),
no tolerance -- it is the same arithmetic on the same kind of host."""
import json
import os
import sys

import pytest


@pytest.fixture(scope="module")
def trace(golden_dir):
    sys.path.insert(0, golden_dir)
    try:
        import make_depth_cut_golden as gen
    finally:
        sys.path.remove(golden_dir)
    with open(os.path.join(golden_dir, "depth_cut_policy.json")) as f:
        d = json.load(f)
    return gen, d


def test_the_trace_covers_what_it_must(trace):
    """Every outcome of the policy is in the record: the cut off / unfenced, cut_block, hints too old or never seen, the
    pauses of both modes, bits 8 and 8 | 2048; the margins at the 1x and the 32x clamp; a pause of 512 forwards (the
    back-off's cap: ten flagged forwards in a row would otherwise reach 4096) and one of 128 (halved twice by 66 clean
    forwards); parked hints restored and parked hints dropped."""
    gen, d = trace
    assert d["script"] == gen.script()            # (the generator still describes the file)
    ops, rec = d["script"], d["forwards"]
    fwd = [op for op in ops if op[0] == "forward"]
    assert len(fwd) == len(rec)
    assert {r[0] for r in rec} == {0, 8, 8 | 2048}
    assert any(r[2] is None for r in rec) and any(op[3] for op in fwd)                 # off / unfenced; cut_block
    assert {"tick", "set_params", "set"} <= {op[0] for op in ops}
    assert {(op[1], op[2]) for op in ops if op[0] == "set"} >= {("cut_repair", False), ("cut_repair", True), ("depth_cut", False)}
    legacy = [c for r in rec for c in r[1] if c[0] == "margin" and len(r[1]) == 1]     # (the repair mode also sets the penalty)
    assert {c[2] for c in legacy} >= {64, 64 * 32} and max(c[2] for c in legacy) == 64 * 32
    assert {c[5] for c in legacy} == {0, 1}
    runs, n = [], 0                               # lengths of the runs of forwards without the cut
    for r in rec:
        if r[0] == 0:
            n += 1
        elif n:
            runs.append(n)
            n = 0
    assert any(x >= 512 for x in runs) and 129 in runs and max(runs) < 512 + 32
    zeros = "00" * gen.REGION                     # view-set changes: hints brought back, and none to bring back
    changed = [r for a, b, r in zip(fwd, fwd[1:], rec[1:]) if a[1] != b[1] and r[2] is not None]
    assert any(r[4] != zeros and r[5] != zeros for r in changed) and any(r[4] == zeros and r[5] == zeros for r in changed)


def test_policy_replays_the_recorded_trace(trace):
    gen, d = trace
    got = gen.drive(d["script"])
    want = d["forwards"]
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "forward %d of the trace: got %r, recorded %r" % (i, g, w)


def test_decision_part_needs_no_library_and_no_tensor():
    """`_DepthCut.decide` alone, with nothing patched: plain host arithmetic."""
    from manus_amd.engine import _DepthCut
    cut = _DepthCut(max_hints=4)
    key = (0, 0, (0, 1))
    assert cut.decide(key, 0, False, True) == (0, (0.125, 64, 0.0625, 2.0e-4, 0))         # first sight: no usable hints
    assert cut.decide(key, 0, False, True) == (8 | 2048, (0.125, 64, 0.0625, 2.0e-4, 0))
    assert cut.decide(key, 0, True, True)[0] == 0                                          # cut_block
    assert cut.decide(key, 0, False, False) == (8, (0.125, 64, 0.0625, 2.0e-4, 0))
    bits, margins = cut.decide(key, 1, False, False)                                       # flagged: 2x, interior only, a pause of 4
    assert bits == 0 and margins == (0.25, 128, 0.125, 4.0e-4, 1) and (cut.pause, cut.backoff) == (3, 8)
    cut.clock += cut.max_age + 1
    assert cut.decide(key, 1, False, True)[0] == 0                                         # hints too old
    assert cut.store == {}
