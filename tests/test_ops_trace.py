"""Every public operator of equiformer_amd/ops.py but the four linears issues exactly the launches recorded in
tests/golden/ops_trace.json: the same entry points in the same order with the same operands (tests/ops_trace.py says how they
are named), outputs and gradients of the same shape and stride, None where None was.  The file was recorded when the first-order
branch of every `_X.backward` and the forward of its `_XBwd` still carried their own copy of the allocation and the call; the
kernels and their arguments being the same, equal traces mean equal results.  Runs on CPU tensors: no GPU needed."""
import json
import os
import re

import pytest

import ops_trace

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "ops_trace.json")) as f:
    GOLDEN = ops_trace.unpack(json.load(f))
CASES = sorted(ops_trace.CASES)

# entry points ops.py calls that another test holds: the grouped GEMMs of the linears (tests/test_linear_trace.py)
COVERED_ELSEWHERE = {"eqf_gemm_group", "eqf_gemmx_group"}


def test_the_recorded_file_covers_every_case_and_pass():
    assert sorted(GOLDEN) == CASES
    for case in CASES:
        assert sorted(GOLDEN[case]) == sorted(ops_trace.PASSES)
        events = GOLDEN[case]["backward_immediate"]["events"]
        assert events and events[0]["call"] != "raised"  # (a record without launches would prove nothing)


def test_the_cases_reach_every_entry_point_of_ops():
    with open(os.path.join(os.path.dirname(HERE), "equiformer_amd", "ops.py")) as f:
        called = set(re.findall(r'call\("(eqf_\w+)"', f.read()))
    seen = {e["call"] for case in CASES for which in ops_trace.PASSES for e in GOLDEN[case][which]["events"]} - {"raised"}
    assert seen == called - COVERED_ELSEWHERE


@pytest.mark.parametrize("which", ops_trace.PASSES)
@pytest.mark.parametrize("case", CASES)
def test_trace_equals_the_recorded_one(case, which):
    got = json.loads(json.dumps(ops_trace.trace(case, which)))
    want = GOLDEN[case][which]
    assert got["tensors"] == want["tensors"]
    assert len(got["events"]) == len(want["events"])
    for i, (g, w) in enumerate(zip(got["events"], want["events"])):
        assert g == w, "event %d" % i
