"""The four linear operators of equiformer_amd/ops.py issue exactly the launches recorded in tests/golden/linear_trace.json:
the same eqf_gemm_group / eqf_gemmx_group chunks with the same descriptors in the same order, the same eqf_colsum calls, the
same operands (tests/linear_trace.py says how they are named), outputs and gradients of the same shape and stride.  The file
was recorded when every operator still had its own autograd Functions; the kernels and their descriptors being the same, equal
traces mean equal results.  Runs on CPU tensors: no GPU needed."""
import json
import os

import pytest

import linear_trace

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "linear_trace.json")) as f:
    GOLDEN = linear_trace.unpack(json.load(f))
CASES = sorted(list(linear_trace.CASES) + [c + "@fp32" for c in linear_trace.FP32_CASES])


def test_the_recorded_file_covers_every_case_and_pass():
    assert sorted(GOLDEN) == CASES
    for case in CASES:
        assert sorted(GOLDEN[case]) == sorted(linear_trace.PASSES)
        assert GOLDEN[case]["backward_immediate"]["events"]  # (a record without launches would prove nothing)


@pytest.mark.parametrize("which", linear_trace.PASSES)
@pytest.mark.parametrize("case", CASES)
def test_trace_equals_the_recorded_one(case, which):
    name, _, mode = case.partition("@")
    got = json.loads(json.dumps(linear_trace.trace(name, which, mode or "split")))
    want = GOLDEN[case][which]
    assert got["tensors"] == want["tensors"]
    assert len(got["events"]) == len(want["events"])
    for i, (g, w) in enumerate(zip(got["events"], want["events"])):
        assert g == w, "event %d" % i
