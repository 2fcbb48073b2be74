"""The step classes -- CapturedTrainStep, BucketedTrainStep, BucketedEvalStep -- go through exactly the events recorded in
tests/golden/step_trace.json (tests/step_trace.py says what an event is and how tensors are named): the device words go out
before the plan's host read-back, the stochastic-depth word advances once per step, eager or not, `advance_captured` comes
immediately before each replay, the optimizer's step count is put back after the recorded region, the first replay follows the
capture, a record returns the same tensors at every replay, the counters move as recorded.  The file was recorded when each
class carried its own copy of the capture protocol.  Runs on the CPU: no GPU needed."""
import json
import os

import pytest

import step_trace

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "step_trace.json")) as f:
    GOLDEN = json.load(f)
SEQUENCES = sorted(step_trace.SEQUENCES)


def _steps(events):
    """the events of a sequence, split at its "step" events"""
    out = []
    for e in events:
        if e[0] == "step":
            out.append([])
        out[-1].append(e)
    return out


def _kinds(step):
    return [e[0] for e in step]


def test_the_recorded_file_covers_every_sequence():
    assert sorted(GOLDEN) == SEQUENCES


@pytest.mark.parametrize("kind", ["train", "eval"])
@pytest.mark.parametrize("mode", ["search", "pbc", "batch"])
def test_the_recorded_bucketed_sequences_are_the_expected_ones(kind, mode):
    steps = _steps(GOLDEN["bucketed %s %s" % (kind, mode)])
    what = ["capture" if "capture enter" in _kinds(s) else "replay" if "replay" in _kinds(s) else "eager" for s in steps[:8]]
    assert what == ["eager", "eager", "capture", "replay", "eager", "eager", "capture", "eager"]
    counters = [next(e for e in s if e[0] == "counters") for s in steps[:8]]
    assert counters[6][1]["evictions"] == 1 and counters[5][1]["evictions"] == 0 and counters[7][1]["replays"] == 3
    assert steps[8][-1][:2] == ["raised", "ValueError"]
    for s in steps[:8]:
        k = _kinds(s)
        plan = next(i for i, e in enumerate(s) if e[0].endswith("_plan") and not e[0].startswith("from_"))
        if kind == "train":  # both words are on their way before the plan reads back
            words = [e[1][0] for e in s[:plan] if e[0] == "copy_"]
            assert words == ["seed_word", "drop_path_word"], words
        if "replay" in k:
            i = k.index("replay")
            assert kind == "eval" or k[i - 1] == "opt.advance_captured"
        if "capture enter" in k:
            assert k.index("replay") > k.index("capture exit")
            if kind == "train":
                assert k.index("opt._step read") < k.index("capture enter") < k.index("capture exit") < k.index("opt._step write")
    # target buffers: new zero-filled ones for a fresh graph, the rows behind the real ones zeroed on a refill
    assert [e[1][1:] for e in steps[0] if e[0] == "zeros"] == [[0, [3]], [0, [16, 3]]]
    assert "zeros" not in _kinds(steps[3])
    assert [e[1][1:] for e in steps[3] if e[0] == "zero_"] == [[4 * 2, [1]], [4 * 3 * 4, [12, 3]]]
    # a record hands out the same buffers at every replay
    returned = [next(e for e in s if e[0] == "returned")[1] for s in steps[:8]]
    first = (lambda r: r[0] if kind == "train" else r[0][0])
    assert first(returned[2]) == first(returned[3]) and first(returned[2]) != first(returned[6])


def test_the_recorded_exact_shape_sequence_is_the_expected_one():
    steps = _steps(GOLDEN["captured train"])
    what = ["capture" if "capture enter" in _kinds(s) else "replay" if "replay" in _kinds(s) else "eager" for s in steps]
    assert what == ["eager", "eager", "capture", "replay", "eager", "eager", "capture", "capture", "eager", "eager", "eager"]
    for s in steps:
        k = _kinds(s)
        assert [e[1][0] for e in s if e[0] == "copy_"].count("drop_path_word") == 1 and s[1][1][0] == "drop_path_word"
        assert k.count("build_graph") == 1  # (one rebuild attempt per step)
        if "replay" in k:
            assert k[k.index("replay") - 1] == "opt.advance_captured"
    dropped = steps[4]  # S2 into the tensors of S1's record: the seed goes out before the build, the record goes
    assert _kinds(dropped)[1:5] == ["copy_", "randint", "copy_", "build_graph"] and dropped[4][2] == "graph#2"
    assert next(e for e in dropped if e[0] == "counters")[2] == []


@pytest.mark.parametrize("name", SEQUENCES)
def test_trace_equals_the_recorded_one(name):
    got = json.loads(json.dumps(step_trace.trace(name)))
    want = GOLDEN[name]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "event %d" % i
    assert len(got) == len(want)
