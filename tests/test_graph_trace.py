"""The graph builders of equiformer_amd/graph.py issue exactly what tests/golden/graph_trace.json records: the same entry points
in the same order with the same operands, the same torch writes between them, results with the same state and tensors, the
same errors with the same text (tests/graph_trace.py says how all of that is named).  The file was recorded when
`from_radius_plan`, `from_radius_pbc_plan` and `from_edges_pbc_plan` each carried their own copy of the padding code and
`from_radius`, `from_radius_pbc` and `from_edges_pbc_plan(capacity=None)` their own copy of the refill; the kernels and their
arguments being the same, equal traces mean equal graphs and equal host work.  Runs on CPU tensors: no GPU needed."""
import json
import os

import pytest

import graph_trace

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "graph_trace.json")) as f:
    GOLDEN = json.load(f)
CASES = sorted(graph_trace.CASES)

ENTRY_POINTS = {"eqf_segment_ptr", "eqf_exclusive_scan_i32", "eqf_radius_graph_count", "eqf_radius_graph_fill", "eqf_csr_by_source",
                "eqf_radius_graph_pbc_count", "eqf_radius_graph_pbc_fill", "eqf_csr_by_source_multi", "eqf_edges_pbc_count",
                "eqf_edges_pbc_fill", "eqf_graph_pad_tail"}


def _events(case):
    return [e for step in GOLDEN[case] for e in step["events"]]


def test_the_recorded_file_covers_every_case_and_every_entry_point_of_the_builders():
    assert sorted(GOLDEN) == CASES
    assert {e["call"] for case in CASES for e in _events(case) if "call" in e} == ENTRY_POINTS


def test_the_recorded_cases_took_the_paths_they_are_named_after():
    for s in graph_trace.SOURCES:
        fresh, refilled, again = GOLDEN["%s: 2 exact into equal counts" % s]
        assert not fresh["is_into"] and refilled["is_into"] and again["is_into"] and again["into_static"]
        first, other = GOLDEN["%s: 3 exact into another E" % s]
        assert not other["is_into"] and other["into_static"] is False and other["result"]["E"] == 5
        first, fewer, more = GOLDEN["%s: 5 padded into fewer then more edges" % s]
        assert fewer["is_into"] and more["is_into"]
        assert [r["result"]["e_real"] for r in (first, fewer, more)] == [6, 4, 7]
        assert fewer["result"]["n_real"] == 4 and more["result"]["capacity"] == [8, 12] and more["result"]["_padded"]
        first, without, with_z = GOLDEN["%s: 6 padded into z presence differs" % s]
        assert not without["is_into"] and "z" not in without["result"]["tensors"] and not with_z["is_into"]
        for which in ("E above", "N above", "Q 7 P 3"):
            made, refused = GOLDEN["%s: 7 does not fit %s" % (s, which)]
            ev = refused["events"]
            at = ev.index({"mark": "build"})
            assert len(ev) == at + 2 and ev[-1]["raised"][0] == "GraphDoesNotFit"  # (nothing between the plan and the refusal)
            assert refused["into_static"] is True
        assert _events("%s: 8 largest molecule padded" % s)[-1]["raised"][0] == "HipOnlyError"
    for s in ("radius", "pbc"):  # the device-sort fallback: no by-source launch, a graph no captured step may refill
        for step in GOLDEN["%s: 8 largest molecule exact" % s]:
            assert not step["result"]["_radius_static"] and not step["is_into"]
            assert not any(e.get("call", "").startswith("eqf_csr_by_source") for e in step["events"])
    assert GOLDEN["radius: 3 exact into another E"][1]["events"][3]["write"] == "clone"
    assert _events("edges: 8 largest molecule exact")[-1]["raised"][0] == "HipOnlyError"
    for case in ("edges: 9 wrong neighbour sum", "edges: 9 status"):
        assert [s["events"][-1]["raised"][0] for s in GOLDEN[case]] == ["ValueError", "ValueError"]


@pytest.mark.parametrize("case", CASES)
def test_trace_equals_the_recorded_one(case):
    got = json.loads(json.dumps(graph_trace.trace(case)))
    want = GOLDEN[case]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert len(g["events"]) == len(w["events"]), "step %d" % k
        for i, (ge, we) in enumerate(zip(g["events"], w["events"])):
            assert ge == we, "step %d, event %d" % (k, i)
        assert g == w, "step %d" % k
