"""Host side of the graph build from a GIVEN periodic edge list (OC20 with otf_graph=False; EdgeGraph.from_edges_pbc and
edges="batch" of the step classes): the inputs of tests/test_gpu_given_edges.py hold what they are meant to exercise, their
pure-torch expectation agrees with oracle/pbc.py, the field check names what a batch lacks, and the two entry points are declared
and bound.  No GPU."""
import ctypes
import inspect
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import given_edges_inputs as gi  # noqa: E402
import periodic_inputs as pi  # noqa: E402


def _ranges(d):
    nb = d["neighbors"].tolist()
    out, start = [], 0
    for n in nb:
        out.append((start, start + n))
        start += n
    return out


def test_every_case_is_a_well_formed_ocpmodels_batch():
    cases = gi.cases()
    assert list(cases) == ["in order", "shuffled", "empty structure", "empty structure first", "empty structure last", "dropped",
                           "truncated", "no edges"]
    for name, d in cases.items():
        N, B, E = d["pos"].shape[0], d["cell"].shape[0], d["edge_index"].shape[1]
        assert d["edge_index"].shape == (2, E) and d["cell_offsets"].shape == (E, 3) and d["neighbors"].shape == (B,), name
        assert int(d["neighbors"].sum()) == E and E <= 1200, (name, E)
        assert d["edge_index"].dtype == d["cell_offsets"].dtype == (torch.int32 if name == "shuffled" else torch.int64), name
        assert d["edge_index"].is_contiguous() and d["cell_offsets"].is_contiguous()
        for b, (a0, a1) in enumerate(_ranges(d)):  # every edge inside its structure
            both = d["edge_index"][:, a0:a1].long()
            assert bool((d["batch"][both] == b).all()), (name, b)
        assert N == len(d["batch"]) == sum(d["natoms"])


def test_expected_agrees_with_the_oracle_and_a_stable_argsort():
    from oracle import pbc
    for name, d in gi.cases().items():
        x = gi.expected(name)
        ei, co = d["edge_index"].long(), d["cell_offsets"].long()
        kept_ei, dist, offsets = pbc.get_pbc_distances(d["pos"].double(), ei, d["cell"].double(), co, d["neighbors"])
        assert torch.equal(ei[:, x["keep"]], kept_ei), name
        order = torch.argsort(kept_ei[1], stable=True)
        assert torch.equal(x["src"].long(), kept_ei[0][order]) and torch.equal(x["dst"].long(), kept_ei[1][order]), name
        assert torch.equal(x["offsets"], offsets[order]), name
        assert torch.equal(x["cell_offsets"].long(), co[x["keep"]][order]), name
        assert torch.equal(ei[:, x["order"].long()], kept_ei[:, order]), name  # `order` indexes the INPUT list
        N = d["pos"].shape[0]
        rp = x["row_ptr"].long()
        assert torch.equal(rp[1:] - rp[:-1], torch.bincount(kept_ei[1], minlength=N)) and int(rp[-1]) == kept_ei.shape[1]
        assert bool((x["dst"][1:] >= x["dst"][:-1]).all())
        same = x["dst"][1:] == x["dst"][:-1]
        assert bool((x["order"][1:][same] > x["order"][:-1][same]).all()), name  # stable: input order inside a row
        assert torch.equal(x["src"][x["src_perm"].long()].long(), torch.sort(x["src"].long(), stable=True).values)
        sp = x["src_ptr"].long()
        assert torch.equal(sp[1:] - sp[:-1], torch.bincount(x["src"].long(), minlength=N))
        assert bool((x["offsets_bound"] >= 0).all()) and x["offsets_bound"].shape == x["offsets"].shape
        if kept_ei.shape[1]:
            assert float(x["offsets_bound"].max()) < 1e-5  # (a few ulps of a 4-20 A lattice vector)


def test_in_order_case_is_in_search_order_and_shuffled_case_is_not():
    d = gi.cases()["in order"]
    dst = d["edge_index"][1]
    assert bool((dst[1:] >= dst[:-1]).all())
    x = gi.expected("in order")
    assert bool(x["keep"].all()) and torch.equal(x["order"].long(), torch.arange(dst.numel()))  # nothing to move
    s = gi.cases()["shuffled"]
    dst = s["edge_index"][1]
    assert not bool((dst[1:] >= dst[:-1]).all())
    assert not torch.equal(gi.expected("shuffled")["order"].long(), torch.arange(dst.numel()))


def test_shuffled_case_straddles_a_pass_boundary_of_the_fill_kernel():
    from equiformer_amd.graph import EDGES_PASS
    assert EDGES_PASS == 256
    d, x = gi.cases()["shuffled"], gi.expected("shuffled")
    assert max(n for n in d["neighbors"].tolist()) > 2 * EDGES_PASS  # a structure walked in more than two passes
    dst = d["edge_index"][1].long()
    straddling, beyond_two = 0, 0
    for a0, a1 in _ranges(d):
        e = torch.arange(a0, a1)
        e = e[x["keep"][a0:a1]]
        passes = (e - a0) // EDGES_PASS
        for node in dst[e].unique().tolist():
            p = passes[dst[e] == node]
            straddling += int(p.min() != p.max())
            beyond_two += int(p.max() >= 2)
    print("shuffled: %d destinations with kept edges on both sides of a pass boundary, %d reach a third pass" % (straddling, beyond_two))
    assert straddling >= 1 and beyond_two >= 1
    rep, mult = pi.repeated_pairs(x["src"], x["dst"], d["pos"].shape[0])
    assert rep >= 1 and mult >= 2


def test_empty_structure_cases():
    d = gi.cases()["empty structure"]
    assert d["neighbors"].tolist() == [166, 0, 146]
    assert gi.cases()["empty structure first"]["neighbors"].tolist() == [0, 166, 146]
    assert gi.cases()["empty structure last"]["neighbors"].tolist() == [166, 146, 0]
    for name, lone in (("empty structure", 6), ("empty structure first", 0), ("empty structure last", 11)):
        rp = gi.expected(name)["row_ptr"].long()
        deg = rp[1:] - rp[:-1]
        assert int(deg[lone]) == 0 and int((deg == 0).sum()) == 1, name  # a node of in-degree 0


def test_dropped_case_drops_exactly_the_inserted_edges():
    d, x = gi.cases()["dropped"], gi.expected("dropped")
    a0, a1 = _ranges(d)[gi.DROP_STRUCTURE]
    dropped = (~x["keep"]).nonzero().view(-1).tolist()
    assert dropped == [a0, a0 + (a1 - a0) // 2, a1 - 1, d["edge_index"].shape[1] - 1], dropped  # first, middle, last + the lone atom's
    for e in dropped:
        assert int(d["edge_index"][0, e]) == int(d["edge_index"][1, e]) and not bool(d["cell_offsets"][e].any())
    assert d["natoms"][-1] == 1 and int(d["neighbors"][-1]) == 1
    rp = x["row_ptr"].long()
    assert int(rp[-1] - rp[-2]) == 0 and int(rp[-1]) == d["edge_index"].shape[1] - 4  # the lone atom's row: empty
    # self-loops with a non-zero image stay
    ei = d["edge_index"].long()
    loops = (ei[0] == ei[1]) & x["keep"]
    assert int(loops.sum()) >= 100 and bool(d["cell_offsets"][loops].any(dim=1).all())
    # no other edge is anywhere near zero length: the fp32 drop decision is the oracle's by construction
    assert float(x["lengths"][x["keep"]].min()) > 1e-3
    assert float(x["lengths"][~x["keep"]].max()) == 0.0


def test_truncated_case_has_full_rows_and_repeated_pairs():
    d, x = gi.cases()["truncated"], gi.expected("truncated")
    rp = x["row_ptr"].long()
    assert bool(((rp[1:] - rp[:-1]) == pi.DENSE_CAP).all()) and int(rp[-1]) == 36 * pi.DENSE_CAP
    rep, mult = pi.repeated_pairs(x["src"], x["dst"], 36)
    assert rep >= 1 and mult == 2


def test_no_edges_case():
    d, x = gi.cases()["no edges"], gi.expected("no edges")
    assert d["neighbors"].tolist() == [0, 0, 0] and d["edge_index"].shape == (2, 0)
    assert x["src"].numel() == 0 and x["row_ptr"].tolist() == [0, 0, 0, 0] and x["mol_ptr"].tolist() == [0, 1, 2, 3]


def test_slab_batches_with_edges_are_shuffled_inside_structures():
    bs = gi.slab_batches_with_edges(2)
    for d in bs:
        assert int(d["neighbors"].sum()) == d["edge_index"].shape[1] and d["neighbors"].shape == (4,)
        dst = d["edge_index"][1]
        assert not bool((dst[1:] >= dst[:-1]).all())
        for b, (a0, a1) in enumerate(_ranges(d)):
            assert bool((d["batch"][d["edge_index"][:, a0:a1]] == b).all())


# ------------------------------------------------------------------------------------------------------------------ the field check
def test_field_check_names_what_a_batch_lacks():
    from equiformer_amd.capture import GIVEN_EDGE_FIELDS, given_edge_fields
    assert GIVEN_EDGE_FIELDS == ("edge_index", "cell_offsets", "neighbors", "cell")
    d = gi.cases()["in order"]
    assert given_edge_fields(d) == GIVEN_EDGE_FIELDS
    assert given_edge_fields(SimpleNamespace(**d)) == GIVEN_EDGE_FIELDS
    for lacking in (("cell_offsets",), ("neighbors",), ("cell",), ("cell_offsets", "neighbors", "cell"), GIVEN_EDGE_FIELDS):
        for make in (dict, lambda m: SimpleNamespace(**m)):
            b = make({k: v for k, v in d.items() if k not in lacking})
            with pytest.raises(ValueError) as err:
                given_edge_fields(b)
            named = str(err.value).split(" missing")[0].split(": ")[-1].split(", ")
            assert named == [n for n in GIVEN_EDGE_FIELDS if n in lacking], (lacking, str(err.value))
    with pytest.raises(ValueError, match="neighbors missing"):
        given_edge_fields(dict(d, neighbors=None))
    # a non-periodic batch (no cell) is refused with edges="batch"
    with pytest.raises(ValueError, match="cell missing"):
        given_edge_fields({k: v for k, v in d.items() if k != "cell"})


def test_keywords_exist_and_default_to_the_search():
    from equiformer_amd import capture, evaluate, synthetic
    from equiformer_amd.graph import EdgeGraph
    for cls in (capture.BucketedTrainStep, evaluate.BucketedEvalStep):
        assert inspect.signature(cls.__init__).parameters["edges"].default == "search"
    assert inspect.signature(capture._BucketedStep._init_buckets).parameters["edges"].default == "search"
    step = capture._BucketedStep()
    with pytest.raises(ValueError, match="edges"):
        step._init_buckets(5.0, ("y",), (), 1, 1, 64, 1024, 50, edges="given")
    step._init_buckets(5.0, ("y",), (), 1, 1, 64, 1024, 50, edges="batch")
    with pytest.raises(ValueError, match="cell_offsets, neighbors missing"):
        step._check_periodic({k: v for k, v in gi.cases()["in order"].items() if k not in ("cell_offsets", "neighbors")})
    assert list(inspect.signature(EdgeGraph.edges_pbc_plan).parameters) == ["pos", "cell", "batch", "edge_index", "cell_offsets",
                                                                            "neighbors", "num_graphs"]
    assert list(inspect.signature(EdgeGraph.from_edges_pbc_plan).parameters) == ["plan", "capacity", "into", "z"]
    assert {"into", "capacity", "z", "num_graphs"} <= set(inspect.signature(EdgeGraph.from_edges_pbc).parameters)
    assert callable(synthetic.attach_given_edges)
    d = gi.cases()["in order"]
    from equiformer_amd import ops
    with pytest.raises(ops.HipOnlyError):  # the builder runs on the GPU only
        EdgeGraph.edges_pbc_plan(d["pos"], d["cell"], d["batch"], d["edge_index"], d["cell_offsets"], d["neighbors"])


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_prototypes_in_the_header_and_the_binding_table():
    from equiformer_amd import lib
    text = open(os.path.join(ROOT, "include", "equiformer_hip.h")).read()
    assert "nets/graph_attention_transformer_oc20.py:280-293" in text and "oracle/pbc.py:get_pbc_distances" in text
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    for name, n in (("eqf_edges_pbc_count", 16), ("eqf_edges_pbc_fill", 19)):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S)
        assert m, "%s is not declared in include/equiformer_hip.h" % name
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        sig = lib.SIGNATURES[name]
        assert len(args) == len(sig) == n, (name, len(args), len(sig))
        for a, t in zip(args, sig):
            assert t is (ctypes.c_void_p if "*" in a else ctypes.c_int), (name, a, t)


def test_library_exports_the_entry_points_and_refuses_bad_arguments_on_the_host(hip_lib):
    one = ctypes.c_void_p(64)
    count, fill = hip_lib.eqf_edges_pbc_count, hip_lib.eqf_edges_pbc_fill
    assert count(one, one, None, one, 1, 4, one, 1, one, 1, 8, one, one, one, one, None) != 0      # no mol_ptr
    assert count(one, one, one, one, 1, 4, one, 1, one, 1, 8, one, one, one, None, None) != 0      # no status word
    assert count(one, one, one, one, 1, 4, None, 1, one, 1, 8, one, one, one, one, None) != 0      # edges without edge_index
    assert count(one, one, one, one, 1, 4, one, 1, one, 1, -1, one, one, one, one, None) != 0      # a negative edge count
    assert fill(one, one, 1, 8, one, 1, one, 1, 8, one, one, None, 8, one, one, one, one, one, None) != 0   # no row_ptr
    assert fill(one, one, 1, 8, one, 1, one, 1, 8, one, one, one, 8, one, one, one, one, None, None) != 0   # no order
    assert fill(one, one, 1, 8, one, 1, one, 1, 8, one, one, one, 9, one, one, one, one, one, None) != 0    # more kept than given
    assert fill(one, one, 1, 16385, one, 1, one, 1, 8, one, one, one, 8, one, one, one, one, one, None) != 0  # beyond the LDS cursors
    assert fill(one, one, 0, 8, one, 1, one, 1, 8, one, one, one, 8, one, one, one, one, one, None) == 0    # no structure: no launch
    assert fill(one, one, 3, 8, one, 1, one, 1, 0, None, None, one, 0, None, None, None, None, None, None) == 0  # no edge: no launch
