"""Host side of the captured periodic (OC20) train step: the varying-batch generator, the binding of
eqf_csr_by_source_multi, the new keyword arguments, and -- with oracle/pbc.py on the CPU -- that the inputs of
tests/test_gpu_periodic_capture.py really hold what they are meant to exercise: (source, destination) pairs that repeat
(one edge per periodic image) and rows truncated to max_neighbors.  No GPU."""
import ctypes
import inspect
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import periodic_inputs as pi  # noqa: E402


def test_oc20_varying_batches_generator():
    from equiformer_amd.synthetic import oc20_like_varying_batches
    bs = oc20_like_varying_batches(5, 4, (20, 36), cell=(8.0, 8.0, 20.0), seed=0)
    assert len(bs) == 5
    totals = set()
    for d in bs:
        n = d["pos"].shape[0]
        assert d["num_graphs"] == 4 and d["y"].shape == (4,) and d["cell"].shape == (4, 3, 3)
        assert d["atomic_numbers"].shape == d["tags"].shape == d["batch"].shape == (n,) and d["pos"].shape == (n, 3)
        assert d["pos"].dtype == torch.float32 and d["atomic_numbers"].dtype == d["tags"].dtype == d["batch"].dtype == torch.int64
        assert int(d["natoms"].sum()) == n and int(d["natoms"].min()) >= 20 and int(d["natoms"].max()) <= 36
        assert torch.equal(torch.bincount(d["batch"], minlength=4), d["natoms"])
        assert bool((d["batch"][1:] >= d["batch"][:-1]).all())
        assert len(set(d["natoms"].tolist())) > 1  # different sizes inside a batch
        assert 1 <= int(d["atomic_numbers"].min()) and int(d["atomic_numbers"].max()) <= 83
        assert 0 <= int(d["tags"].min()) and int(d["tags"].max()) <= 2
        # slab shape: orthorhombic cell, every atom inside it and in its lower 45 %
        assert torch.equal(d["cell"], torch.diag(torch.tensor([8.0, 8.0, 20.0]))[None].repeat(4, 1, 1))
        assert float(d["pos"].min()) >= 0.0 and float(d["pos"][:, :2].max()) <= 8.0 and float(d["pos"][:, 2].max()) <= 0.45 * 20.0
        totals.add(n)
    assert len(totals) > 1  # different totals between batches
    again = oc20_like_varying_batches(5, 4, (20, 36), cell=(8.0, 8.0, 20.0), seed=0)
    assert all(torch.equal(a[k], b[k]) for a, b in zip(bs, again) for k in ("pos", "atomic_numbers", "tags", "batch", "y"))
    other = oc20_like_varying_batches(5, 4, (20, 36), cell=(8.0, 8.0, 20.0), seed=1)
    assert any(a["pos"].shape != b["pos"].shape or not torch.equal(a["pos"], b["pos"]) for a, b in zip(bs, other))
    # the defaults are the bench shape's surroundings: 11 x 11 x 30 A, 60-96 atoms
    d = oc20_like_varying_batches(1, 16, seed=2)[0]
    assert d["cell"][0].diagonal().tolist() == [11.0, 11.0, 30.0] and 60 <= int(d["natoms"].min()) <= int(d["natoms"].max()) <= 96


def _oracle(d, cap):
    from oracle import pbc
    ei, off, nb = pbc.radius_graph_pbc(d["pos"], d["cell"], [int(n) for n in d["natoms"]], pi.R, cap)
    return ei, torch.bincount(ei[1], minlength=d["pos"].shape[0])


def test_gpu_test_inputs_hold_repeated_pairs_and_truncated_rows():
    for name, d, cap in (("triclinic", pi.small_triclinic(), 500), ("triclinic, other seed", pi.small_triclinic(seed=11), 500),
                         ("cubic", pi.small_cubic(), 50), ("with an empty structure", pi.with_an_empty_structure(), 50)):
        ei, deg = _oracle(d, cap)
        rep, mult = pi.repeated_pairs(ei[0], ei[1], d["pos"].shape[0])
        print("%s: %d edges, %d repeated pairs, multiplicity up to %d" % (name, ei.shape[1], rep, mult))
        assert rep >= 1 and mult >= 2
        assert int(deg.max()) <= cap
    # the capped variant: rows truncated, pairs still repeat
    d = pi.small_triclinic()
    ei, deg = _oracle(d, 12)
    _, deg_full = _oracle(d, 10 ** 6)
    assert int((deg < deg_full).sum()) >= 1 and int(deg.max()) == 12
    assert pi.repeated_pairs(ei[0], ei[1], 21)[0] >= 1
    # a structure without any edge, between two that have some
    d = pi.with_an_empty_structure()
    _, deg = _oracle(d, 50)
    assert int(deg[6]) == 0 and int(deg[:6].min()) > 0 and int(deg[7:].min()) > 0


def test_dense_cells_keep_their_edge_count_under_jitter_and_change_their_edge_list():
    """the exact-shape capture test needs batches of ONE (nodes, edges) shape with different graphs: every row truncated"""
    base, _ = _oracle(pi.dense_cells(), pi.DENSE_CAP)
    lists = [base]
    for j in range(1, 4):
        d = pi.dense_cells(jitter=0.05, jitter_seed=j)
        ei, deg = _oracle(d, pi.DENSE_CAP)
        _, deg_full = _oracle(d, 10 ** 6)
        assert bool((deg == pi.DENSE_CAP).all()) and bool((deg_full > pi.DENSE_CAP).all())
        assert ei.shape == base.shape
        lists.append(ei)
    assert any(not torch.equal(a, base) for a in lists[1:])
    assert pi.repeated_pairs(base[0], base[1], 36)[0] >= 1


def test_slab_batches_vary_and_repeat_pairs():
    sizes = set()
    for d in pi.slab_batches(12):
        ei, _ = _oracle(d, pi.SLAB_CAP)
        assert pi.repeated_pairs(ei[0], ei[1], d["pos"].shape[0])[0] >= 1
        sizes.add((d["pos"].shape[0], ei.shape[1]))
    assert len(sizes) >= 10  # nearly every batch has its own (nodes, edges)


def test_by_source_multi_prototype_in_the_binding_table_matches_the_header():
    from equiformer_amd import lib
    text = open(os.path.join(ROOT, "include", "equiformer_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    protos = {}
    for name in ("eqf_csr_by_source", "eqf_csr_by_source_multi"):
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S)
        assert m, "%s is not declared in include/equiformer_hip.h" % name
        protos[name] = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert protos["eqf_csr_by_source_multi"] == protos["eqf_csr_by_source"]  # the same arguments
    sig = lib.SIGNATURES["eqf_csr_by_source_multi"]
    assert sig == lib.SIGNATURES["eqf_csr_by_source"] and len(sig) == len(protos["eqf_csr_by_source_multi"]) == 8
    for a, t in zip(protos["eqf_csr_by_source_multi"], sig):
        assert t is (ctypes.c_void_p if "*" in a else ctypes.c_int), (a, t)


def test_library_exports_by_source_multi_and_refuses_bad_arguments_on_the_host(hip_lib):
    assert hasattr(hip_lib, "eqf_csr_by_source_multi")
    one = ctypes.c_void_p(64)
    f = hip_lib.eqf_csr_by_source_multi
    assert f(None, one, one, 1, 8, one, one, None) != 0
    assert f(one, one, one, 1, 8, None, one, None) != 0
    assert f(one, one, one, 1, 16385, one, one, None) != 0  # more nodes per structure than the LDS cursors hold
    assert f(one, one, one, 0, 8, one, one, None) == 0      # no structure: nothing to launch


def test_new_keyword_arguments_exist_and_the_builders_stay_gpu_only():
    from equiformer_amd import ops
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20
    p = inspect.signature(EdgeGraph.from_radius_pbc).parameters
    assert list(p)[:6] == ["pos", "cell", "batch", "r", "max_num_neighbors", "num_graphs"] and p["max_num_neighbors"].default == 50
    assert [p[k].default for k in ("into", "capacity", "z")] == [None, None, None]
    assert list(inspect.signature(EdgeGraph.from_radius_pbc_plan).parameters) == ["plan", "capacity", "into", "z"]
    f = inspect.signature(GraphAttentionTransformerOC20.forward).parameters
    assert list(f) == ["self", "data", "graph", "offsets"] and f["graph"].default is None and f["offsets"].default is None
    d = pi.small_cubic()
    with pytest.raises(ops.HipOnlyError):
        EdgeGraph.from_radius_pbc(d["pos"], d["cell"], d["batch"], pi.R)
    with pytest.raises(ops.HipOnlyError):
        EdgeGraph.radius_pbc_plan(d["pos"], d["cell"], d["batch"], pi.R)


def test_package_does_not_import_bench():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "equiformer_amd")):
        for f in files:
            if f.endswith(".py"):
                assert not re.search(r"^\s*(from|import)\s+bench\b", open(os.path.join(dirpath, f)).read(), re.M), f
