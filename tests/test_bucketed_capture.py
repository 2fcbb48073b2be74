"""Host side of the shape-bucketed captured train step (equiformer_amd/capture.py BucketedTrainStep): the bucket policy, the
binding of eqf_graph_pad_tail, the varying-batch generator, and the eager-step counter of CapturedTrainStep.  No GPU."""
import ctypes
import gc
import os
import random
import re
import weakref

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_min_phantom_nodes_is_the_smallest_count_with_enough_ordered_pairs():
    from equiformer_amd.graph import min_phantom_nodes
    assert min_phantom_nodes(0) == 0
    for q in list(range(1, 400)) + [1023, 1024, 4095, 10 ** 6]:
        p = min_phantom_nodes(q)
        assert p * (p - 1) >= q and (p - 1) * (p - 2) < q, (q, p)


def test_bucket_of_is_monotone_idempotent_on_its_corner_and_reserves_the_phantom_nodes():
    from equiformer_amd.capture import bucket_corner, bucket_of
    from equiformer_amd.graph import min_phantom_nodes
    rnd = random.Random(0)
    for node_step, edge_step in ((64, 1024), (16, 128), (1, 1), (7, 300), (128, 2048)):
        p_res = min_phantom_nodes(edge_step - 1)
        for _ in range(300):
            B, N, E = rnd.randint(1, 256), rnd.randint(1, 5000), rnd.randint(0, 60000)
            key = bucket_of(B, N, E, node_step, edge_step)
            assert key[0] == B and key[1] % node_step == 0 and key[2] % edge_step == 0
            # fits, with room for the phantom edges it implies; and not a whole step too large
            P, Q = key[1] - N, key[2] - E
            assert 0 <= Q < edge_step and P >= p_res >= min_phantom_nodes(Q)
            assert P < p_res + node_step
            # monotone in N and in E
            k2 = bucket_of(B, N + rnd.randint(0, 200), E + rnd.randint(0, 3000), node_step, edge_step)
            assert k2[1] >= key[1] and k2[2] >= key[2]
            # the bucket's own corner (its largest real shape) maps to the bucket; one more node or edge does not
            n_max, e_max = bucket_corner(key, node_step, edge_step)
            assert bucket_of(B, n_max, e_max, node_step, edge_step) == key
            assert bucket_of(B, n_max + 1, e_max, node_step, edge_step)[1] == key[1] + node_step
            assert bucket_of(B, n_max, e_max + 1, node_step, edge_step)[2] == key[2] + edge_step
    with pytest.raises(ValueError):
        bucket_of(1, 1, 1, 0, 1)


def test_distinct_buckets_around_the_qm9_bench_shape_are_what_the_step_sizes_imply():
    """1 000 random (N, E) around the QM9 bench batch (N = 2 304, E = 25 354): the distinct buckets are exactly the cells of the
    (node_step, edge_step) grid that the samples' own ranges touch -- counted here from the step sizes, not a constant."""
    from equiformer_amd.capture import DEFAULT_EDGE_STEP, DEFAULT_NODE_STEP, bucket_of
    from equiformer_amd.graph import min_phantom_nodes
    rnd = random.Random(1)
    pts = [(int(rnd.gauss(2304, 45)), int(rnd.gauss(25354, 1000))) for _ in range(1000)]
    for node_step, edge_step in ((DEFAULT_NODE_STEP, DEFAULT_EDGE_STEP), (32, 512), (128, 4096)):
        p_res = min_phantom_nodes(edge_step - 1)
        cells = {(-(-(n + p_res) // node_step), -(-e // edge_step)) for n, e in pts}
        keys = {bucket_of(128, n, e, node_step, edge_step) for n, e in pts}
        assert len(keys) == len(cells)
        assert keys == {(128, a * node_step, b * edge_step) for a, b in cells}
        n_lo, n_hi = min(n for n, _ in pts), max(n for n, _ in pts)
        e_lo, e_hi = min(e for _, e in pts), max(e for _, e in pts)
        assert len(keys) <= ((n_hi - n_lo) // node_step + 2) * ((e_hi - e_lo) // edge_step + 2)
    # the defaults keep the padding small at the bench shape: <= 4 % of the edges, <= 4.2 % of the nodes
    assert (DEFAULT_EDGE_STEP - 1) / 25354 < 0.041
    assert (min_phantom_nodes(DEFAULT_EDGE_STEP - 1) + DEFAULT_NODE_STEP - 1) / 2304 < 0.042


def test_pad_tail_prototype_in_the_binding_table_matches_the_header():
    from equiformer_amd import lib
    text = open(os.path.join(ROOT, "include", "equiformer_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+eqf_graph_pad_tail\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert m, "eqf_graph_pad_tail is not declared in include/equiformer_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    sig = lib.SIGNATURES["eqf_graph_pad_tail"]
    assert len(args) == len(sig) == 15
    for a, t in zip(args, sig):
        if "*" in a:
            assert t is ctypes.c_void_p, (a, t)
        else:
            assert a.startswith("int ") and t is ctypes.c_int, (a, t)
    assert args[-1] == "void* stream"
    assert [a.split()[-1].lstrip("*") for a in args[:5]] == ["n", "e", "n_cap", "e_cap", "n_mol"]


def test_library_exports_pad_tail(hip_lib):
    assert hasattr(hip_lib, "eqf_graph_pad_tail")
    # bad arguments are refused on the host, before any launch (no GPU needed): missing tensors, counts over the capacity,
    # more phantom edges than P (P - 1) ordered pairs
    one = ctypes.c_void_p(64)
    f = hip_lib.eqf_graph_pad_tail
    assert f(4, 4, 8, 8, 1, None, one, one, one, one, None, None, None, None, None) != 0
    assert f(9, 4, 8, 8, 1, one, one, one, one, one, None, None, None, None, None) != 0
    assert f(4, 9, 8, 8, 1, one, one, one, one, one, None, None, None, None, None) != 0
    assert f(6, 0, 8, 3, 1, one, one, one, one, one, None, None, None, None, None) != 0  # P = 2, Q = 3 > 2


def test_captured_train_step_counts_eager_steps_without_keeping_the_graph_alive():
    """CapturedTrainStep._seen stored (count, EdgeGraph) per shape: every shape ever seen kept its index tensors for ever."""
    from equiformer_amd.capture import CapturedTrainStep

    class Opt:
        _reducer = None
        flat_p = torch.zeros(1)

        def zero_grad(self, set_to_none=True):
            pass

        def step(self):
            pass

    class G:
        N, E = 5, 7

    cs = CapturedTrainStep.__new__(CapturedTrainStep)  # (the constructor pins host memory: needs a GPU runtime)
    cs.opt, cs.min_eager, cs.max_graphs = Opt(), 3, 4
    cs._graphs, cs._seen, cs.replays, cs.eager_steps = {}, {}, 0, 0
    cs.forward_loss = lambda g: torch.zeros((), requires_grad=True) * 1.0
    g = G()
    ref = weakref.ref(g)
    cs.step(lambda into: g)
    assert cs.eager_steps == 1 and cs._seen == {(5, 7): 1}
    del g
    gc.collect()
    assert ref() is None, "CapturedTrainStep keeps the EdgeGraph of an eager step alive"
    cs.step(lambda into: G())
    assert cs._seen == {(5, 7): 2}


def test_varying_batches_generator():
    from equiformer_amd.synthetic import qm9_like_batch, qm9_like_varying_batches
    bs = qm9_like_varying_batches(5, 6, (9, 15), side=5.5, seed=0)
    assert len(bs) == 5
    totals = set()
    for d in bs:
        n = d["pos"].shape[0]
        assert d["num_graphs"] == 6 and d["y"].shape == (6,) and d["z"].shape == (n,) and d["batch"].shape == (n,)
        assert int(d["natoms"].sum()) == n and int(d["natoms"].min()) >= 9 and int(d["natoms"].max()) <= 15
        assert torch.equal(torch.bincount(d["batch"], minlength=6), d["natoms"])
        assert bool((d["batch"][1:] >= d["batch"][:-1]).all())
        assert len(set(d["natoms"].tolist())) > 1  # different sizes inside a batch
        totals.add(n)
    assert len(totals) > 1  # different totals between batches
    again = qm9_like_varying_batches(5, 6, (9, 15), side=5.5, seed=0)
    assert all(torch.equal(a["pos"], b["pos"]) for a, b in zip(bs, again))
    # the existing generator is untouched
    d = qm9_like_batch(2, 18, seed=0)
    assert d["pos"].shape == (36, 3)


def test_bucketed_train_step_refuses_a_reducer():
    from equiformer_amd.capture import BucketedTrainStep

    class Opt:
        _reducer = object()

    with pytest.raises(ValueError):
        BucketedTrainStep(Opt(), lambda g, v: None, 5.0)
