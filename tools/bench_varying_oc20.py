#!/usr/bin/env python
"""OC20 train-step rate over periodic batches whose atom and edge counts change every step (what an OC20 loader yields), one MI355X:

    python tools/bench_varying_oc20.py [--batches 48] [--regions 3] [--out profiles/oc20_varying.json]

The full OC20 model of bench.py (oc20_l1_256_nonlinear, 16 structures per batch, r = 5, max_neighbors = 500), slab structures of
60-96 atoms in the 11 x 11 x 30 A cell so that N and E scatter around the bench shape (16 x 78 atoms).  From ONE process and ONE
build, real structures/s of
  (a) `bucketed`:   equiformer_amd.capture.BucketedTrainStep (batch padded to its bucket, one HIP graph per bucket),
  (b) `eager`:      the plain eager step on the same, unpadded batches (`model(data)`: the model builds its periodic graph),
  (c) `eager_sort`: (b) with the by-source view of the graph taken from torch.argsort + torch.bincount, as before
                    eqf_csr_by_source_multi existed (the new kernel's few microseconds are spent as well: an upper bound of the old step),
each as `--regions` timed regions of one pass over all batches (synchronised wall clock), the legs alternating.  Before the
timed regions every leg runs untimed passes until its graphs exist (bucketed: min_eager + 1 passes).  Also times, with device
events on the bench batch (16 x 78 atoms), eqf_csr_by_source_multi against the argsort + bincount it replaces.  Prints one JSON
line."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODEL = "oc20_l1_256_nonlinear"
RADIUS, MAX_NEIGHBORS = 5.0, 500


def _median(v):
    return sorted(v)[len(v) // 2]


def time_by_source(dev, iters=200, regions=5):
    """microseconds per call on the bench batch: the cursor kernel vs the sort path (argsort + int32 cast + bincount + cumsum + cat)"""
    from equiformer_amd.graph import EdgeGraph, _P, _i32, _ptr_from_counts, _stream
    from equiformer_amd.lib import call
    from equiformer_amd.synthetic import oc20_like_varying_batches
    d = oc20_like_varying_batches(1, 16, (78, 78), seed=1000)[0]
    g, _, _ = EdgeGraph.from_radius_pbc(d["pos"].to(dev), d["cell"].to(dev), d["batch"].to(dev), RADIUS, MAX_NEIGHBORS, 16)
    perm, ptr = torch.empty_like(g.src_perm), torch.empty_like(g.src_ptr)

    def kernel():
        call("eqf_csr_by_source_multi", _P(g.src), _P(g.row_ptr), _P(g.mol_ptr), 16, 78, _P(perm), _P(ptr), _stream())

    def sort():
        order = torch.argsort(g.src.to(torch.int64), stable=True)
        return _i32(order), _ptr_from_counts(torch.bincount(g.src.to(torch.int64), minlength=g.N))

    kernel()
    p2, q2 = sort()
    assert torch.equal(perm, p2) and torch.equal(ptr, q2)
    out = {"nodes": g.N, "edges": g.E, "iters": iters}
    for name, fn in (("kernel_us", kernel), ("sort_us", sort)):
        vals = []
        for _ in range(regions):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            vals.append(a.elapsed_time(b) * 1e3 / iters)
        out[name] = {"value": _median(vals), "values": vals}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--structures", type=int, default=16)
    ap.add_argument("--atoms-min", type=int, default=60)
    ap.add_argument("--atoms-max", type=int, default=96)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--node-step", type=int, default=64)
    ap.add_argument("--edge-step", type=int, default=2048)
    ap.add_argument("--max-graphs", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_varying_oc20.py needs an MI355X"
    from equiformer_amd import capture, lib, nets
    from equiformer_amd.graph import EdgeGraph, _i32, _ptr_from_counts
    from equiformer_amd.optim import FlatAdamW, add_weight_decay
    from equiformer_amd.synthetic import oc20_like_varying_batches
    lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B = args.structures
    model = nets.model_entrypoint(MODEL)().to(dev).train()
    opt = FlatAdamW(add_weight_decay(model, 1e-3, model.no_weight_decay()), lr=2e-4)
    to_dev = lambda d: {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}  # noqa: E731
    batches = [to_dev(d) for d in oc20_like_varying_batches(args.batches, B, (args.atoms_min, args.atoms_max), seed=1000)]

    def data_of(d):
        return SimpleNamespace(pos=d["pos"], batch=d["batch"], atomic_numbers=d["atomic_numbers"], tags=d["tags"], cell=d["cell"],
                               natoms=d["natoms"])

    # (b) eager, unpadded: the model builds its graph
    def eager_step(d):
        opt.zero_grad(set_to_none=True)
        loss = (model(data_of(d)).squeeze(-1) - d["y"]).abs().mean()
        loss.backward()
        opt.step()
        return loss.detach()

    # (c) eager with the sorted by-source view
    def eager_sort_step(d):
        opt.zero_grad(set_to_none=True)
        g, offsets, _ = EdgeGraph.from_radius_pbc(d["pos"], d["cell"], d["batch"], RADIUS, MAX_NEIGHBORS, B)
        g.src_perm = _i32(torch.argsort(g.src.to(torch.int64), stable=True))
        g.src_ptr = _ptr_from_counts(torch.bincount(g.src.to(torch.int64), minlength=g.N))
        loss = (model(data_of(d), graph=g, offsets=offsets).squeeze(-1) - d["y"]).abs().mean()
        loss.backward()
        opt.step()
        return loss.detach()

    # (a) bucketed
    def padded_loss(g, v):
        return (model(v, graph=g, offsets=v.offsets).squeeze(-1)[:v.B] - v.y[:v.B]).abs().mean()
    bs = capture.BucketedTrainStep(opt, padded_loss, RADIUS, graph_targets=("y",), node_targets=("tags",),
                                   max_num_neighbors=MAX_NEIGHBORS, node_step=args.node_step, edge_step=args.edge_step,
                                   max_graphs=args.max_graphs)

    legs = [("eager", eager_step), ("bucketed", bs.step), ("eager_sort", eager_sort_step)]

    def one_pass(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for d in batches:
            step(d)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    by_source = time_by_source(dev)
    # warm-up: clocks, allocator pools, lazily built tables; then every bucket's graph (min_eager eager steps + the capture)
    one_pass(eager_step)
    one_pass(eager_sort_step)
    torch.cuda.synchronize()
    mem0 = (torch.cuda.memory_allocated(), torch.cuda.memory_reserved())
    t_cap0 = time.perf_counter()
    for _ in range(bs.min_eager + 1):
        one_pass(bs.step)
    t_cap = time.perf_counter() - t_cap0
    torch.cuda.synchronize()
    mem1 = (torch.cuda.memory_allocated(), torch.cuda.memory_reserved())
    n_live = max(1, len(bs.live_graphs()))
    warm = dict(replays=bs.replays, eager_steps=bs.eager_steps, captures=bs.captures, evictions=bs.evictions)

    times = {name: [] for name, _ in legs}
    for _ in range(args.regions):
        for name, step in legs:  # alternating: a drift of the box's clocks reaches every leg alike
            times[name].append(one_pass(step))
    units = B * len(batches)
    rate = {name: [units / t for t in ts] for name, ts in times.items()}
    plans = [EdgeGraph.radius_pbc_plan(d["pos"], d["cell"], d["batch"], RADIUS, MAX_NEIGHBORS, B) for d in batches]
    sizes = [(p.N, p.E) for p in plans]
    keys = [capture.bucket_of(B, n, e, bs.node_step, bs.edge_step) for n, e in sizes]
    out = {
        "what": "OC20 %s train step over %d different batches of %d slab structures (%d-%d atoms, 11 x 11 x 30 A cell), r=%.1f, "
                "max_neighbors=%d, split mode; structures/s of real structures, one timed region = one pass over all batches, "
                "synchronised wall clock" % (MODEL, len(batches), B, args.atoms_min, args.atoms_max, RADIUS, MAX_NEIGHBORS),
        "build": lib.built_hash(),
        "unit": "structures/s",
        "regions": args.regions,
        "bucketed": {"value": _median(rate["bucketed"]), "values": rate["bucketed"]},
        "eager": {"value": _median(rate["eager"]), "values": rate["eager"]},
        "eager_sort": {"value": _median(rate["eager_sort"]), "values": rate["eager_sort"]},
        "eager_spread": (max(rate["eager"]) - min(rate["eager"])) / min(rate["eager"]),
        "eager_sort_spread": (max(rate["eager_sort"]) - min(rate["eager_sort"])) / min(rate["eager_sort"]),
        "bucketed_over_eager": min(rate["bucketed"]) / max(rate["eager"]),
        "bucketed_over_eager_sort": min(rate["bucketed"]) / max(rate["eager_sort"]),
        "by_source": by_source,
        "nodes": {"min": min(n for n, _ in sizes), "max": max(n for n, _ in sizes), "mean": sum(n for n, _ in sizes) / len(sizes)},
        "edges": {"min": min(e for _, e in sizes), "max": max(e for _, e in sizes), "mean": sum(e for _, e in sizes) / len(sizes)},
        "node_step": bs.node_step, "edge_step": bs.edge_step, "min_eager": bs.min_eager, "max_graphs": bs.max_graphs,
        "buckets_hit": len(set(keys)),
        "live_graphs": len(bs.live_graphs()),
        "warmup": dict(warm, seconds=t_cap, passes=bs.min_eager + 1),
        "timed": {"replays": bs.replays - warm["replays"], "eager_steps": bs.eager_steps - warm["eager_steps"],
                  "captures": bs.captures - warm["captures"], "evictions": bs.evictions - warm["evictions"]},
        "padded_edge_share": 1.0 - bs.real_edges / bs.padded_edges,
        "padded_node_share": 1.0 - bs.real_nodes / bs.padded_nodes,
        "bytes_per_live_graph": {"allocated": (mem1[0] - mem0[0]) / n_live, "reserved": (mem1[1] - mem0[1]) / n_live},
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
