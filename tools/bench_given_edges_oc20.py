#!/usr/bin/env python
"""OC20 batches that bring their own edge list (the reference's otf_graph=False: what an OC20 LMDB delivers), one MI355X:

    python tools/bench_given_edges_oc20.py [--batches 48] [--regions 5] [--out profiles/oc20_given_edges.json]

The 48 batches of 16 slab structures of tools/bench_varying_oc20.py (60-96 atoms, 11 x 11 x 30 A cell) with `edge_index`,
`cell_offsets` (int64) and `neighbors` attached from the GPU search at r = 5, max_neighbors = 50
(equiformer_amd.synthetic.attach_given_edges); the full model of bench.py (oc20_l1_256_nonlinear) with otf_graph=False.  From ONE
process and ONE build, per batch (p10 / median / p90 over the batches of each batch's median over `--regions` regions):
  (a) the graph build alone, microseconds, device events around `--iters` calls:
        `build_parent`: the model's `_graph` -- repeat_interleave, bmm, the zero-length test with its read-back, EdgeGraph.from_edges
                        (argsort, bincount, cumsum) and the by-source device sort;
        `build_new`:    EdgeGraph.from_edges_pbc (eqf_edges_pbc_count / _fill, eqf_csr_by_source_multi, one read-back);
        `build_refill`: the same `into=` a graph of the batch (what a replayed step pays);
  (b) `step_eager`:    the eager train step `model(data)`, milliseconds, synchronised wall clock;
  (c) `step_bucketed`: the same step through BucketedTrainStep(edges="batch"), milliseconds, after every bucket has its graph.
The legs of (b) and (c) alternate inside a region.  Prints one JSON line."""
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
RADIUS, MAX_NEIGHBORS = 5.0, 50


def _median(v):
    return sorted(v)[len(v) // 2]


def _quantiles(v):
    s = sorted(v)
    pick = lambda q: s[min(len(s) - 1, int(q * len(s)))]  # noqa: E731
    return {"p10": pick(0.10), "median": pick(0.50), "p90": pick(0.90), "n": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--structures", type=int, default=16)
    ap.add_argument("--atoms-min", type=int, default=60)
    ap.add_argument("--atoms-max", type=int, default=96)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--node-step", type=int, default=64)
    ap.add_argument("--edge-step", type=int, default=2048)
    ap.add_argument("--max-graphs", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_given_edges_oc20.py needs an MI355X"
    from equiformer_amd import capture, lib, nets
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW, add_weight_decay
    from equiformer_amd.synthetic import attach_given_edges, oc20_like_varying_batches
    lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B = args.structures
    model = nets.model_entrypoint(MODEL)(otf_graph=False, max_neighbors=MAX_NEIGHBORS).to(dev).train()
    opt = FlatAdamW(add_weight_decay(model, 1e-3, model.no_weight_decay()), lr=2e-4)
    to_dev = lambda d: {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}  # noqa: E731
    batches = [attach_given_edges(to_dev(d), RADIUS, MAX_NEIGHBORS)
               for d in oc20_like_varying_batches(args.batches, B, (args.atoms_min, args.atoms_max), seed=1000)]

    def data_of(d):
        return SimpleNamespace(pos=d["pos"], batch=d["batch"], atomic_numbers=d["atomic_numbers"], tags=d["tags"], cell=d["cell"],
                               natoms=d["natoms"], edge_index=d["edge_index"], cell_offsets=d["cell_offsets"], neighbors=d["neighbors"])

    def new_build(d, into=None):
        return EdgeGraph.from_edges_pbc(d["pos"], d["cell"], d["batch"], d["edge_index"], d["cell_offsets"], d["neighbors"], B,
                                        into=into)[0]

    # ---- (a) the graph build alone
    def events(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / args.iters

    build = {"build_parent": [], "build_new": [], "build_refill": []}
    for d in batches:
        data, pos = data_of(d), d["pos"]
        g_parent, off_parent = model._graph(data, pos, d["batch"])
        g_new = new_build(d)
        assert torch.equal(g_parent.src, g_new.src) and torch.equal(g_parent.src_perm, g_new.src_perm)  # (also the warm-up)
        assert float((off_parent - g_new.offsets).abs().max()) < 1e-5
        legs = (("build_parent", lambda: model._graph(data, pos, d["batch"])), ("build_new", lambda: new_build(d)),
                ("build_refill", lambda: new_build(d, into=g_new)))
        vals = {name: [] for name, _ in legs}
        for _ in range(args.regions):
            for name, fn in legs:
                vals[name].append(events(fn))
        for name in vals:
            build[name].append(_median(vals[name]))

    # ---- (b), (c) the train step
    def eager_step(d):
        opt.zero_grad(set_to_none=True)
        loss = (model(data_of(d)).squeeze(-1) - d["y"]).abs().mean()
        loss.backward()
        opt.step()
        return loss.detach()

    def padded_loss(g, v):
        return (model(v, graph=g, offsets=v.offsets).squeeze(-1)[:v.B] - v.y[:v.B]).abs().mean()
    bs = capture.BucketedTrainStep(opt, padded_loss, RADIUS, graph_targets=("y",), node_targets=("tags",),
                                   max_num_neighbors=MAX_NEIGHBORS, node_step=args.node_step, edge_step=args.edge_step,
                                   max_graphs=args.max_graphs, edges="batch")

    def timed(step, d):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(d)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for d in batches:  # warm-up: clocks, allocator pools, lazily built tables; then every bucket's graph
        eager_step(d)
    for _ in range(bs.min_eager + 1):
        for d in batches:
            bs.step(d)
    warm = dict(replays=bs.replays, eager_steps=bs.eager_steps, captures=bs.captures, evictions=bs.evictions)
    step = {"step_eager": [[] for _ in batches], "step_bucketed": [[] for _ in batches]}
    for _ in range(args.regions):
        for i, d in enumerate(batches):  # alternating: a drift of the clocks reaches both legs alike
            step["step_eager"][i].append(timed(eager_step, d))
            step["step_bucketed"][i].append(timed(bs.step, d))
    per_batch = {name: [_median(v) for v in vals] for name, vals in step.items()}
    sizes = [(int(d["pos"].shape[0]), int(d["edge_index"].shape[1])) for d in batches]
    out = {
        "what": "OC20 %s with otf_graph=False over %d batches of %d slab structures (%d-%d atoms, 11 x 11 x 30 A cell) that carry "
                "edge_index / cell_offsets / neighbors from the search at r=%.1f, max_neighbors=%d; per-batch medians over %d "
                "regions, their p10 / median / p90 over the batches" % (MODEL, len(batches), B, args.atoms_min, args.atoms_max,
                                                                        RADIUS, MAX_NEIGHBORS, args.regions),
        "build": lib.built_hash(),
        "regions": args.regions, "iters": args.iters,
        "build_us": {name: _quantiles(v) for name, v in build.items()},
        "step_ms": {name: _quantiles(v) for name, v in per_batch.items()},
        "structures_per_s": {name: B * len(batches) / (sum(v) * 1e-3) for name, v in per_batch.items()},
        "nodes": {"min": min(n for n, _ in sizes), "max": max(n for n, _ in sizes), "mean": sum(n for n, _ in sizes) / len(sizes)},
        "edges": {"min": min(e for _, e in sizes), "max": max(e for _, e in sizes), "mean": sum(e for _, e in sizes) / len(sizes)},
        "node_step": bs.node_step, "edge_step": bs.edge_step, "min_eager": bs.min_eager, "max_graphs": bs.max_graphs,
        "live_graphs": len(bs.live_graphs()),
        "warmup": warm,
        "timed": {"replays": bs.replays - warm["replays"], "eager_steps": bs.eager_steps - warm["eager_steps"],
                  "captures": bs.captures - warm["captures"], "evictions": bs.evictions - warm["evictions"]},
        "padded_edge_share": 1.0 - bs.real_edges / bs.padded_edges,
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
