#!/usr/bin/env python
"""Train-step rate over batches whose node / edge counts change every step (what a real loader yields), one MI355X:

    python tools/bench_varying.py [--batches 48] [--regions 3] [--out profiles/varying_batches.json]

The full QM9 model of bench.py (graph_attention_transformer_nonlinear_l2, 128 molecules per batch), molecules of 12-24 atoms so
that N and E scatter around the bench shape (2 304 nodes, ~25 354 edges).  From ONE process and ONE build, real molecules/s of
  (a) `bucketed`: equiformer_amd.capture.BucketedTrainStep (batch padded to its bucket, one HIP graph per bucket),
  (b) `eager`:    the plain eager step on the same, unpadded batches,
  (c) `captured_fixed`: CapturedTrainStep on ONE fixed batch of the bench shape (orientation: the padding-free ceiling),
each as `--regions` timed regions of one pass over all batches (synchronised wall clock), the legs alternating.  Before the
timed regions every leg runs untimed passes until its graphs exist (bucketed: min_eager + 1 passes).  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODEL = "graph_attention_transformer_nonlinear_l2"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--molecules", type=int, default=128)
    ap.add_argument("--atoms-min", type=int, default=12)
    ap.add_argument("--atoms-max", type=int, default=24)
    ap.add_argument("--side", type=float, default=6.5)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--max-graphs", type=int, default=None)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_varying.py needs an MI355X"
    from equiformer_amd import capture, lib, nets
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW, add_weight_decay
    from equiformer_amd.synthetic import qm9_like_batch, qm9_like_varying_batches
    lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B = args.molecules
    model = nets.model_entrypoint(MODEL)(irreps_in="5x0e", radius=5.0, num_basis=128).to(dev).train()
    opt = FlatAdamW(add_weight_decay(model, 5e-3, model.no_weight_decay()), lr=5e-4)
    to_dev = lambda d: {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}  # noqa: E731
    batches = [to_dev(d) for d in qm9_like_varying_batches(args.batches, B, (args.atoms_min, args.atoms_max), side=args.side,
                                                           seed=1000)]
    fixed = to_dev(qm9_like_batch(B, 18, side=args.side, seed=1000))

    # (b) eager, unpadded
    def eager_step(d):
        opt.zero_grad(set_to_none=True)
        g = EdgeGraph.from_radius(d["pos"], d["batch"], 5.0, num_graphs=B)
        loss = (model(None, d["pos"], d["batch"], d["z"], graph=g).squeeze(-1) - d["y"]).abs().mean()
        loss.backward()
        opt.step()
        return loss.detach()

    # (a) bucketed
    def padded_loss(g, v):
        return (model(None, v.pos, v.batch, v.z, graph=g).squeeze(-1)[:v.B] - v.y[:v.B]).abs().mean()
    kw = {} if args.max_graphs is None else dict(max_graphs=args.max_graphs)
    bs = capture.BucketedTrainStep(opt, padded_loss, 5.0, **kw)

    # (c) the fixed batch, exact-shape capture
    def fixed_loss(g):
        return (model(None, fixed["pos"], fixed["batch"], fixed["z"], graph=g).squeeze(-1) - fixed["y"]).abs().mean()
    cs = capture.CapturedTrainStep(opt, fixed_loss)

    def fixed_step(_):
        return cs.step(lambda into: EdgeGraph.from_radius(fixed["pos"], fixed["batch"], 5.0, num_graphs=B, into=into))

    legs = [("eager", eager_step), ("bucketed", bs.step), ("captured_fixed", fixed_step)]

    def one_pass(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for d in batches:
            step(d)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    # warm-up: clocks, allocator pools, lazily built tables; then every bucket's graph (min_eager eager steps + the capture)
    one_pass(eager_step)
    torch.cuda.synchronize()
    mem0 = (torch.cuda.memory_allocated(), torch.cuda.memory_reserved())
    t_cap0 = time.perf_counter()
    for _ in range(bs.min_eager + 1):
        one_pass(bs.step)
    t_cap = time.perf_counter() - t_cap0
    torch.cuda.synchronize()
    mem1 = (torch.cuda.memory_allocated(), torch.cuda.memory_reserved())
    n_live = max(1, len(bs.live_graphs()))
    for _ in range(cs.min_eager + 2):
        fixed_step(None)
    warm = dict(replays=bs.replays, eager_steps=bs.eager_steps, captures=bs.captures, evictions=bs.evictions)

    times = {name: [] for name, _ in legs}
    for _ in range(args.regions):
        for name, step in legs:  # alternating: a drift of the box's clocks reaches every leg alike
            times[name].append(one_pass(step))
    mols = B * len(batches)
    rate = {name: [mols / t for t in ts] for name, ts in times.items()}
    sizes = [(int(d["pos"].shape[0]), EdgeGraph.from_radius(d["pos"], d["batch"], 5.0, num_graphs=B).E) for d in batches]
    keys = [capture.bucket_of(B, n, e, bs.node_step, bs.edge_step) for n, e in sizes]
    out = {
        "what": "QM9 %s train step over %d different batches of %d molecules (%d-%d atoms), r=5.0, split mode; molecules/s of real "
                "molecules, one timed region = one pass over all batches, synchronised wall clock" % (
                    MODEL, len(batches), B, args.atoms_min, args.atoms_max),
        "build": lib.built_hash(),
        "unit": "molecules/s",
        "regions": args.regions,
        "bucketed": {"value": sorted(rate["bucketed"])[len(rate["bucketed"]) // 2], "values": rate["bucketed"]},
        "eager": {"value": sorted(rate["eager"])[len(rate["eager"]) // 2], "values": rate["eager"]},
        "captured_fixed": {"value": sorted(rate["captured_fixed"])[len(rate["captured_fixed"]) // 2], "values": rate["captured_fixed"],
                           "nodes": int(fixed["pos"].shape[0]), "replays": cs.replays},
        "eager_spread": (max(rate["eager"]) - min(rate["eager"])) / min(rate["eager"]),
        "bucketed_over_eager": min(rate["bucketed"]) / max(rate["eager"]),
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
