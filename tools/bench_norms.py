#!/usr/bin/env python
"""Step time of the eager QM9 bench-batch train step (128 molecules x 18 atoms, graph_attention_transformer_nonlinear_l2,
matrix mode "split", radius graph + forward + L1 + backward + AdamW) once per norm_layer in ONE process: 'layer' is the
yardstick (its path does not know the other norms exist), 'fast_layer' runs the same kernels, 'graph' and 'instance' run
csrc/graphnorm.hip.  Not a bench.py line: for DESIGN.md's record.

    python tools/bench_norms.py [--steps 30] [--warmup 3] [--out profiles/norm_types.json]

Per-kernel times are not taken here (every step is timed between two device synchronisations); take them with a kernel
trace of this script run for one norm type:  --only graph --steps 20.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from equiformer_amd import ops  # noqa: E402
from equiformer_amd.graph import EdgeGraph  # noqa: E402
from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer, _l2_kwargs  # noqa: E402
from equiformer_amd.optim import FlatAdamW, add_weight_decay  # noqa: E402
from equiformer_amd.synthetic import qm9_like_batch  # noqa: E402

NORM_TYPES = ("layer", "fast_layer", "graph", "instance")


def run(norm_type, args, dev):
    torch.manual_seed(0)
    model = GraphAttentionTransformer(**_l2_kwargs("5x0e", 5.0, 128, None, None, None, norm_layer=norm_type)).to(dev).train()
    opt = FlatAdamW(add_weight_decay(model, 5e-3, model.no_weight_decay()), lr=5e-4)
    d = {k: v.to(dev) for k, v in qm9_like_batch(args.batch, args.atoms, side=args.side, seed=1000).items()}

    def step():
        opt.zero_grad(set_to_none=True)
        g = EdgeGraph.from_radius(d["pos"], d["batch"], 5.0, num_graphs=args.batch)
        pred = model(f_in=None, pos=d["pos"], batch=d["batch"], node_atom=d["z"], graph=g)
        loss = (pred.squeeze() - d["y"]).abs().mean()
        loss.backward()
        opt.step()
        return loss

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        loss = step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    q = lambda f: times[min(len(times) - 1, int(f * len(times)))]  # noqa: E731
    return dict(norm_layer=norm_type, median_ms=statistics.median(times), min_ms=times[0], p10_ms=q(0.1), p90_ms=q(0.9),
                max_ms=times[-1], steps=args.steps, warmup=args.warmup, final_loss=float(loss))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--atoms", type=int, default=18)
    ap.add_argument("--side", type=float, default=6.5)
    ap.add_argument("--only", default="", help="one norm type (for a kernel trace)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.steps >= 20 or args.only, "at least 20 timed steps"
    dev = torch.device("cuda:0")
    prev = ops.set_matrix_mode("split")
    recs = [run(nt, args, dev) for nt in (NORM_TYPES if not args.only else (args.only,))]
    ops.set_matrix_mode(prev)
    base = recs[0]["median_ms"]
    for r in recs:
        r["vs_layer"] = r["median_ms"] / base
        print("norm_layer=%-10s median %.2f ms  (min %.2f, p10 %.2f, p90 %.2f, max %.2f)  x%.3f of 'layer'"
              % (r["norm_layer"], r["median_ms"], r["min_ms"], r["p10_ms"], r["p90_ms"], r["max_ms"], r["vs_layer"]), flush=True)
    out = dict(workload="QM9 eager train step, %d molecules x %d atoms, side %.1f, r=5.0, num_basis=128, alpha_drop=0.2, "
                        "matrix mode split; radius graph rebuilt every step" % (args.batch, args.atoms, args.side),
               device=torch.cuda.get_device_name(0), timing="wall clock between device synchronisations, per step",
               records=recs)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
