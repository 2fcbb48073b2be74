#!/usr/bin/env python
"""Eager train step of the OC20 E(3) model on the fused against the un-fused tensor-product kernels, one MI355X:

    python tools/bench_e3_oc20.py [--steps 20] [--regions 5] [--out profiles/e3_oc20.json]

oc20_l1_256_e3_nonlinear as registered (6 blocks), the slab batch of bench.py's OC20 sub-record (16 structures x 78 atoms,
r = 5, max_neighbors = 500), split matrix mode.  From ONE process and ONE build: milliseconds per step (forward, backward,
FlatAdamW) with `set_fused(True)` -- the fused SeparableFCTP kernels, planned by (degree, parity) segment -- and with
`set_fused(False)` -- depth-wise tensor product written to memory, per-irrep linears, what E(3) models ran on before --, as
`--regions` timed regions of `--steps` steps each (synchronised wall clock), the two legs alternating.  `spread` is the
run-to-run spread of a leg, (max - min) / min over its regions; `unfused_over_fused` compares the slowest fused region with
the fastest un-fused one.  Prints one JSON line."""
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

MODEL = "oc20_l1_256_e3_nonlinear"
RADIUS, MAX_NEIGHBORS = 5.0, 500


def _median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--structures", type=int, default=16)
    ap.add_argument("--atoms", type=int, default=78)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_e3_oc20.py needs an MI355X"
    from equiformer_amd import lib, nets, ops
    from equiformer_amd.optim import FlatAdamW, add_weight_decay
    from equiformer_amd.synthetic import oc20_like_varying_batches
    lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = nets.model_entrypoint(MODEL)().to(dev).train()
    ga = model.blocks[0].ga
    assert ga.act_sfc_spec.supported and ga.sep_value.sfc_spec.supported and model.edge_deg_embed.sfc_spec.supported
    opt = FlatAdamW(add_weight_decay(model, 1e-3, model.no_weight_decay()), lr=2e-4)
    d = oc20_like_varying_batches(1, args.structures, (args.atoms, args.atoms), seed=1000)[0]
    d = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}
    data = SimpleNamespace(pos=d["pos"], batch=d["batch"], atomic_numbers=d["atomic_numbers"], tags=d["tags"], cell=d["cell"],
                           natoms=d["natoms"])

    def step():
        opt.zero_grad(set_to_none=True)
        loss = (model(data).squeeze(-1) - d["y"]).abs().mean()
        loss.backward()
        opt.step()
        return loss.detach()

    def region(fused):
        model.set_fused(fused)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.steps

    for fused in (True, False, True, False):  # warm-up: clocks, allocator pools, lazily built tables
        region(fused)
    ms = {True: [], False: []}
    for _ in range(args.regions):
        for fused in (True, False):  # alternating: a drift of the box's clocks reaches both legs alike
            ms[fused].append(region(fused))
    spread = {k: (max(v) - min(v)) / min(v) for k, v in ms.items()}
    out = {
        "what": "eager train step of %s, %d x %d-atom slabs, r=%.1f, max_neighbors=%d, matrix mode %s; ms per step, one timed "
                "region = %d steps, synchronised wall clock" % (MODEL, args.structures, args.atoms, RADIUS, MAX_NEIGHBORS,
                                                                ops.get_matrix_mode(), args.steps),
        "build": lib.built_hash(),
        "unit": "ms/step",
        "regions": args.regions,
        "fused": {"value": _median(ms[True]), "values": ms[True], "spread": spread[True]},
        "unfused": {"value": _median(ms[False]), "values": ms[False], "spread": spread[False]},
        "spread": max(spread.values()),
        "unfused_over_fused_median": _median(ms[False]) / _median(ms[True]),
        "unfused_over_fused": min(ms[False]) / max(ms[True]),
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
