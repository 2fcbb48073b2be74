#!/usr/bin/env python
"""Evaluation-loop time over batches whose node and edge counts change every step, one MI355X:

    python tools/bench_eval.py [--batches 48] [--repeats 7] [--workloads qm9,oc20,md17] [--out profiles/eval_step.json]

Three workloads at the sizes of bench.py, full models in eval mode, split matrix mode:
  qm9   graph_attention_transformer_nonlinear_l2, 128 molecules of 12-24 atoms per batch (tools/bench_varying.py's batches)
  oc20  oc20_l1_256_nonlinear, 16 slab structures of 60-96 atoms per batch (tools/bench_varying_oc20.py's batches)
  md17  graph_attention_transformer_nonlinear_exp_l2_md17, 8 aspirin frames per batch, a fresh jitter per batch; forces by the
        first-order pass of eval mode
For each, from ONE process and ONE build, two loops over the same batches:
  (a) `eager`:    the evaluation loop as it is written without equiformer_amd.evaluate -- the model call under no_grad (MD17: the
                  model enables grad for its force pass itself), the reference's torch metric expressions and its `.item()` calls
                  (engine.py:136-139: 2 per batch, main_md17.py:451-462: 4, the IS2RE evaluator: 3) into host-side running sums;
  (b) `bucketed`: equiformer_amd.evaluate.evaluate_* on a BucketedEvalStep that is kept between passes (one HIP graph per
                  bucket; one read-back at the end of a pass plus the graph build's own per batch).
One timed region = one pass over all batches, synchronised wall clock; the legs alternate.  Before the timed regions the eager
leg runs one untimed pass and the bucketed leg min_eager + 1 (until its graphs exist).  Reports, per workload and leg, the median
and the 10th / 90th percentile of the milliseconds per batch over the repeats, the counters, and that both legs agree on the
MAE.  Prints one JSON line."""
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

RADIUS = 5.0
OC20_MAX_NEIGHBORS = 500
MEAN, STD = 0.25, 1.5  # a normaliser that is not the identity


def _pct(values, q):
    v = sorted(values)
    x = q * (len(v) - 1)
    lo = int(x)
    hi = min(lo + 1, len(v) - 1)
    return v[lo] + (v[hi] - v[lo]) * (x - lo)


def _stats(ms):
    return {"median": _pct(ms, 0.5), "p10": _pct(ms, 0.1), "p90": _pct(ms, 0.9), "values": ms}


class _Avg:
    def __init__(self):
        self.sum, self.count = 0.0, 0

    def update(self, val, n):
        self.sum += val * n
        self.count += n

    @property
    def avg(self):
        return self.sum / self.count


def qm9(dev, n_batches):
    from equiformer_amd import evaluate, nets
    from equiformer_amd.synthetic import qm9_like_varying_batches
    model = nets.model_entrypoint("graph_attention_transformer_nonlinear_l2")(irreps_in="5x0e", radius=RADIUS, num_basis=128)
    model = model.to(dev).eval()
    batches = qm9_like_varying_batches(n_batches, 128, (12, 24), side=6.5, seed=1000)
    step = evaluate.qm9_eval_step(model, (MEAN, STD), RADIUS, max_graphs=32)

    def eager(batches):
        loss_m, mae_m = _Avg(), _Avg()
        criterion = torch.nn.L1Loss()
        with torch.no_grad():
            for d in batches:
                pred = model(None, d["pos"], d["batch"], d["z"]).squeeze()
                loss = criterion(pred, (d["y"] - MEAN) / STD)
                loss_m.update(loss.item(), n=pred.shape[0])
                err = pred.detach() * STD + MEAN - d["y"]
                mae_m.update(torch.mean(torch.abs(err)).item(), n=pred.shape[0])
        return mae_m.avg

    def bucketed(batches):
        return evaluate.evaluate_qm9(model, (MEAN, STD), 0, batches, RADIUS, step=step)[0]
    text = "QM9 graph_attention_transformer_nonlinear_l2, eval mode, 128 molecules of 12-24 atoms per batch, r=5.0, num_basis=128"
    return batches, eager, bucketed, step, 128, text


def oc20(dev, n_batches):
    from equiformer_amd import evaluate, nets
    from equiformer_amd.synthetic import oc20_like_varying_batches
    model = nets.model_entrypoint("oc20_l1_256_nonlinear")().to(dev).eval()
    batches = oc20_like_varying_batches(n_batches, 16, (60, 96), seed=1000)
    step = evaluate.oc20_eval_step(model, RADIUS, task_mean=MEAN, task_std=STD, max_num_neighbors=OC20_MAX_NEIGHBORS,
                                   edge_step=2048, max_graphs=32)

    def eager(batches):
        tot = {"energy_mae": 0.0, "energy_mse": 0.0, "energy_within_threshold": 0.0}
        numel = 0
        with torch.no_grad():
            for d in batches:
                data = SimpleNamespace(pos=d["pos"], batch=d["batch"], atomic_numbers=d["atomic_numbers"], tags=d["tags"],
                                       cell=d["cell"], natoms=d["natoms"])
                pred = model(data).view(-1) * STD + MEAN  # the normalizer's denorm
                err = torch.abs(d["y"] - pred)
                tot["energy_mae"] += torch.sum(err).item()
                tot["energy_mse"] += torch.sum((d["y"] - pred) ** 2).item()
                tot["energy_within_threshold"] += (err < 0.02).sum().item()
                numel += pred.numel()
        return tot["energy_mae"] / numel

    def bucketed(batches):
        return evaluate.evaluate_oc20(model, batches, RADIUS, step=step)["energy_mae"]["metric"]
    text = ("OC20 oc20_l1_256_nonlinear, eval mode, 16 slab structures of 60-96 atoms per batch (11 x 11 x 30 A cell), r=5.0, "
            "max_neighbors=%d" % OC20_MAX_NEIGHBORS)
    return batches, eager, bucketed, step, 16, text


def md17(dev, n_batches):
    from equiformer_amd import evaluate, nets
    from equiformer_amd.synthetic import md17_aspirin_batch
    model = nets.model_entrypoint("graph_attention_transformer_nonlinear_exp_l2_md17")(
        irreps_in="64x0e", radius=RADIUS, num_basis=32, task_mean=MEAN, task_std=STD).to(dev).eval()
    batches = []
    for i in range(n_batches):
        d = md17_aspirin_batch(8, jitter=0.05, seed=1000 + i)
        batches.append(dict(d, y=d["y"].view(-1, 1), num_graphs=8))
    step = evaluate.md17_eval_step(model, RADIUS, edge_step=256)

    def l2mae(a, b):
        return torch.mean(torch.norm(a - b, p=2, dim=-1))

    def eager(batches):
        lm = {"energy": _Avg(), "force": _Avg()}
        mm = {"energy": _Avg(), "force": _Avg()}
        with torch.no_grad():
            for d in batches:
                pred_y, pred_dy = model(node_atom=d["z"], pos=d["pos"], batch=d["batch"])
                loss_e = l2mae(pred_y, (d["y"] - MEAN) / STD)
                loss_f = l2mae(pred_dy, d["dy"] / STD)
                lm["energy"].update(loss_e.item(), n=pred_y.shape[0])
                lm["force"].update(loss_f.item(), n=pred_dy.shape[0])
                energy_err = torch.mean(torch.abs(pred_y.detach() * STD + MEAN - d["y"])).item()
                mm["energy"].update(energy_err, n=pred_y.shape[0])
                force_err = torch.mean(torch.abs(pred_dy.detach() * STD - d["dy"])).item()
                mm["force"].update(force_err, n=pred_dy.shape[0])
        return mm["force"].avg

    def bucketed(batches):
        return evaluate.evaluate_md17(model, batches, RADIUS, step=step)[0]["force"].avg
    text = ("MD17 aspirin graph_attention_transformer_nonlinear_exp_l2_md17, eval mode (first-order force pass), 8 frames of 21 "
            "atoms per batch, jitter 0.05 A, r=5.0, num_basis=32")
    return batches, eager, bucketed, step, 8, text


WORKLOADS = {"qm9": qm9, "oc20": oc20, "md17": md17}


def run(name, dev, n_batches, repeats):
    batches, eager, bucketed, step, units, text = WORKLOADS[name](dev, n_batches)
    batches = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()} for d in batches]

    def one_pass(loop):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mae = loop(batches)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(batches), mae

    one_pass(eager)
    t0 = time.perf_counter()
    for _ in range(step.min_eager + 1):
        one_pass(bucketed)
    t_cap = time.perf_counter() - t0
    warm = dict(replays=step.replays, eager_steps=step.eager_steps, captures=step.captures, evictions=step.evictions, seconds=t_cap)
    ms = {"eager": [], "bucketed": []}
    mae = {}
    for _ in range(repeats):
        for leg, loop in (("eager", eager), ("bucketed", bucketed)):  # alternating: a drift of the clocks reaches both legs
            t, mae[leg] = one_pass(loop)
            ms[leg].append(t)
    e, b = _stats(ms["eager"]), _stats(ms["bucketed"])
    return {
        "what": text, "unit": "ms per batch", "batches": len(batches), "units_per_batch": units, "repeats": repeats,
        "eager": e, "bucketed": b,
        "speedup_median": e["median"] / b["median"],
        # beyond the spread: the slow end of the bucketed loop against the fast end of the eager one
        "speedup_p90_over_p10": e["p10"] / b["p90"],
        "mae": mae, "mae_rel_diff": abs(mae["eager"] - mae["bucketed"]) / abs(mae["eager"]),
        "node_step": step.node_step, "edge_step": step.edge_step, "min_eager": step.min_eager, "max_graphs": step.max_graphs,
        "live_graphs": len(step.live_graphs()), "warmup": warm,
        "timed": {"replays": step.replays - warm["replays"], "eager_steps": step.eager_steps - warm["eager_steps"],
                  "captures": step.captures - warm["captures"], "evictions": step.evictions - warm["evictions"]},
        "padded_edge_share": 1.0 - step.real_edges / step.padded_edges,
        "padded_node_share": 1.0 - step.real_nodes / step.padded_nodes,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--workloads", default="qm9,oc20,md17")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_eval.py needs an MI355X"
    from equiformer_amd import lib
    lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    out = {"build": lib.built_hash()}
    for name in args.workloads.split(","):
        out[name] = run(name, dev, args.batches, args.repeats)
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
