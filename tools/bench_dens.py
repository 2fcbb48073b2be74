#!/usr/bin/env python
"""The DeNS train step three ways, one MI355X, one process, one build:

    python tools/bench_dens.py [--steps 30] [--out profiles/dens_step.json]

The shipped `equiformer_md17_dens_l2`, 8 aspirin frames per batch (168 atoms), r = 5.0, split mode.  Three loops, device-
synchronised wall time per step, 3 untimed warm-up steps each (the captured loop: as many as its graphs need), then
`--steps` timed steps per loop in alternating blocks of 5, so that a drift of the clocks reaches every loop alike:
  (A) `aten`:     the step as the reference writes it (main_md17_dens.py:379-427, :514-548): ATen corruption with boolean-mask
                  indexing, three L2MAE terms over `pred_dy[mask]`, two `isnan` tests, six `.item()` metrics, the model
                  building its own radius graph -- the code paths of the commit before the fused step existed;
  (B) `fused`:    add_masked_gaussian_noise_to_pos + DeNSLoss, eager;
  (C) `captured`: DeNSTrainStep (one HIP graph per shape bucket).
Median, p10 and p90 of the step time per loop.

    python tools/bench_dens.py --launch-path aten|fused --iters K

runs ONLY corruption + loss + loss backward (+ the metrics of (A)) K times on stand-in predictions, no model: under
`rocprofv3 --kernel-trace --stats` the difference of the kernel counts of two values of K, divided by the difference of K,
is the launches per step of that path; `--launches-aten / --launches-fused` put the two figures into the JSON line."""
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

MODEL = "equiformer_md17_dens_l2"
FRAMES, RADIUS = 8, 5.0
# md17/configs/equiformer_dens: denoising_pos_std, denoising_pos_prob, denoising_corrupt_ratio; loss weights; stand-in statistics
STD, PROB, RATIO = 0.05, 0.5, 0.25
W_E, W_F, W_D = 1.0, 80.0, 5.0
TASK_MEAN, TASK_STD = 0.1, 1.3


def aten_corrupt(data, std, prob, corrupt_ratio=None):
    """main_md17_dens.py:514-548, statement by statement."""
    batch_size = data.batch.max() + 1
    denoising_pos_mask = torch.rand(batch_size, dtype=data.pos.dtype, device=data.pos.device)
    denoising_pos_mask = (denoising_pos_mask < prob)
    denoising_pos_mask = denoising_pos_mask[data.batch]
    data.denoising_pos_mask = denoising_pos_mask
    data.noise_mask = data.denoising_pos_mask
    if corrupt_ratio is not None:
        corrupt_mask = torch.rand((data.pos.shape[0]), dtype=data.pos.dtype, device=data.pos.device)
        corrupt_mask = (corrupt_mask < corrupt_ratio)
        data.corrupt_mask = corrupt_mask
        data.noise_mask = data.noise_mask * data.corrupt_mask
    data.force = data.dy.clone()
    data.force[(~data.noise_mask)] *= 0
    noise_vec = torch.zeros_like(data.pos)
    noise_vec = noise_vec.normal_(mean=0.0, std=std)
    data.pos[data.noise_mask] = data.pos[data.noise_mask] + noise_vec[data.noise_mask]
    data.noise_vec = noise_vec
    return data


def l2mae(a, b):
    return torch.mean(torch.norm(a - b, p=2, dim=-1))


def aten_loss(pred_y, pred_dy, data):
    """main_md17_dens.py:389-403"""
    loss_e = l2mae(pred_y, ((data.y - TASK_MEAN) / TASK_STD))
    loss_f = l2mae(pred_dy[(~data.noise_mask)], (data.dy[(~data.noise_mask)] / TASK_STD))
    loss_d = l2mae(pred_dy[(data.noise_mask)], data.noise_vec[(data.noise_mask)] / STD)
    loss = W_E * loss_e
    if not loss_f.isnan():
        loss = loss + W_F * loss_f
    if not loss_d.isnan():
        loss = loss + W_D * loss_d
    return loss, loss_e, loss_f, loss_d


def aten_metrics(pred_y, pred_dy, data, loss_e, loss_f, loss_d):
    """main_md17_dens.py:411-427: six host reads"""
    out = [loss_e.item()]
    if not loss_f.isnan():
        out.append(loss_f.item())
    if not loss_d.isnan():
        out.append(loss_d.item())
    out.append(torch.mean(torch.abs(pred_y.detach() * TASK_STD + TASK_MEAN - data.y)).item())
    if not loss_f.isnan():
        err = pred_dy.detach() * TASK_STD - data.dy
        out.append(torch.mean(torch.abs(err[(~data.noise_mask)])).item())
    if not loss_d.isnan():
        err = pred_dy.detach() * STD - data.noise_vec
        out.append(torch.mean(torch.abs(err[data.noise_mask])).item())
    return out


def launch_path(path, iters, batch, dev):
    """corruption + loss + loss backward (+ metrics) alone, for a kernel trace"""
    from equiformer_amd.dens import DeNSLoss, add_masked_gaussian_noise_to_pos
    n, B = batch["pos"].shape[0], FRAMES
    g = torch.Generator().manual_seed(1)
    pred_y = torch.randn(B, 1, generator=g).to(dev).requires_grad_(True)
    pred_dy = torch.randn(n, 3, generator=g).to(dev).requires_grad_(True)
    L = DeNSLoss(TASK_MEAN, TASK_STD, STD, W_E, W_F, W_D) if path == "fused" else None
    torch.cuda.synchronize()
    for k in range(iters):
        data = SimpleNamespace(**batch)  # (no clone of pos here: the count is the step's, the noise may pile up)
        if path == "aten":
            aten_corrupt(data, STD, PROB, RATIO)
            loss, le, lf, ld = aten_loss(pred_y, pred_dy, data)
            loss.backward()
            aten_metrics(pred_y, pred_dy, data, le, lf, ld)
        else:
            add_masked_gaussian_noise_to_pos(data, STD, PROB, RATIO, seed=k)
            L(pred_y, pred_dy, data).backward()
        pred_y.grad = pred_dy.grad = None
    torch.cuda.synchronize()
    print(json.dumps({"launch_path": path, "iters": iters}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--launch-path", choices=("aten", "fused"), default=None)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--launches-aten", type=float, default=None)
    ap.add_argument("--launches-fused", type=float, default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dens.py needs an MI355X"
    from equiformer_amd import lib, nets, ops
    from equiformer_amd.dens import DeNSLoss, DeNSTrainStep, add_masked_gaussian_noise_to_pos
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW
    from equiformer_amd.synthetic import md17_aspirin_batch
    lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    d = md17_aspirin_batch(FRAMES, seed=0)
    batch = dict(pos=d["pos"].to(dev), z=d["z"].to(dev), batch=d["batch"].to(dev), y=d["y"].view(-1, 1).to(dev), dy=d["dy"].to(dev))
    if args.launch_path:
        return launch_path(args.launch_path, args.iters, batch, dev)
    assert ops.get_matrix_mode() == "split"
    model = nets.model_entrypoint(MODEL)().to(dev).train()
    opt = FlatAdamW(model.parameters(), lr=5e-4, weight_decay=1e-6)
    L = DeNSLoss(TASK_MEAN, TASK_STD, STD, W_E, W_F, W_D)
    ts = DeNSTrainStep(model, opt, L, RADIUS, STD, PROB, RATIO, seed=0)
    counter = [0]

    def step_aten():
        data = SimpleNamespace(**dict(batch, pos=batch["pos"].clone()))  # (the loader's fresh batch: the corruption is in place)
        aten_corrupt(data, STD, PROB, RATIO)
        pred_y, pred_dy = model(data)
        loss, le, lf, ld = aten_loss(pred_y, pred_dy, data)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        aten_metrics(pred_y, pred_dy, data, le, lf, ld)

    def step_fused():
        data = SimpleNamespace(**batch)
        add_masked_gaussian_noise_to_pos(data, STD, PROB, RATIO, seed=counter[0])
        counter[0] += 1
        opt.zero_grad(set_to_none=True)
        g = EdgeGraph.from_radius(data.pos, data.batch, RADIUS, num_graphs=FRAMES)
        pred_y, pred_dy = model(data, graph=g)
        L(pred_y, pred_dy, data).backward()
        opt.step()

    cbatch = dict(batch, y=d["y"].to(dev), num_graphs=FRAMES)

    def step_captured():
        ts.step(cbatch)

    legs = [("aten", step_aten), ("fused", step_fused), ("captured", step_captured)]

    def timed(step):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for name, step in legs[:2]:
        for _ in range(args.warmup):
            timed(step)
    warm_captured = 0
    while warm_captured < args.warmup or (ts.replays < 4 and warm_captured < 40):  # every bucket the noise reaches gets its graph
        timed(step_captured)
        warm_captured += 1
    warm = dict(steps=warm_captured, eager_steps=ts.eager_steps, captures=ts.captures, replays=ts.replays)
    ms = {name: [] for name, _ in legs}
    block = 5
    while len(ms["aten"]) < args.steps:
        for name, step in legs:
            for _ in range(block):
                ms[name].append(timed(step))

    def summary(v):
        s = sorted(v)
        q = lambda p: s[min(len(s) - 1, int(round(p * (len(s) - 1))))]  # noqa: E731
        return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "frames_per_s": FRAMES / (q(0.5) * 1e-3), "steps": len(s)}

    res = {name: summary(v) for name, v in ms.items()}
    out = {
        "what": "DeNS train step, %s, %d aspirin frames per batch (%d atoms), r=%.1f, split mode, one process; device-synchronised "
                "wall time per step, loops alternating in blocks of %d steps" % (MODEL, FRAMES, batch["pos"].shape[0], RADIUS, block),
        "build": lib.built_hash(),
        "corruption": {"std": STD, "prob": PROB, "corrupt_ratio": RATIO},
        "warmup_steps": {"aten": args.warmup, "fused": args.warmup, "captured": warm},
        "aten": res["aten"], "fused": res["fused"], "captured": res["captured"],
        "captured_timed": {"eager_steps": ts.eager_steps - warm["eager_steps"], "captures": ts.captures - warm["captures"],
                           "replays": ts.replays - warm["replays"], "live_graphs": len(ts.bucketed.live_graphs())},
        "fused_over_aten": res["aten"]["median_ms"] / res["fused"]["median_ms"],
        "captured_over_aten": res["aten"]["median_ms"] / res["captured"]["median_ms"],
        "launches_corruption_plus_loss": {"aten": args.launches_aten, "fused": args.launches_fused,
                                          "how": "rocprofv3 --kernel-trace --stats on --launch-path runs of their own: kernel "
                                                 "count difference of two iteration counts over the difference of iterations"},
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
