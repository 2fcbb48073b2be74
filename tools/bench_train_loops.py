#!/usr/bin/env python
"""Training-loop time over batches whose node and edge counts change every step, one MI355X:

    python tools/bench_train_loops.py [--batches 48] [--repeats 7] [--workloads qm9,md17,oc20] [--out profiles/train_loops.json]

Three workloads at the sizes of bench.py (the batches of tools/bench_eval.py), full models in training mode, split matrix mode:
  qm9   graph_attention_transformer_nonlinear_l2, 128 molecules of 12-24 atoms per batch, L1 on the normalised target
  md17  graph_attention_transformer_nonlinear_exp_l2_md17, 8 aspirin frames per batch (fresh jitter), L2MAE, energy weight 1,
        force weight 80 (forces by the create_graph pass, second-order backward)
  oc20  oc20_l1_256_nonlinear (energy head), 16 slab structures of 60-96 atoms per batch, L1 on the normalised energy
For each, from ONE process and ONE build, two loops over the same batches, each with its own model and FlatAdamW from the
same initial weights:
  (a) `aten`: a BucketedTrainStep whose forward_loss is the loss of INTEGRATION.md written in ATen (the per-node term weighted by
      view.node_mask), which also copies the reference's metric expressions into a fixed device buffer; after every step the
      reference's `.item()` read-backs of them into host-side AverageMeters (engine.py:85-87: 2; main_md17.py:392-400: 4; the
      OC20 trainer's loss + evaluator metrics, energy_trainer_v2.py:275-283: 4);
  (b) `loop`: equiformer_amd.train.train_one_epoch_* on the step of qm9_train_step / md17_train_step / oc20_train_step (the fused
      loss with the meters folded in; one read-back at the end of the pass).
One timed region = one pass over all batches, synchronised wall clock; the legs alternate.  Before the timed regions each leg
runs min_eager + 1 untimed passes (until its graphs exist).  Reports per workload and leg the median and the 10th / 90th
percentile of the milliseconds per batch over the repeats, and the counters.  Then the loss operator ALONE at the workload's
shape (stand-in predictions, forward + backward): device kernels per call from the torch profiler, and microseconds per call
of 200 calls back to back through Python and of the same 200 calls replayed from one captured HIP graph, both timed by device
events, the two losses alternating, 7 blocks after an untimed one.  Prints one JSON line."""
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
W_E, W_F = 1.0, 80.0
LR = 1e-4


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


def _seeded(make):
    torch.manual_seed(0)
    return make()


# ------------------------------------------------------------------------------------------------------------------ workloads
def qm9(dev, n_batches):
    from equiformer_amd import nets
    from equiformer_amd.synthetic import qm9_like_varying_batches

    def make():
        m = nets.model_entrypoint("graph_attention_transformer_nonlinear_l2")(irreps_in="5x0e", radius=RADIUS, num_basis=128)
        return m.to(dev).train()
    batches = qm9_like_varying_batches(n_batches, 128, (12, 24), side=6.5, seed=1000)

    def predict(m, g, v):
        return m(None, v.pos, v.batch, v.z, graph=g), None

    def aten_loss(pred, F, v, buf):
        p = pred.squeeze(-1)[:v.B]
        loss = (p - (v.y[:v.B] - MEAN) / STD).abs().mean()  # L1Loss, engine.py:71
        buf[0:2].copy_(torch.stack([loss.detach(), (p.detach() * STD + MEAN - v.y[:v.B]).abs().mean()]))
        return loss

    def read(buf, B, N, meters):  # engine.py:85-87
        meters[0].update(buf[0].item(), B)
        meters[1].update(buf[1].item(), B)
    return dict(make=make, batches=batches, predict=predict, aten_loss=aten_loss, read=read, units=128, node_targets=(),
                bucket=dict(max_graphs=32), text="QM9 graph_attention_transformer_nonlinear_l2, 128 molecules of 12-24 atoms "
                "per batch, r=5.0, num_basis=128, L1")


def md17(dev, n_batches):
    from equiformer_amd import nets
    from equiformer_amd.synthetic import md17_aspirin_batch

    def make():
        m = nets.model_entrypoint("graph_attention_transformer_nonlinear_exp_l2_md17")(
            irreps_in="64x0e", radius=RADIUS, num_basis=32, task_mean=MEAN, task_std=STD)
        return m.to(dev).train()
    batches = []
    for i in range(n_batches):
        d = md17_aspirin_batch(8, jitter=0.05, seed=1000 + i)
        batches.append(dict(d, y=d["y"].view(-1, 1), num_graphs=8))

    def predict(m, g, v):
        return m(node_atom=v.z, pos=v.pos, batch=v.batch, graph=g)

    def aten_loss(E, F, v, buf):
        w = v.node_mask
        loss_e = (E[:v.B] - (v.y[:v.B] - MEAN) / STD).abs().mean()
        loss_f = ((F - v.dy / STD).norm(dim=1) * w).sum() / w.sum()
        Fd = F.detach()
        mae_f = ((Fd * STD - v.dy).abs() * w[:, None]).sum() / (3.0 * w.sum())
        buf[0:4].copy_(torch.stack([loss_e.detach(), loss_f.detach(), (E.detach()[:v.B] * STD + MEAN - v.y[:v.B]).abs().mean(),
                                    mae_f]))
        return W_E * loss_e + W_F * loss_f

    def read(buf, B, N, meters):  # main_md17.py:392-400
        for q, n in ((0, B), (1, N), (2, B), (3, N)):
            meters[q].update(buf[q].item(), n)
    return dict(make=make, batches=batches, predict=predict, aten_loss=aten_loss, read=read, units=8, node_targets=("dy",),
                bucket=dict(edge_step=256), text="MD17 aspirin graph_attention_transformer_nonlinear_exp_l2_md17, 8 frames of 21 "
                "atoms per batch, jitter 0.05 A, r=5.0, num_basis=32, L2MAE, energy weight 1, force weight 80")


def oc20(dev, n_batches):
    from equiformer_amd import nets
    from equiformer_amd.synthetic import oc20_like_varying_batches

    def make():
        return nets.model_entrypoint("oc20_l1_256_nonlinear")().to(dev).train()
    batches = oc20_like_varying_batches(n_batches, 16, (60, 96), seed=1000)

    def predict(m, g, v):
        out = m(v, graph=g, offsets=v.offsets)
        return (out[0] if isinstance(out, tuple) else out), None

    def aten_loss(E, F, v, buf):
        p = E.reshape(-1)[:v.B]
        loss = (p - (v.y[:v.B] - MEAN) / STD).abs().mean()
        err = (p.detach() * STD + MEAN - v.y[:v.B])
        buf[0:4].copy_(torch.stack([loss.detach(), err.abs().mean(), (err * err).mean(), (err.abs() < 0.02).float().mean()]))
        return loss

    def read(buf, B, N, meters):  # loss.item() and the evaluator's three metrics
        for q in range(4):
            meters[q].update(buf[q].item(), B)
    return dict(make=make, batches=batches, predict=predict, aten_loss=aten_loss, read=read, units=16, node_targets=("tags",),
                bucket=dict(max_num_neighbors=OC20_MAX_NEIGHBORS, edge_step=2048, max_graphs=32),
                text="OC20 oc20_l1_256_nonlinear, 16 slab structures of 60-96 atoms per batch (11 x 11 x 30 A cell), r=5.0, "
                "max_neighbors=%d, L1" % OC20_MAX_NEIGHBORS)


WORKLOADS = {"qm9": qm9, "md17": md17, "oc20": oc20}


# ------------------------------------------------------------------------------------------------------------------ the two loops
def _legs(name, w, dev):
    from equiformer_amd import train
    from equiformer_amd.capture import BucketedTrainStep
    from equiformer_amd.optim import FlatAdamW
    m_a = _seeded(w["make"])
    opt_a = FlatAdamW(m_a.parameters(), lr=LR, weight_decay=1e-2)
    buf = torch.zeros(4, dtype=torch.float32, device=dev)

    def forward_loss(g, v):
        E, F = w["predict"](m_a, g, v)
        return w["aten_loss"](E, F, v, buf)
    aten_step = BucketedTrainStep(opt_a, forward_loss, RADIUS, graph_targets=("y",), node_targets=w["node_targets"],
                                  **w["bucket"])

    def aten(batches):
        m_a.train()
        meters = [_Avg() for _ in range(4)]
        for d in batches:
            aten_step.step(d)
            w["read"](buf, int(d["num_graphs"]), d["pos"].shape[0], meters)
        return meters[1].sum / meters[1].count

    m_b = _seeded(w["make"])
    opt_b = FlatAdamW(m_b.parameters(), lr=LR, weight_decay=1e-2)
    if name == "qm9":
        step = train.qm9_train_step(m_b, opt_b, (MEAN, STD), RADIUS, criterion="l1", **w["bucket"])

        def loop(batches):
            return train.train_one_epoch_qm9(step, batches)
    elif name == "md17":
        step = train.md17_train_step(m_b, opt_b, RADIUS, W_E, W_F, criterion="l2mae", **w["bucket"])

        def loop(batches):
            return train.train_one_epoch_md17(step, batches)[1]["force"].avg
    else:
        step = train.oc20_train_step(m_b, opt_b, RADIUS, task_mean=MEAN, task_std=STD, criterion="l1", **w["bucket"])

        def loop(batches):
            return train.train_one_epoch_oc20(step, batches)[0]["energy_mae"]["metric"]
    return dict(aten=(aten, aten_step), loop=(loop, step.bucketed))


def _counters(s):
    return dict(replays=s.replays, eager_steps=s.eager_steps, captures=s.captures, evictions=s.evictions)


def run(name, dev, n_batches, repeats):
    w = WORKLOADS[name](dev, n_batches)
    batches = [{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()} for d in w["batches"]]
    legs = _legs(name, w, dev)

    def one_pass(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(batches)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / len(batches)

    warm = {}
    for leg, (fn, s) in legs.items():
        t0 = time.perf_counter()
        for _ in range(s.min_eager + 1):
            one_pass(fn)
        warm[leg] = dict(_counters(s), seconds=time.perf_counter() - t0)
    ms = {leg: [] for leg in legs}
    for _ in range(repeats):
        for leg, (fn, _) in legs.items():  # alternating: a drift of the clocks reaches both legs
            ms[leg].append(one_pass(fn))
    res = {"what": w["text"], "unit": "ms per batch", "batches": len(batches), "units_per_batch": w["units"], "repeats": repeats,
           "lr": LR}
    for leg, (_, s) in legs.items():
        c = _counters(s)
        res[leg] = dict(_stats(ms[leg]), warmup=warm[leg], timed={k: c[k] - warm[leg][k] for k in c},
                        live_graphs=len(s.live_graphs()))
    a, b = res["aten"], res["loop"]
    res["ratio_median"] = a["median"] / b["median"]
    res["aten_p10_over_loop_p90"] = a["p10"] / b["p90"]  # > 1: the loop's slow end is faster than the ATen loop's fast end
    res["loss_alone"] = loss_alone(name, w, dev, batches[0])
    return res


# ------------------------------------------------------------------------------------------------------------ the loss alone
def loss_alone(name, w, dev, d, calls=200, blocks=7):
    """forward + backward of the two losses on stand-in predictions of the workload's shape (B + 1 energy rows, N_cap force rows
    with a phantom tail): device kernels per call and microseconds per call"""
    from equiformer_amd import train
    g = torch.Generator().manual_seed(1)
    B = int(d["num_graphs"])
    N = d["pos"].shape[0]
    n_cap = N + 16
    forces = name == "md17"
    y = torch.cat([d["y"].reshape(-1), torch.zeros(1, device=dev)])
    v = SimpleNamespace(B=B, y=y.reshape(-1, 1) if forces else y,
                        node_mask=(torch.arange(n_cap, device=dev) < N).float())
    v.dy = torch.cat([d["dy"], torch.zeros(16, 3, device=dev)]) if forces else None
    E = torch.randn(B + 1, 1, generator=g).to(dev).requires_grad_(True)
    F = torch.randn(n_cap, 3, generator=g).to(dev).requires_grad_(True) if forces else None
    crit = {"qm9": "l1", "md17": "l2mae", "oc20": "l1"}[name]
    L = train.EFLoss(MEAN, STD, crit, W_E, W_F if forces else 0.0)
    buf = torch.zeros(4, device=dev)
    if name == "oc20":
        def aten_f():
            return w["aten_loss"](E, None, v, buf)
    elif forces:
        def aten_f():
            return w["aten_loss"](E, F, v, buf)
    else:
        def aten_f():
            return w["aten_loss"](E, None, v, buf)

    def fused_f():
        return L(E, v.y, B, F, v.dy, v.node_mask) if forces else L(E, v.y, B)
    ins = [E] + ([F] if forces else [])

    def one(f):
        for t in ins:
            t.grad = None
        f().backward()
    out = {}
    for leg, f in (("aten", aten_f), ("fused", fused_f)):
        one(f)
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            one(f)
            torch.cuda.synchronize()
        kinds = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        out[leg] = {"device_activities": len(kinds), "names": sorted({e.name for e in kinds})}
    # captured: `calls` calls in one graph per loss (grads kept: set_to_none inside a capture is not needed, they accumulate)
    graphs = {}
    for leg, f in (("aten", aten_f), ("fused", fused_f)):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(3):
                f().backward()
        torch.cuda.current_stream().wait_stream(s)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(calls):
                f().backward()
        graphs[leg] = gr
    us = {(leg, mode): [] for leg in ("aten", "fused") for mode in ("python", "graph")}
    for blk in range(blocks + 1):
        for leg, f in (("aten", aten_f), ("fused", fused_f)):
            for mode in ("python", "graph"):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0.record()
                if mode == "graph":
                    graphs[leg].replay()
                else:
                    for _ in range(calls):
                        f().backward()
                t1.record()
                torch.cuda.synchronize()
                if blk:
                    us[(leg, mode)].append(t0.elapsed_time(t1) * 1e3 / calls)
    for (leg, mode), v_ in us.items():
        out[leg]["us_" + mode] = _stats(v_)
    out["shape"] = {"energy_rows": B + 1, "force_rows": n_cap if forces else 0}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--workloads", default="qm9,md17,oc20")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_train_loops.py needs an MI355X"
    from equiformer_amd import lib
    lib.load()
    dev = torch.device("cuda:0")
    out = {"build": lib.built_hash()}
    for name in args.workloads.split(","):
        out[name] = run(name, dev, args.batches, args.repeats)
        torch.cuda.empty_cache()
        print(json.dumps({name: {k: out[name][k] for k in ("ratio_median", "aten_p10_over_loop_p90")}}), flush=True)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
