#!/usr/bin/env python
"""The DeNS and IS2RE + IS2RS training loops against the per-step read-back loop, one MI355X:

    python tools/bench_aux_loops.py [--batches 48] [--repeats 7] [--workloads dens,is2rs] [--out profiles/aux_loops.json]

Two workloads, full models in training mode, split matrix mode, 48 different batches each:
  dens   equiformer_md17_dens_l2, 8 aspirin frames per batch (168 atoms, fresh jitter per batch), r = 5, the corruption and
         the weights of tools/bench_dens.py, the denoising weight decayed linearly per pass
  is2rs  oc20_l1_256_nonlinear_aux, 16 slab structures of 60-96 atoms per batch with relaxed positions (pos + 0.2 A Gaussian on
         the free atoms), r = 5, max_neighbors = 500, as tools/bench_is2rs.py; a cosine lr_lambda and the auxiliary weight
         decaying from 15 over 100 passes
For each, from ONE process and ONE build, two legs over the same batches, each with its own model and FlatAdamW from the same
initial weights and the same step class (dens.DeNSTrainStep, is2rs.IS2RSTrainStep: captured, one HIP graph per bucket):
  (a) `readback`: what the parent commit allows -- a loop that writes the same schedules, then after every step reads
      `loss.stats` back (and, for IS2RS, the returned loss) and folds the figures into host-side AverageMeters;
  (b) `loop`: train.train_one_epoch_dens / train_one_epoch_is2rs on the steps of dens_train_step / is2rs_train_step (the
      meters folded on the device, read back once at the end of the pass).
One timed region = one pass over all batches, synchronised wall clock; the legs alternate.  Before the timed regions each leg
runs min_eager + 1 untimed passes (until its graphs exist).  Reports per workload and leg the median and the 10th / 90th
percentile of the milliseconds per batch over the repeats, and the counters.  Prints one JSON line."""
import argparse
import functools
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
from bench_train_loops import _Avg, _counters, _stats  # noqa: E402

RADIUS = 5.0
# tools/bench_dens.py
DENS_MODEL, FRAMES = "equiformer_md17_dens_l2", 8
STD, PROB, RATIO = 0.05, 0.5, 0.25
W_E, W_F, W_D = 1.0, 80.0, 5.0
TASK_MEAN, TASK_STD = 0.1, 1.3
EPOCHS = 300
# tools/bench_is2rs.py
IS2RS_MODEL, STRUCTURES, MAX_NEIGHBORS = "oc20_l1_256_nonlinear_aux", 16, 500
W0 = 15.0
NORM = dict(target_mean=-1.5, target_std=2.3, positions_mean=0.0, positions_std=0.4)
LR = 2e-4


def _seeded(make):
    torch.manual_seed(0)
    return make()


def dens(dev, n_batches):
    from equiformer_amd import nets, train
    from equiformer_amd.dens import DeNSLoss, DeNSTrainStep
    from equiformer_amd.optim import FlatAdamW
    from equiformer_amd.synthetic import md17_aspirin_batch
    batches = []
    for i in range(n_batches):
        d = md17_aspirin_batch(FRAMES, jitter=0.05, seed=1000 + i)
        batches.append({k: d[k].to(dev) for k in ("pos", "z", "batch", "y", "dy")})
        batches[-1]["num_graphs"] = FRAMES

    def make():
        return nets.model_entrypoint(DENS_MODEL)().to(dev).train()
    m_a = _seeded(make)
    opt_a = FlatAdamW(m_a.parameters(), lr=5e-4, weight_decay=1e-6)
    L = DeNSLoss(TASK_MEAN, TASK_STD, STD, W_E, W_F, W_D)
    ts_a = DeNSTrainStep(m_a, opt_a, L, RADIUS, STD, PROB, RATIO, seed=0)
    passes = [0, 0]

    def readback(bs):  # main_md17_dens.py:372-427 around the captured step: the stats read back after every step
        m_a.train()
        L.set_weights(denoising_pos_weight=train.dens_denoising_pos_weight(W_D, passes[0], EPOCHS))
        passes[0] += 1
        meters = [_Avg() for _ in train.DENS_METERS]
        for d in bs:
            ts_a.step(d)
            s = L.stats.tolist()
            for meter, (_, v, w) in zip(meters, train.DENS_METERS):
                n = FRAMES if w == train.GRAPHS else s[w]
                if n != 0:
                    meter.update(s[v], n)
        return meters[4].sum / meters[4].count

    m_b = _seeded(make)
    opt_b = FlatAdamW(m_b.parameters(), lr=5e-4, weight_decay=1e-6)
    ts_b = train.dens_train_step(m_b, opt_b, RADIUS, STD, PROB, W_E, W_F, W_D, corrupt_ratio=RATIO, task_mean=TASK_MEAN,
                                 task_std=TASK_STD, seed=0)

    def loop(bs):
        mae, _ = train.train_one_epoch_dens(ts_b, bs, passes[1], EPOCHS, W_D, linear_decay=True)
        passes[1] += 1
        return mae["force"].avg
    return dict(batches=batches, legs=dict(readback=(readback, ts_a.bucketed), loop=(loop, ts_b.bucketed)), units=FRAMES,
                text="DeNS %s, %d aspirin frames per batch (jitter 0.05 A), r=%.1f, std %.2f, prob %.2f, corrupt_ratio %.2f, "
                     "weights %g / %g / %g (linear decay over %d passes)" % (DENS_MODEL, FRAMES, RADIUS, STD, PROB, RATIO, W_E, W_F,
                                                                           W_D, EPOCHS))


def is2rs(dev, n_batches):
    from equiformer_amd import nets, train
    from equiformer_amd.is2rs import IS2RSLoss, IS2RSTrainStep, auxiliary_task_weight
    from equiformer_amd.optim import FlatAdamW
    from equiformer_amd.synthetic import oc20_like_varying_batches
    gen = torch.Generator().manual_seed(7)
    batches = []
    for d in oc20_like_varying_batches(n_batches, STRUCTURES, (60, 96), seed=1000):
        free = (d["tags"] > 0).view(-1, 1)
        d["pos_relaxed"] = torch.where(free, d["pos"] + 0.2 * torch.randn(d["pos"].shape, generator=gen), d["pos"])
        batches.append({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()})
    total = 100 * n_batches
    lam = functools.partial(train.lr_lambda_cosine, warmup=n_batches, warmup_factor=0.2, total=total, lr_min_factor=0.01)
    bucket = dict(node_step=64, edge_step=2048, max_graphs=16)

    def make():
        return nets.model_entrypoint(IS2RS_MODEL)(drop_path_rate=0.0).to(dev).train()  # (as tools/bench_is2rs.py)
    m_a = _seeded(make)
    opt_a = FlatAdamW(m_a.parameters(), lr=LR, weight_decay=1e-3)
    L = IS2RSLoss(auxiliary_task_weight=W0, **NORM)
    ts_a = IS2RSTrainStep(m_a, opt_a, L, RADIUS, MAX_NEIGHBORS, seed=0, **bucket)

    def readback(bs):  # energy_trainer_v2.py:252-288 around the captured step: loss.item() and the metrics after every step
        m_a.train()
        meters = [_Avg() for _ in train.IS2RS_METERS]
        for d in bs:
            k = ts_a.steps
            for g in opt_a.param_groups:
                g["lr"] = LR * lam(k)
            L.set_weights(auxiliary_task_weight=auxiliary_task_weight(W0, k + 1, total))
            loss = float(ts_a.step(d))
            s = L.stats.tolist()
            for meter, (_, v, w) in zip(meters, train.IS2RS_METERS):
                n = 1 if w == train.ONE else s[w]
                if n != 0:
                    meter.update(loss if v == train.LOSS else s[v], n)
        return meters[1].sum / meters[1].count

    m_b = _seeded(make)
    opt_b = FlatAdamW(m_b.parameters(), lr=LR, weight_decay=1e-3)
    ts_b = train.is2rs_train_step(m_b, opt_b, RADIUS, MAX_NEIGHBORS, auxiliary_task_weight=W0, seed=0, **NORM, **bucket)

    def loop(bs):
        return train.train_one_epoch_is2rs(ts_b, bs, lr_lambda=lam, total_steps=total)["energy_mae"].avg
    return dict(batches=batches, legs=dict(readback=(readback, ts_a.bucketed), loop=(loop, ts_b.bucketed)), units=STRUCTURES,
                text="IS2RE + IS2RS %s, %d slab structures of 60-96 atoms per batch, r=%.1f, max_neighbors=%d, auxiliary weight "
                     "from %g over %d steps, cosine lr" % (IS2RS_MODEL, STRUCTURES, RADIUS, MAX_NEIGHBORS, W0, total))


WORKLOADS = {"dens": dens, "is2rs": is2rs}


def run(name, dev, n_batches, repeats):
    w = WORKLOADS[name](dev, n_batches)
    batches, legs = w["batches"], w["legs"]

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
    res = {"what": w["text"], "unit": "ms per batch", "batches": len(batches), "units_per_batch": w["units"], "repeats": repeats}
    for leg, (_, s) in legs.items():
        c = _counters(s)
        res[leg] = dict(_stats(ms[leg]), warmup=warm[leg], timed={k: c[k] - warm[leg][k] for k in c},
                        live_graphs=len(s.live_graphs()))
    a, b = res["readback"], res["loop"]
    res["ratio_median"] = a["median"] / b["median"]
    res["loop_not_slower"] = b["p10"] <= a["p90"]      # the loop's fast end reaches the read-back loop's slow end
    res["ranges_separate"] = b["p90"] < a["p10"]       # a gain: the loop's slow end is faster than the read-back's fast end
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--workloads", default="dens,is2rs")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aux_loops.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_aux_loops.py needs an MI355X"
    from equiformer_amd import lib, ops
    lib.load()
    assert ops.get_matrix_mode() == "split"
    dev = torch.device("cuda:0")
    out = {"build": lib.built_hash()}
    for name in args.workloads.split(","):
        out[name] = run(name, dev, args.batches, args.repeats)
        torch.cuda.empty_cache()
        print(json.dumps({name: {k: out[name][k] for k in ("ratio_median", "loop_not_slower", "ranges_separate")}}), flush=True)
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
