#!/usr/bin/env python
"""OC20 prediction pass (the trainer's `predict`, energy_trainer_v2.py:134-225) over periodic batches whose atom and edge counts
change every batch, one MI355X:

    python tools/bench_predict_oc20.py [--batches 48] [--passes 9] [--out profiles/predict_oc20.json]

The 48 batches of 16 slab structures of tools/bench_varying_oc20.py (60-96 atoms, 11 x 11 x 30 A cell, seed 1000), two models:
`oc20_l1_256_nonlinear_aux` with write_pos and `oc20_l1_256_nonlinear` without.  From ONE process and ONE build, per model,
milliseconds per batch of
  (a) `predict`:    equiformer_amd.evaluate.predict_oc20 -- padded to the bucket, one HIP graph per bucket, energies / ids /
                    positions appended on the device, one read-back per pass;
  (b) `evaluate`:   equiformer_amd.evaluate.evaluate_oc20 on the same model and batches (the validation pass: the same
                    forward, a meter update instead of the append) -- what the prediction pass may cost at most;
  (c) `eager_loop`: the reference-shaped loop: `model(data)` on the unpadded batch (the model builds its periodic graph),
                    denormalisation in ATen, `.tolist()` on ids and energies and, with write_pos, the two boolean indices,
                    `natoms.tolist()`, `torch.split` and `.cpu()` per structure, every batch.
One sample = one pass over all batches (synchronised wall clock) divided by the number of batches; the legs alternate, `--passes`
samples each; reported: median and the 10th / 90th percentile.  Before the timed passes every leg runs untimed passes until its
graphs exist (min_eager + 1).  `faster_than` is claimed only where the p10-p90 ranges do not overlap.  Prints one JSON line."""
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

MODELS = (("oc20_l1_256_nonlinear_aux", True), ("oc20_l1_256_nonlinear", False))
# a target and a positions normalizer (configuration constants of a run; their values do not enter the timing)
NORM = dict(target_mean=-0.7554, target_std=2.887, positions_mean=(0.0, 0.0, 0.0), positions_std=(0.1119, 0.1119, 0.1119))


def _quantile(v, q):
    v = sorted(v)
    x = q * (len(v) - 1)
    i = int(x)
    return v[i] if i + 1 >= len(v) else v[i] + (x - i) * (v[i + 1] - v[i])


def _summary(v):
    return {"median": _quantile(v, 0.5), "p10": _quantile(v, 0.1), "p90": _quantile(v, 0.9), "values": v}


def bench_model(name, write_pos, batches, args, dev):
    from equiformer_amd import evaluate, nets
    torch.manual_seed(0)
    model = nets.model_entrypoint(name)().to(dev).eval()
    radius, cap = float(model.max_radius), int(model.max_neighbors)
    bucket = dict(max_num_neighbors=cap, node_step=args.node_step, edge_step=args.edge_step, max_graphs=args.max_graphs)
    pstep = evaluate.oc20_predict_step(model, radius, write_pos=write_pos, **NORM, **bucket)
    estep = evaluate.oc20_eval_step(model, radius, task_mean=NORM["target_mean"], task_std=NORM["target_std"], **bucket)
    e_std, e_mean = torch.tensor(NORM["target_std"], device=dev), torch.tensor(NORM["target_mean"], device=dev)
    p_std, p_mean = torch.tensor(NORM["positions_std"], device=dev), torch.tensor(NORM["positions_mean"], device=dev)

    def eager_loop():
        predictions, pos_preds = {"id": [], "energy": []}, {}
        with torch.no_grad():
            for d in batches:
                out = model(SimpleNamespace(pos=d["pos"], batch=d["batch"], atomic_numbers=d["atomic_numbers"], tags=d["tags"],
                                            cell=d["cell"], natoms=d["natoms"]))
                energy, delta = out if isinstance(out, tuple) else (out, None)
                energy = energy.view(-1) * e_std + e_mean
                predictions["id"].extend([str(i) for i in d["sid"].tolist()])
                predictions["energy"].extend(energy.tolist())
                if write_pos:
                    delta = delta * p_std + p_mean
                    mask = d["tags"] > 0
                    pred = d["pos"].clone()  # (the reference moves the batch's own tensor; the batches here are reused)
                    pred[mask] = pred[mask] + delta[mask]
                    sids = [str(s) for s in d["sid"].tolist()]
                    for s, p in zip(sids, torch.split(pred, d["natoms"].tolist())):
                        pos_preds[s] = p.detach().cpu()
        if write_pos:
            predictions["pos"] = pos_preds
        return predictions

    legs = [("predict", lambda: evaluate.predict_oc20(model, batches, radius, step=pstep, write_pos=write_pos)),
            ("evaluate", lambda: evaluate.evaluate_oc20(model, batches, radius, step=estep)),
            ("eager_loop", eager_loop)]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / len(batches), out

    results = {}
    for leg, fn in legs:  # warm-up: clocks, allocator pools, every bucket's graph
        for _ in range(pstep.min_eager + 1):
            results[leg] = timed(fn)[1]
    warm = {k: dict(replays=s.replays, eager_steps=s.eager_steps, captures=s.captures, evictions=s.evictions)
            for k, s in (("predict", pstep), ("evaluate", estep))}
    # the legs agree on what they predict
    got, want = results["predict"], results["eager_loop"]
    assert got["id"] == want["id"] and len(got["id"]) == sum(int(d["sid"].shape[0]) for d in batches)
    e_got, e_want = torch.tensor(got["energy"], dtype=torch.float64), torch.tensor(want["energy"], dtype=torch.float64)
    agree = {"energy_rel": float((e_got - e_want).abs().max() / e_want.abs().max())}
    if write_pos:
        agree["pos_abs"] = max(float((got["pos"][s].double() - want["pos"][s].double()).abs().max()) for s in want["pos"])
    times = {leg: [] for leg, _ in legs}
    for _ in range(args.passes):
        for leg, fn in legs:  # alternating: a drift of the box's clocks reaches every leg alike
            times[leg].append(timed(fn)[0])
    out = {leg: _summary(v) for leg, v in times.items()}
    out["unit"] = "ms per batch"
    out["write_pos"] = write_pos
    out["agreement_with_eager_loop"] = agree
    out["faster_than"] = {"predict_vs_eager_loop": out["predict"]["p90"] < out["eager_loop"]["p10"],
                          "evaluate_vs_predict": out["evaluate"]["p90"] < out["predict"]["p10"],
                          "predict_vs_evaluate": out["predict"]["p90"] < out["evaluate"]["p10"]}
    out["warmup"] = warm
    out["timed"] = {k: dict(replays=s.replays - warm[k]["replays"], eager_steps=s.eager_steps - warm[k]["eager_steps"],
                            captures=s.captures - warm[k]["captures"]) for k, s in (("predict", pstep), ("evaluate", estep))}
    out["live_graphs"] = len(pstep.live_graphs())
    out["sink"] = {"graph_capacity": pstep.sink.graph_capacity, "atom_capacity": pstep.sink.atom_capacity}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=48)
    ap.add_argument("--structures", type=int, default=16)
    ap.add_argument("--atoms-min", type=int, default=60)
    ap.add_argument("--atoms-max", type=int, default=96)
    ap.add_argument("--passes", type=int, default=9)
    ap.add_argument("--node-step", type=int, default=64)
    ap.add_argument("--edge-step", type=int, default=2048)
    ap.add_argument("--max-graphs", type=int, default=16)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_predict_oc20.py needs an MI355X"
    from equiformer_amd import lib
    from equiformer_amd.synthetic import oc20_like_varying_batches
    lib.load()
    dev = torch.device("cuda:0")
    batches = []
    for k, d in enumerate(oc20_like_varying_batches(args.batches, args.structures, (args.atoms_min, args.atoms_max), seed=1000)):
        d = {k2: (v.to(dev) if torch.is_tensor(v) else v) for k2, v in d.items()}
        d["sid"] = torch.arange(k * args.structures, (k + 1) * args.structures, device=dev) * 7919 % 1000003
        batches.append(d)
    out = {
        "what": "OC20 prediction pass over %d different batches of %d slab structures (%d-%d atoms, 11 x 11 x 30 A cell), split "
                "mode; milliseconds per batch, one sample = one pass over all batches (synchronised wall clock) / batches, %d "
                "samples per leg, legs alternating" % (len(batches), args.structures, args.atoms_min, args.atoms_max, args.passes),
        "build": lib.built_hash(),
        "passes": args.passes, "node_step": args.node_step, "edge_step": args.edge_step, "max_graphs": args.max_graphs,
        "atoms": sum(int(d["pos"].shape[0]) for d in batches),
        "models": {name: bench_model(name, write_pos, batches, args, dev) for name, write_pos in MODELS},
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
