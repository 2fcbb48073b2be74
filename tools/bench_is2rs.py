#!/usr/bin/env python
"""The IS2RE + IS2RS train step three ways, one MI355X, one process, one build:

    python tools/bench_is2rs.py [--batches 48] [--regions 3] [--out profiles/is2rs_step.json]
    python tools/bench_is2rs.py --drop-path-rate 0.05 --out profiles/is2rs_step_droppath.json
    python tools/bench_is2rs.py --out-drop 0.1 --out profiles/is2rs_step_outdrop.json

The `l1_256_nonlinear_aux` model (6 blocks, feature 512x0e+256x1e, IS2RS head; drop_path_rate 0 unless --drop-path-rate says
otherwise, see the end), 16 slab structures of 60-96 atoms per batch
(synthetic.oc20_like_varying_batches, as tools/bench_varying_oc20.py), relaxed positions = pos + 0.2 A Gaussian on the free
atoms, r = 5, max_neighbors = 500, the auxiliary weight decaying from 15.  Three loops over the same batches:
  (A) `aten`:     the step as the reference writes it (base_trainer_v2.py:81-126, energy_trainer_v2.py:413-442): ATen
                  perturbation with `batch.pos[tags] = new_pos[tags]`, the two L1 terms over boolean-indexed rows, the model
                  building its own periodic graph;
  (B) `fused`:    interpolate_init_relaxed_pos + IS2RSLoss, eager, unpadded;
  (C) `captured`: IS2RSTrainStep (one HIP graph per shape bucket).
Every step is timed on its own (device-synchronised wall clock); one region = one pass over all batches, the legs alternating
region by region; untimed passes first (the captured leg: min_eager + 1 of them, so that every bucket has its graph).  Median,
p10 and p90 of the step time and structures/s (real structures over the median step) per leg.  The launches of the perturbation
and of the loss + its backward ALONE (stand-in predictions, no model) are counted with the torch profiler for (A) and (B).

--drop-path-rate P > 0 (the shipped configuration: 0.05) times per-graph stochastic depth instead, four legs over the same
batches in one run, one model:
  `captured`:      IS2RSTrainStep, the keep mask drawn in the kernel from the step's device word (equiformer_amd/droppath.py);
  `eager_device`:  (B) under droppath.device_draws(step_seed(seed, k)): the same draws, launched from the host;
  `eager_host`:    (B) with the mask drawn from torch's CPU generator and uploaded, call by call -- the only way to train this
                   configuration without the device draw;
  `captured_p0`:   IS2RSTrainStep with the rate set to 0 while its graphs are captured: what stochastic depth costs a replay.

--out-drop P > 0 (the IS2RE-100k recipe `l1_256_nonlinear_aux_100k`: 0.1) times the dropout on the scalar channels in front of the
energy head (equiformer_amd/dropout.py), four legs over the same batches in one run, one model:
  `captured`:      IS2RSTrainStep, the mask drawn in eqf_irreps_dropout from the step's device word;
  `eager`:         (B) under droppath.device_draws(step_seed(seed, k)): the same draws, launched from the host;
  `captured_p0`, `eager_p0`: the same two with out_drop set to 0 while the step is launched or captured: what the dropout costs;
and the operator alone beside eqf_segment_scale at the feature shape (`dropout_alone`).
Prints one JSON line."""
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

MODEL = "oc20_l1_256_nonlinear_aux"
MODEL_100K = "oc20_l1_256_nonlinear_aux_100k"    # the IS2RE-100k recipe: alpha_drop 0.1, out_drop 0.1, no stochastic depth
RADIUS, MAX_NEIGHBORS = 5.0, 500
W0 = 15.0                                    # auxiliary_task_weight of the shipped _aux configurations
E_MEAN, E_STD = -1.5, 2.3                    # stand-in statistics
P_MEAN, P_STD = 0.0, 0.4


def aten_perturb(batch):
    """The perturbation in the ATen formulation of base_trainer_v2.py:81-126, restated from its formulas: a per-structure coin
    gathered to the atoms, a per-atom factor, per-component noise, dense blends over all atoms, and the boolean-index assignment
    of the free atoms (the uniform-direction noise of :98-106, which :108 overwrites, left out)."""
    pos, dev = batch.pos, batch.pos.device
    n = pos.shape[0]
    structures = batch.batch.max() + 1                                          # (a device scalar: read back by the next line)
    coin = torch.floor(torch.rand((structures, 1), device=dev) + 0.5)[batch.batch]  # 1 with probability 1/2, per atom
    f = torch.empty((n, 1), device=dev).uniform_(0.0, 1.0)
    noise = torch.empty((n, 3), device=dev).normal_(0.0, 0.3)
    moved = (pos * f + (1 - f) * batch.pos_relaxed) + noise
    blended = moved * coin + pos * (1 - coin)
    free = batch.tags > 0
    batch.pos[free] = blended[free]
    return batch


def aten_loss(energy, vectors, batch, weight):
    """The `mae` / `mae` loss in the ATen formulation of energy_trainer_v2.py:413-442: L1 on the normalised energy plus the
    weighted L1 over the boolean-indexed free rows of the normalised displacement."""
    l_e = torch.nn.functional.l1_loss(energy.view(-1), (batch.y - E_MEAN) / E_STD)
    target = ((batch.pos_relaxed - batch.pos) - P_MEAN) / P_STD
    free = batch.tags > 0
    l_aux = torch.nn.functional.l1_loss(vectors[free], target[free])
    return l_e + weight * l_aux


def count_launches(fn, iters=4):
    """device activities per call of fn (kernels, and copies / fills apart), from the torch profiler"""
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    copies = sum(1 for e in evs if e.name.lower().startswith(("memcpy", "memset", "copy", "fill")))
    return {"kernels": (len(evs) - copies) / iters, "copies_and_fills": copies / iters}


def summary(v, B):
    s = sorted(v)
    q = lambda p: s[min(len(s) - 1, int(round(p * (len(s) - 1))))]  # noqa: E731
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "structures_per_s": B / (q(0.5) * 1e-3), "steps": len(s)}


def row_scaling_alone(rate, rows=1248, D=768, graphs=16, launches=200, repeats=7):
    """The two row scalings alone on [rows, D] (16 structures of 78 atoms, the feature width 512x0e+256x1e): eqf_segment_droppath
    (factor drawn in the kernel) against eqf_segment_scale (factor read from a table).  Device events around `launches`
    back-to-back launches, the two alternating, median over `repeats` blocks: microseconds per launch INCLUDING the rate at which
    the host launches -- not a kernel time."""
    from equiformer_amd import droppath, ops
    dev = torch.device("cuda:0")
    x = torch.randn(rows, D, device=dev)
    seg = torch.repeat_interleave(torch.arange(graphs, dtype=torch.int32), rows // graphs).to(dev)
    f = droppath.keep_factors(0, 0, graphs, rate).to(dev)
    fns = {"segment_droppath": lambda: droppath.segment_droppath(x, seg, rate, 0, 0),
           "segment_scale": lambda: ops.segment_scale(x, f, seg)}
    assert torch.equal(fns["segment_droppath"](), fns["segment_scale"]())
    us = {k: [] for k in fns}
    for _ in range(repeats + 1):  # (the first block of each: untimed warm-up)
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            torch.cuda.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / launches)
    med = {k: sorted(v[1:])[len(v[1:]) // 2] for k, v in us.items()}
    return {"rows": rows, "D": D, "graphs": graphs, "us_per_launch": med, "blocks": {k: v[1:] for k, v in us.items()},
            "bytes_moved": 8 * rows * D,
            "how": "device events around %d back-to-back launches through the Python operator, alternating, median of %d blocks; "
                   "includes the host's launch rate" % (launches, repeats)}


def stochastic_depth_legs(args, rate, batches, B, lib, ts, ts0, L, legs):
    """--drop-path-rate > 0: the four legs of the module docstring, timed as the default run times its three"""
    def one_pass(step):
        out = []
        for d in batches:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(d)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    for name, step in legs:  # untimed: one pass of the eager legs, min_eager + 1 of the captured ones (every bucket has its graph)
        for _ in range(ts.bucketed.min_eager + 1 if name.startswith("captured") else 1):
            one_pass(step)
    warm = {n: dict(eager_steps=t.eager_steps, captures=t.captures, replays=t.replays) for n, t in (("captured", ts), ("captured_p0", ts0))}
    ms = {name: [] for name, _ in legs}
    for _ in range(args.regions):
        for name, step in legs:
            ms[name] += one_pass(step)
    res = {name: summary(v, B) for name, v in ms.items()}
    out = {
        "what": "IS2RE + IS2RS train step with per-graph stochastic depth, %s (drop_path_rate %g), %d different batches of %d slab "
                "structures (%d-%d atoms), r=%.1f, max_neighbors=%d, split mode, one process, one model; device-synchronised wall "
                "time per step, one region = one pass over all batches, legs alternating"
                % (MODEL, rate, len(batches), B, args.atoms_min, args.atoms_max, RADIUS, MAX_NEIGHBORS),
        "build": lib.built_hash(), "regions": args.regions, "drop_path_rate": rate,
    }
    out.update(res)
    out["captured_range_ms"] = res["captured"]["p90_ms"] - res["captured"]["p10_ms"]
    out["eager_host_range_ms"] = res["eager_host"]["p90_ms"] - res["eager_host"]["p10_ms"]
    out["captured_over_eager_host"] = res["eager_host"]["median_ms"] / res["captured"]["median_ms"]
    out["captured_over_eager_device"] = res["eager_device"]["median_ms"] / res["captured"]["median_ms"]
    out["cost_over_captured_p0_ms"] = res["captured"]["median_ms"] - res["captured_p0"]["median_ms"]
    out["row_scaling_alone"] = row_scaling_alone(rate)
    out["warmup"] = warm
    out["captured_timed"] = {n: dict(eager_steps=t.eager_steps - warm[n]["eager_steps"], captures=t.captures - warm[n]["captures"],
                                     replays=t.replays - warm[n]["replays"], live_graphs=len(t.bucketed.live_graphs()))
                             for n, t in (("captured", ts), ("captured_p0", ts0))}
    out["last_stats"] = dict(zip(("loss_e", "loss_aux", "n_free", "energy_mae", "energy_mse", "energy_within_threshold", "pos_mae"),
                                 L.stats.cpu().tolist()))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


def dropout_alone(rate, rows=1248, irreps="512x0e+256x1e", graphs=16, launches=200, repeats=9):
    """eqf_irreps_dropout alone at the OC20 feature shape (16 structures of 78 atoms x 512x0e+256x1e, D = 1280) beside
    eqf_segment_scale -- an existing kernel that moves the same bytes -- in one process.  Two ways, both with device events
    around `launches` launches, the operators alternating, `repeats` blocks after one untimed block each: launched back to back
    through the Python operators (includes the host's launch rate), and the same launches replayed from one captured HIP graph
    per operator (the device's own pace).  Microseconds per launch: median, p10 and p90 over the blocks."""
    from equiformer_amd import dropout, droppath, ops
    from equiformer_amd.layout import RowLayout
    dev = torch.device("cuda:0")
    lay = RowLayout(irreps)
    x = torch.randn(rows, lay.dim, device=dev)
    seg = torch.repeat_interleave(torch.arange(graphs, dtype=torch.int32), rows // graphs).to(dev)
    f = droppath.keep_factors(0, 0, graphs, rate).to(dev)
    fns = {"irreps_dropout_scalars": lambda: dropout.irreps_dropout(x, lay, rate, 0, 0, scalars_only=True),
           "irreps_dropout_all": lambda: dropout.irreps_dropout(x, lay, rate, 0, 0),
           "segment_scale": lambda: ops.segment_scale(x, f, seg)}
    for so in (True, False):
        want = x * dropout.keep_mask(0, 0, rows, lay, rate, so, expand="cf").to(dev)
        assert torch.equal(fns["irreps_dropout_scalars" if so else "irreps_dropout_all"](), want)

    def timed(run):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / launches

    def many(fn):
        for _ in range(launches):
            fn()

    def stats(v):
        s = sorted(v)
        q = lambda p: s[min(len(s) - 1, int(round(p * (len(s) - 1))))]  # noqa: E731
        return {"median": q(0.5), "p10": q(0.1), "p90": q(0.9)}

    eager = {k: [] for k in fns}
    for _ in range(repeats + 1):  # (the first block of each: untimed warm-up)
        for k, fn in fns.items():
            eager[k].append(timed(lambda: many(fn)))
    out = {"rows": rows, "irreps": irreps, "D": lay.dim, "bytes_moved": 8 * rows * lay.dim, "launches_per_block": launches, "blocks": repeats,
           "us_per_launch": {k: stats(v[1:]) for k, v in eager.items()},
           "how": "device events around %d launches, the operators alternating, %d blocks after one untimed block; us_per_launch: back "
                  "to back through the Python operators (includes the host's launch rate); us_per_launch_in_graph: the same launches "
                  "replayed from one captured HIP graph per operator" % (launches, repeats)}
    try:  # (a capture that does not come up must not cost the other timings)
        graphs_of, replay = {}, {k: [] for k in fns}
        side = torch.cuda.Stream()
        for k, fn in fns.items():
            with torch.cuda.stream(side):
                many(fn)  # (warm-up on the capture stream: allocator and kernels loaded)
                torch.cuda.synchronize()
                graphs_of[k] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs_of[k], stream=side):
                    many(fn)
            torch.cuda.synchronize()
        for _ in range(repeats + 1):
            for k in fns:
                replay[k].append(timed(graphs_of[k].replay))
        out["us_per_launch_in_graph"] = {k: stats(v[1:]) for k, v in replay.items()}
    except Exception as exc:
        out["us_per_launch_in_graph_error"] = "%s: %s" % (type(exc).__name__, exc)
    for key in ("us_per_launch", "us_per_launch_in_graph"):
        if key not in out:
            continue
        d, s = out[key]["irreps_dropout_scalars"], out[key]["segment_scale"]
        out[key]["ratio_scalars_over_segment_scale"] = d["median"] / s["median"]
        out[key]["p10_p90_overlap"] = d["p10"] <= s["p90"] and s["p10"] <= d["p90"]
    return out


def out_drop_legs(args, rate, batches, B, lib, ts, ts0, L, legs):
    """--out-drop > 0: the four legs of the module docstring, timed as the default run times its three"""
    def one_pass(step):
        out = []
        for d in batches:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(d)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    for name, step in legs:  # untimed: one pass of the eager legs, min_eager + 1 of the captured ones (every bucket has its graph)
        for _ in range(ts.bucketed.min_eager + 1 if name.startswith("captured") else 1):
            one_pass(step)
    warm = {n: dict(eager_steps=t.eager_steps, captures=t.captures, replays=t.replays) for n, t in (("captured", ts), ("captured_p0", ts0))}
    ms = {name: [] for name, _ in legs}
    for _ in range(args.regions):
        for name, step in legs:
            ms[name] += one_pass(step)
    res = {name: summary(v, B) for name, v in ms.items()}
    out = {
        "what": "IS2RE + IS2RS train step with dropout on the scalar channels in front of the energy head, %s (alpha_drop 0.1, out_drop "
                "%g, no stochastic depth), %d different batches of %d slab structures (%d-%d atoms), r=%.1f, max_neighbors=%d, split "
                "mode, one process, one model; device-synchronised wall time per step, one region = one pass over all batches, legs "
                "alternating; the _p0 legs: the same model with out_drop set to 0 while its steps are launched or captured"
                % (MODEL_100K, rate, len(batches), B, args.atoms_min, args.atoms_max, RADIUS, MAX_NEIGHBORS),
        "build": lib.built_hash(), "regions": args.regions, "out_drop": rate,
    }
    out.update(res)
    for name in res:
        out[name + "_range_ms"] = res[name]["p90_ms"] - res[name]["p10_ms"]
    out["captured_over_eager"] = res["eager"]["median_ms"] / res["captured"]["median_ms"]
    out["cost_over_captured_p0_ms"] = res["captured"]["median_ms"] - res["captured_p0"]["median_ms"]
    out["cost_over_eager_p0_ms"] = res["eager"]["median_ms"] - res["eager_p0"]["median_ms"]
    out["operator_alone"] = dropout_alone(rate)
    out["warmup"] = warm
    out["captured_timed"] = {n: dict(eager_steps=t.eager_steps - warm[n]["eager_steps"], captures=t.captures - warm[n]["captures"],
                                     replays=t.replays - warm[n]["replays"], live_graphs=len(t.bucketed.live_graphs()))
                             for n, t in (("captured", ts), ("captured_p0", ts0))}
    out["last_stats"] = dict(zip(("loss_e", "loss_aux", "n_free", "energy_mae", "energy_mse", "energy_within_threshold", "pos_mae"),
                                 L.stats.cpu().tolist()))
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


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
    ap.add_argument("--drop-path-rate", type=float, default=0.0)
    ap.add_argument("--out-drop", type=float, default=0.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "is2rs_step.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_is2rs.py needs an MI355X"
    from equiformer_amd import droppath, lib, nets, ops
    from equiformer_amd.is2rs import IS2RSLoss, IS2RSTrainStep, auxiliary_task_weight, interpolate_init_relaxed_pos, step_seed
    from equiformer_amd.nets.layers import GraphDropPath
    from equiformer_amd.optim import FlatAdamW, add_weight_decay
    from equiformer_amd.synthetic import oc20_like_varying_batches
    lib.load()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B = args.structures
    assert ops.get_matrix_mode() == "split"
    rate = float(args.drop_path_rate)
    out_drop = float(args.out_drop)
    assert not (rate > 0.0 and out_drop > 0.0), "--drop-path-rate and --out-drop are two runs"
    if out_drop > 0.0:
        model = nets.model_entrypoint(MODEL_100K)(out_drop=out_drop).to(dev).train()
    else:
        model = nets.model_entrypoint(MODEL)(drop_path_rate=rate).to(dev).train()
    drop_modules = [m for m in model.modules() if isinstance(m, GraphDropPath)]

    def set_rate(p):  # (read when a step is launched from the host: an eager step or a capture, never a replay)
        for m in drop_modules:
            m.drop_prob = p
    opt = FlatAdamW(add_weight_decay(model, 1e-3, model.no_weight_decay()), lr=2e-4)
    gen = torch.Generator().manual_seed(7)
    batches = []
    for d in oc20_like_varying_batches(args.batches, B, (args.atoms_min, args.atoms_max), seed=1000):
        free = (d["tags"] > 0).view(-1, 1)
        d["pos_relaxed"] = torch.where(free, d["pos"] + 0.2 * torch.randn(d["pos"].shape, generator=gen), d["pos"])
        batches.append({k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()})
    total_steps = 100 * len(batches)  # the decay of a run of 100 passes: the weight changes every step, slowly
    L = IS2RSLoss(E_MEAN, E_STD, P_MEAN, P_STD, W0)
    ts = IS2RSTrainStep(model, opt, L, RADIUS, MAX_NEIGHBORS, interpolate=True, seed=0, total_steps=total_steps,
                        auxiliary_task_weight=W0, node_step=args.node_step, edge_step=args.edge_step, max_graphs=args.max_graphs)
    counter = {"aten": 0, "fused": 0}

    def step_aten(d):
        data = SimpleNamespace(**dict(d, pos=d["pos"].clone()))  # (the loader's fresh batch: the perturbation is in place)
        aten_perturb(data)
        w = auxiliary_task_weight(W0, counter["aten"], total_steps)
        counter["aten"] += 1
        opt.zero_grad(set_to_none=True)
        energy, vectors = model(data)
        aten_loss(energy, vectors, data, w).backward()
        opt.step()

    def step_fused(d):
        data = SimpleNamespace(**d)
        interpolate_init_relaxed_pos(data, seed=counter["fused"])
        L.set_weights(auxiliary_task_weight=auxiliary_task_weight(W0, counter["fused"], total_steps))
        counter["fused"] += 1
        opt.zero_grad(set_to_none=True)
        energy, vectors = model(data)
        L(energy, vectors, data).backward()
        opt.step()

    legs = [("aten", step_aten), ("fused", step_fused), ("captured", ts.step)]
    if out_drop > 0.0:
        ts0 = IS2RSTrainStep(model, opt, L, RADIUS, MAX_NEIGHBORS, interpolate=True, seed=0, total_steps=total_steps,
                             auxiliary_task_weight=W0, node_step=args.node_step, edge_step=args.edge_step,
                             max_graphs=args.max_graphs)
        counter["device"] = 0

        def step_eager(d):  # (the draws of the captured leg, launched from the host)
            with droppath.device_draws(step_seed(0, counter["device"])):
                counter["device"] += 1
                step_fused(d)

        def at_rate_zero(step):  # (the rate is read when a step is launched from the host: an eager step or a capture, never a replay)
            def run(d):
                model.out_dropout.drop_prob = 0.0
                try:
                    step(d)
                finally:
                    model.out_dropout.drop_prob = out_drop
            return run
        return out_drop_legs(args, out_drop, batches, B, lib, ts, ts0, L,
                             [("captured", ts.step), ("eager", step_eager), ("captured_p0", at_rate_zero(ts0.step)),
                              ("eager_p0", at_rate_zero(step_eager))])
    if rate > 0.0:
        ts0 = IS2RSTrainStep(model, opt, L, RADIUS, MAX_NEIGHBORS, interpolate=True, seed=0, total_steps=total_steps,
                             auxiliary_task_weight=W0, node_step=args.node_step, edge_step=args.edge_step,
                             max_graphs=args.max_graphs)
        counter["device"] = 0

        def step_device(d):
            with droppath.device_draws(step_seed(0, counter["device"])):
                counter["device"] += 1
                step_fused(d)

        def step_p0(d):
            set_rate(0.0)
            try:
                ts0.step(d)
            finally:
                set_rate(rate)
        return stochastic_depth_legs(args, rate, batches, B, lib, ts, ts0, L,
                                     [("captured", ts.step), ("eager_device", step_device), ("eager_host", step_fused),
                                      ("captured_p0", step_p0)])

    def one_pass(step):
        out = []
        for d in batches:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(d)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    # the perturbation and the loss alone, on the first batch with stand-in predictions
    d0 = batches[0]
    n0 = d0["pos"].shape[0]
    pred_y = torch.randn(B, 1, generator=gen).to(dev).requires_grad_(True)
    pred_pos = torch.randn(n0, 3, generator=gen).to(dev).requires_grad_(True)
    fresh = lambda: SimpleNamespace(**dict(d0, pos=d0["pos"].clone()))  # noqa: E731
    held = fresh()

    def loss_only(fn):
        pred_y.grad = pred_pos.grad = None
        fn().backward()
    try:
        launches = {
            "perturbation": {"aten": count_launches(lambda: aten_perturb(held)),
                             "fused": count_launches(lambda: interpolate_init_relaxed_pos(SimpleNamespace(**d0), seed=1))},
            "loss_and_backward": {"aten": count_launches(lambda: loss_only(lambda: aten_loss(pred_y, pred_pos, held, W0))),
                                  "fused": count_launches(lambda: loss_only(lambda: L(pred_y, pred_pos, held)))},
            "how": "torch profiler, device activities per call over 4 calls after one untimed call; the aten perturbation counted "
                   "without the clone of pos that stands in for the loader's fresh batch",
        }
    except Exception as exc:  # (a profiler that does not come up must not cost the timings)
        launches = {"error": "%s: %s" % (type(exc).__name__, exc)}

    one_pass(step_aten)
    one_pass(step_fused)
    t_cap0 = time.perf_counter()
    for _ in range(ts.bucketed.min_eager + 1):
        one_pass(ts.step)
    t_cap = time.perf_counter() - t_cap0
    warm = dict(eager_steps=ts.eager_steps, captures=ts.captures, replays=ts.replays, evictions=ts.bucketed.evictions,
                seconds=t_cap, passes=ts.bucketed.min_eager + 1)
    ms = {name: [] for name, _ in legs}
    for _ in range(args.regions):
        for name, step in legs:  # alternating: a drift of the box's clocks reaches every leg alike
            ms[name] += one_pass(step)

    res = {name: summary(v, B) for name, v in ms.items()}
    bk = ts.bucketed
    out = {
        "what": "IS2RE + IS2RS train step, %s (drop_path_rate 0), %d different batches of %d slab structures (%d-%d atoms), r=%.1f, "
                "max_neighbors=%d, split mode, one process; device-synchronised wall time per step, one region = one pass over all "
                "batches, legs alternating" % (MODEL, len(batches), B, args.atoms_min, args.atoms_max, RADIUS, MAX_NEIGHBORS),
        "build": lib.built_hash(),
        "regions": args.regions,
        "aten": res["aten"], "fused": res["fused"], "captured": res["captured"],
        "fused_over_aten": res["aten"]["median_ms"] / res["fused"]["median_ms"],
        "captured_over_aten": res["aten"]["median_ms"] / res["captured"]["median_ms"],
        "captured_over_fused": res["fused"]["median_ms"] / res["captured"]["median_ms"],
        "launches": launches,
        "warmup": warm,
        "captured_timed": {"eager_steps": ts.eager_steps - warm["eager_steps"], "captures": ts.captures - warm["captures"],
                           "replays": ts.replays - warm["replays"], "evictions": bk.evictions - warm["evictions"],
                           "live_graphs": len(bk.live_graphs())},
        "node_step": bk.node_step, "edge_step": bk.edge_step, "min_eager": bk.min_eager, "max_graphs": bk.max_graphs,
        "padded_edge_share": 1.0 - bk.real_edges / bk.padded_edges,
        "padded_node_share": 1.0 - bk.real_nodes / bk.padded_nodes,
        "last_stats": dict(zip(("loss_e", "loss_aux", "n_free", "energy_mae", "energy_mse", "energy_within_threshold", "pos_mae"),
                               L.stats.cpu().tolist())),
    }
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
