#!/usr/bin/env python
"""EdgeDegreeEmbeddingNetwork alone at the bench size (QM9 irreps, 128 molecules x 18 atoms, E ~ 25 k): forward + backward of
the collapsed path (csrc/edgedeg.hip: fold, one E x 64 GEMM, segmented scatter) and of the fused SeparableFCTP path,
ALTERNATING in one process, each with its own radial MLP un-banked (both run its first two layers; the fused path also runs
the 64 -> 960 last layer the collapsed one folds away).  Prints the median microseconds per path and the kernels each launches.

    python tools/bench_edge_degree.py [--reps 30] [--out profiles/edge_degree/operator_alone.txt]
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from equiformer_amd import ops  # noqa: E402
from equiformer_amd.graph import EdgeGraph  # noqa: E402
from equiformer_amd.nets.layers import EdgeContext, EdgeDegreeEmbeddingNetwork  # noqa: E402
from equiformer_amd.synthetic import qm9_like_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = EdgeDegreeEmbeddingNetwork("128x0e+64x1e+32x2e", "1x0e+1x1e+1x2e", [128, 64, 64], 15.57930850982666).to(dev)
    d = {k: v.to(dev) for k, v in qm9_like_batch(args.batch, 18, side=6.5, seed=1000).items()}
    g = EdgeGraph.from_radius(d["pos"], d["batch"], 5.0, num_graphs=args.batch)
    _, _, sh = ops.edge_geometry(d["pos"], None, g, 2)
    sh = sh.detach()
    es = torch.randn(g.E, 128, device=dev)
    gout = torch.randn(g.N, m.D, device=dev)

    def step(collapsed):
        m.use_collapsed = collapsed
        m.zero_grad(set_to_none=True)
        ectx = EdgeContext(g, sh, es, hidden_only=[m.rad] if collapsed else [])
        ectx.coupling(m.dw.table)
        out = m(gout, ectx)
        out.backward(gout)

    times = {True: [], False: []}
    for _ in range(3):
        step(True), step(False)
    torch.cuda.synchronize()
    for _ in range(args.reps):
        for collapsed in (True, False):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(collapsed)
            b.record()
            torch.cuda.synchronize()
            times[collapsed].append(a.elapsed_time(b) * 1e3)
    lines = ["EdgeDegreeEmbeddingNetwork forward + backward, N = %d, E = %d, %s, matrix mode %s, %d alternating repetitions "
             "(stream time between two events, host launch gaps included)"
             % (g.N, g.E, torch.cuda.get_device_name(0), ops.get_matrix_mode(), args.reps)]
    for collapsed in (True, False):
        t = sorted(times[collapsed])
        lines.append("%-9s median %7.1f us  min %7.1f  max %7.1f" % ("collapsed" if collapsed else "fused", statistics.median(t),
                                                                    t[0], t[-1]))
    from torch.profiler import ProfilerActivity, profile
    for collapsed in (True, False):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step(collapsed)
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        lines.append("%s launches (%d, %.1f us of kernel time):" % ("collapsed" if collapsed else "fused", len(evs),
                                                                    sum(e.device_time for e in evs)))
        lines += ["  %7.1f us  %s" % (e.device_time, e.name[:110]) for e in evs]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
