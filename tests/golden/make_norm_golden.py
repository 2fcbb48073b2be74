#!/usr/bin/env python
"""Fixtures of the graph, instance and fast layer norms, computed by the REFERENCE'S OWN model classes.

    python tests/golden/make_norm_golden.py [--reference DIR]            # check the stored fixtures (default)
    python tests/golden/make_norm_golden.py [--reference DIR] --write    # rewrite tests/golden/norms/

oracle/nets.py restates `norm_layer='layer'` only, so these fixtures come straight from the reference's `nets` package
(imported unchanged, fp64, through the helpers of make_reference_golden.py) with the name-keyed weights of
tests/golden/weights.py filled into the reference model itself (float32-rounded values; `mean_shift` gets 0.15 * randn,
far from its initial ones).  They live in tests/golden/norms/, not beside the older fixtures: make_reference_golden.py
asks every .npz of tests/golden/ itself for an oracle run.

  norms/qm9_graph.npz, norms/qm9_instance.npz   SMALL_L2, three molecules of 6, 10 and 15 atoms (each its own input):
      energies, loss and the gradients GRAD_NAMES  [ref: nets/graph_norm.py:9-134, nets/instance_norm.py:9-134 under
      GraphAttentionTransformer.forward, nets/graph_attention_transformer.py:864-899]
  norms/md17_graph.npz                          SMALL_L2 on the inputs of md17_small_l2.npz: energy and forces
  norms/param_tables.json                       per norm type: parameter names / shapes in registration order and
      no_weight_decay() of the QM9 and the MD17 model [ref: get_norm_layer :39-51, no_weight_decay :843-861]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_golden as mrg  # noqa: E402
from make_golden import SMALL_L2  # noqa: E402
from weights import fill_deterministic  # noqa: E402

OUT = os.path.join(HERE, "norms")
NORM_TYPES = ("layer", "graph", "instance", "fast_layer")
QM9_KW = dict(irreps_in="5x0e", max_radius=5.0, number_of_basis=32, **SMALL_L2)
MD17_KW = dict(irreps_in="64x0e", max_radius=5.0, number_of_basis=32, basis_type="exp", **SMALL_L2)
QM9_CASES = {"qm9_graph": ("graph", 21, 32), "qm9_instance": ("instance", 22, 33)}  # tag: norm type, weight seed, input seed
MD17_SEED = 23
GRAD_NAMES = ("blocks.0.norm_1.mean_shift", "blocks.0.norm_1.affine_weight", "norm.affine_weight", "norm.affine_bias",
              "blocks.0.ga.sep_act.lin.tp.weight", "rbf.mean")
# Three molecules of different sizes.  Per-molecule, per-channel statistics over few atoms condition the model badly: a
# channel that is nearly the same on every atom of a molecule is centred to a small difference, and every upstream rounding
# error grows by |x| / |x - mean|.  The measure used here is the reference's OWN model run in float32 on the CPU against its
# float64 run (worst of energy and the stored gradients).  With 3, 7 and 12 atoms it is 2.5e-6 to 1.2e-4 depending on the
# seed -- no room under the project's 1e-4 model bar, whose matrix steps carry 16-bit activations -- with 5, 9 and 14 atoms
# 3.3e-6 to 6.6e-6, with the sizes and input seeds below 2.0e-6 (graph) and 3.6e-6 (instance).
SIZES = (6, 10, 15)


def grad_names(norm_type):
    return [n for n in GRAD_NAMES if norm_type == "graph" or not n.endswith("mean_shift")]


def qm9_input(seed):
    """three molecules of SIZES atoms in a cube of edge 2.8 A (every pair inside the 5 A cutoff), min distance 0.9 A"""
    from equiformer_amd.synthetic import QM9_P, QM9_Z, _sample_points
    rng = np.random.default_rng(seed)
    pos = np.concatenate([_sample_points(rng, n, 2.8, 0.9) for n in SIZES]).astype(np.float32)
    z = rng.choice(QM9_Z, size=sum(SIZES), p=QM9_P).astype(np.int64)
    return dict(pos=pos, z=z, batch=np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64),
                y=rng.standard_normal(len(SIZES)).astype(np.float32))


def load(tag):
    z = np.load(os.path.join(OUT, tag + ".npz"))
    return ({k[4:]: z[k] for k in z.files if k.startswith("in::")},
            {k[5:]: z[k] for k in z.files if k.startswith("out::")})


def qm9_loss_and_grads(model, ins, norm_type, dtype=torch.float64):
    """(energy, loss, {name: gradient}) of a QM9-shaped model (reference or product) on a fixture's inputs"""
    t = torch.as_tensor
    dev = next(model.parameters()).device
    e = model(f_in=None, pos=t(ins["pos"]).to(dtype).to(dev), batch=t(ins["batch"]).to(dev), node_atom=t(ins["z"]).to(dev))
    loss = (e.squeeze() - t(ins["y"]).to(dtype).to(dev)).abs().mean()
    names = grad_names(norm_type)
    params = dict(model.named_parameters())
    gs = torch.autograd.grad(loss, [params[n] for n in names])
    return e, loss, dict(zip(names, gs))


def reference_outputs(reference=None, shims=None):
    """{tag: (inputs, outputs)} from a fresh run of the reference's model classes"""
    from oracle.refshim import DEFAULT_REFERENCE
    mrg.import_reference(reference or DEFAULT_REFERENCE, shims)
    from nets.graph_attention_transformer import GraphAttentionTransformer as RefQM9
    from nets.graph_attention_transformer_md17 import GraphAttentionTransformerMD17 as RefMD17
    res = {}
    for tag, (norm_type, wseed, iseed) in QM9_CASES.items():
        ins = qm9_input(iseed)
        m = mrg.as_double(fill_deterministic(RefQM9(norm_layer=norm_type, **QM9_KW), wseed))
        e, loss, gs = qm9_loss_and_grads(m, ins, norm_type)
        outs = dict(energy=e.detach().numpy(), loss=np.asarray(loss.item()))
        outs.update({"g::" + n: g.numpy() for n, g in gs.items()})
        res[tag] = (ins, outs)
    ins, _ = mrg.load_fixture("md17_small_l2")
    m = mrg.as_double(fill_deterministic(RefMD17(norm_layer="graph", **MD17_KW), MD17_SEED))
    e, f = m(node_atom=torch.as_tensor(ins["z"]), pos=torch.as_tensor(ins["pos"]).double(), batch=torch.as_tensor(ins["batch"]))
    res["md17_graph"] = (ins, dict(energy=e.detach().numpy(), forces=f.detach().numpy()))
    return res


def table_of(model):
    return dict(params=[[n, list(p.shape)] for n, p in model.named_parameters()], no_weight_decay=sorted(model.no_weight_decay()))


def reference_tables(reference=None, shims=None):
    from oracle.refshim import DEFAULT_REFERENCE
    mrg.import_reference(reference or DEFAULT_REFERENCE, shims)
    from nets.graph_attention_transformer import GraphAttentionTransformer as RefQM9
    from nets.graph_attention_transformer_md17 import GraphAttentionTransformerMD17 as RefMD17
    return {nt: dict(qm9=table_of(RefQM9(norm_layer=nt, **QM9_KW)), md17=table_of(RefMD17(norm_layer=nt, **MD17_KW)))
            for nt in NORM_TYPES}


def load_tables():
    with open(os.path.join(OUT, "param_tables.json")) as fh:
        return json.load(fh)


def check(reference=None, shims=None, log=print):
    """stored fixtures against a fresh reference run: -> {(tag, key): relative difference}"""
    errs = {}
    for tag, (ins, outs) in reference_outputs(reference, shims).items():
        sins, souts = load(tag)
        assert set(sins) == set(ins) and set(souts) == set(outs), tag
        for k in ins:
            assert np.array_equal(sins[k], ins[k]), (tag, k)
        for k in sorted(outs):
            errs[(tag, k)] = mrg.rel(souts[k], outs[k])
            log("  %-14s %-40s fixture vs reference %.3e" % (tag, k, errs[(tag, k)]))
    assert load_tables() == json.loads(json.dumps(reference_tables(reference, shims))), "param_tables.json is stale"
    return errs


def write(reference=None, shims=None):
    os.makedirs(OUT, exist_ok=True)
    for tag, (ins, outs) in reference_outputs(reference, shims).items():
        arrs = {"in::" + k: np.asarray(v) for k, v in ins.items()}
        arrs.update({"out::" + k: np.asarray(v) for k, v in outs.items()})
        path = os.path.join(OUT, tag + ".npz")
        np.savez_compressed(path, **arrs)
        print(tag, "%.0f kB" % (os.path.getsize(path) / 1e3))
    with open(os.path.join(OUT, "param_tables.json"), "w") as fh:
        json.dump(reference_tables(reference, shims), fh, indent=0, sort_keys=True)
        fh.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None, help="checkout of atomicarchitects/equiformer")
    ap.add_argument("--write", action="store_true")
    a = ap.parse_args()
    if a.write:
        write(a.reference)
    worst = max(check(a.reference).values())
    print("worst relative difference vs a fresh reference run: %.3e (tolerance %.0e)" % (worst, mrg.TOL))
    if worst > mrg.TOL:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
