#!/usr/bin/env python
"""Pin the oracle and the golden fixtures to the REFERENCE'S OWN model code.

    python tests/golden/make_reference_golden.py [--reference /root/reference]            # check (default)
    python tests/golden/make_reference_golden.py [--reference /root/reference] --write    # rewrite the out:: arrays

Imports the reference's `nets` package UNCHANGED (atomicarchitects/equiformer, nets/__init__.py:1-11), builds the same
reduced models as tests/golden/make_golden.py with the same deterministic weights (assigned BY NAME from
tests/golden/weights.py -- parameter names are part of the reference's API; a name present on one
side only is an error), feeds them the inputs stored in the fixtures and compares (or rewrites) the stored outputs in
fp64.  Two ways to satisfy the reference's five un-vendored dependencies:

  * its real environment (e3nn 0.4.4, torch_geometric, torch_scatter, torch_cluster, ocpmodels): nothing to do;
  * this image, where none of them exists: `oracle/refshim` supplies thin stand-ins for the ~25 symbols `nets/` touches
    (each delegating to the restated primitive of oracle/e3.py / oracle/pbc.py) -- the MODEL code that runs is still
    the reference's own source.  That is what `check_all()` does by default and what tests/test_reference_pin.py runs
    on every CPU test pass in the build container (the GPU box has no /root/reference: the test skips there).

The one adaptation needed to run the reference in fp64: its embeddings feed a float32 one-hot into LinearRS
(nets/graph_attention_transformer.py:686-688), which e3nn would reject against float64 weights; a forward pre-hook
casts the input of every LinearRS to the weight dtype.
"""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import make_golden as mg  # noqa: E402  (reduced model configurations)
from weights import fill_deterministic  # noqa: E402

TOL = 1e-9  # fp64 against fp64


def load_fixture(name):
    z = np.load(os.path.join(HERE, name + ".npz"))
    ins = {k[4:]: z[k] for k in z.files if k.startswith("in::")}
    outs = {k[5:]: z[k] for k in z.files if k.startswith("out::")}
    return ins, outs


def import_reference(reference, shims=None):
    """-> the reference's `nets` module.  shims=None: use oracle/refshim only if the real dependencies are absent."""
    if shims is None:
        try:
            import e3nn  # noqa: F401
            import torch_geometric  # noqa: F401
            shims = "refshim" in os.path.abspath(e3nn.__file__)
        except ImportError:
            shims = True
    if shims:
        from oracle.refshim import load_reference_nets
        return load_reference_nets(reference)
    sys.path.insert(0, reference)
    import nets
    return nets


def as_double(ref_model):
    """reference model -> fp64 + the LinearRS input cast described in the header."""
    from nets.tensor_product_rescale import LinearRS
    ref_model = ref_model.double().eval()
    for m in ref_model.modules():
        if isinstance(m, LinearRS) and not hasattr(m, "_cast_hook"):
            m._cast_hook = m.register_forward_pre_hook(lambda mod, a: (a[0].to(mod.tp.weight.dtype),))
    return ref_model


def copy_by_name(src_model, dst_model):
    """Parameters by NAME, both directions checked; e3nn's extra buffers stay as the reference built them."""
    src = dict(src_model.named_parameters())
    dst = dict(dst_model.named_parameters())
    only_dst, only_src = sorted(set(dst) - set(src)), sorted(set(src) - set(dst))
    if only_dst or only_src:
        raise AssertionError("parameter names differ: destination-only %s, source-only %s" % (only_dst, only_src))
    with torch.no_grad():
        for name, p in dst.items():
            assert tuple(p.shape) == tuple(src[name].shape), (name, p.shape, src[name].shape)
            p.copy_(src[name].to(p.dtype))
    sb, db = dict(src_model.named_buffers()), dict(dst_model.named_buffers())
    for name in set(sb) & set(db):  # e.g. ExpNormalSmearing.means / betas: must already agree
        if sb[name].numel():
            assert torch.allclose(sb[name].double(), db[name].double(), rtol=1e-6, atol=0), name


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _oc20_data(ins, cell=7.0):
    """ocpmodels-shaped batch of the OC20 fixtures (cubic cell of make_golden.py): edge_index + integer cell_offsets +
    per-structure neighbour counts, i.e. the otf_graph=False contract of ..._oc20.py:280-293."""
    B = int(ins["batch"].max()) + 1
    ei = torch.as_tensor(ins["edge_index"])
    batch = torch.as_tensor(ins["batch"])
    return SimpleNamespace(pos=torch.as_tensor(ins["pos"]).double(), batch=batch,
                           atomic_numbers=torch.as_tensor(ins["z"]), tags=torch.as_tensor(ins["tags"]), edge_index=ei,
                           cell=(torch.eye(3) * cell)[None].repeat(B, 1, 1).double(),
                           cell_offsets=torch.as_tensor(np.rint(ins["offsets"] / cell)).double(),
                           neighbors=torch.bincount(batch[ei[1]], minlength=B),
                           natoms=torch.bincount(batch, minlength=B))


def reference_outputs(reference="/root/reference", shims=None, log=print, with_reference=True):
    """{fixture tag: {output name: array}} computed by the reference's own model classes, and the same from the oracle
    restatement (oracle/nets.py) with identical weights: -> (ref_outs, oracle_outs).  with_reference=False: the oracle's
    outputs only (ref_outs empty; no reference checkout needed)."""
    RefQM9 = RefMD17 = RefOC20 = RefDP = RefDPMD17 = RefDeNS = None
    if with_reference:
        import_reference(reference, shims)
        from nets.graph_attention_transformer import GraphAttentionTransformer as RefQM9  # [ref: :737-899]
        from nets.graph_attention_transformer_md17 import GraphAttentionTransformerMD17 as RefMD17  # [ref: :127-327]
        from nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20 as RefOC20  # [ref: :85-381]
        from nets.dp_attention_transformer import DotProductAttentionTransformer as RefDP  # [ref: :255-411]
        from nets.dp_attention_transformer_md17 import DotProductAttentionTransformerMD17 as RefDPMD17  # [ref: :57-235]
        from nets.equiformer_md17_dens import Equiformer_MD17_DeNS as RefDeNS  # [ref: :55-354]
    from oracle import nets as onets
    R, O = {}, {}
    t = torch.as_tensor

    def pair(ocls, rcls, seed, okw, rargs=(), rkw=None):
        om = fill_deterministic(ocls(**okw).eval(), seed).double()  # weights rounded to fp32 like make_golden.py
        if rcls is None:
            return om, None
        rm = as_double(rcls(*rargs, **(okw if rkw is None else rkw)))
        copy_by_name(om, rm)
        return om, rm

    def runs(rm, om):
        return [(m, store) for m, store in ((rm, R), (om, O)) if m is not None]

    # ---- QM9-shaped, non-linear and linear messages [ref: GraphAttentionTransformer.forward :864-899]
    for tag, seed, kw, gkeys in (
            ("qm9_small", 11, mg.SMALL_L2, ("g_sep_act_lin", "g_alpha_dot", "g_rad0", "g_rbf_mean")),
            ("qm9_small_linear", 14, dict(mg.SMALL_L2, nonlinear_message=False), ("g_sep_lin", "g_alpha_dot", "g_sep_bias"))):
        ins, _ = load_fixture(tag)
        om, rm = pair(onets.GraphAttentionTransformer, RefQM9, seed,
                      dict(irreps_in="5x0e", max_radius=5.0, number_of_basis=32, **kw))
        for m, store in runs(rm, om):
            e = m(f_in=None, pos=t(ins["pos"]).double(), batch=t(ins["batch"]), node_atom=t(ins["z"]))
            loss = (e.squeeze() - t(ins["y"]).double()).abs().mean()
            if tag == "qm9_small":
                ps = [m.blocks[0].ga.sep_act.lin.tp.weight, m.blocks[1].ga.alpha_dot,
                      m.blocks[0].ga.sep_act.dtp_rad.net[0].weight, m.rbf.mean]
            else:
                ps = [m.blocks[0].ga.sep.lin.tp.weight, m.blocks[1].ga.alpha_dot, m.blocks[0].ga.sep.lin.bias[0]]
            gs = torch.autograd.grad(loss, ps)
            store[tag] = dict(energy=e.detach().numpy(), loss=loss.item(), **{k: g.numpy() for k, g in zip(gkeys, gs)})

    # ---- MD17-shaped: energy and forces [ref: GraphAttentionTransformerMD17.forward :276-327]
    for tag, ocls, rcls, seed, kw in (
            ("md17_small_l2", onets.GraphAttentionTransformerMD17, RefMD17, 12, mg.SMALL_L2),
            ("md17_small_l3", onets.GraphAttentionTransformerMD17, RefMD17, 12, mg.SMALL_L3),
            ("dp_md17_small", onets.DotProductAttentionTransformerMD17, RefDPMD17, 19, mg.SMALL_DP_L2)):
        ins, _ = load_fixture(tag)
        om, rm = pair(ocls, rcls, seed, dict(irreps_in="64x0e", max_radius=5.0, number_of_basis=32, basis_type="exp", **kw))
        for m, store in runs(rm, om):
            e, f = m(node_atom=t(ins["z"]), pos=t(ins["pos"]).double(), batch=t(ins["batch"]))
            store[tag] = dict(energy=e.detach().numpy(), forces=f.detach().numpy())

    # ---- QM9-shaped outputs of the dot-product-attention and E(3) families
    for tag, ocls, rcls, seed, kw in (
            ("dp_qm9_small", onets.DotProductAttentionTransformer, RefDP, 15, mg.SMALL_DP_L2),
            ("e3_qm9_small", onets.GraphAttentionTransformer, RefQM9, 16, mg.SMALL_E3_L2)):
        ins, _ = load_fixture(tag)
        om, rm = pair(ocls, rcls, seed, dict(irreps_in="5x0e", max_radius=5.0, number_of_basis=32, **kw))
        for m, store in runs(rm, om):
            e = m(f_in=None, pos=t(ins["pos"]).double(), batch=t(ins["batch"]), node_atom=t(ins["z"]))
            store[tag] = dict(energy=e.detach().numpy())

    # ---- OC20-shaped [ref: GraphAttentionTransformerOC20.forward :305-381], precomputed periodic edges
    for tag, seed, kw in (("oc20_small", 13, dict(mg.SMALL_OC20, number_of_basis=32)),
                          ("oc20_aux_small", 17, dict(mg.SMALL_OC20, number_of_basis=32, use_auxiliary_task=True,
                                                      irreps_feature="64x0e+32x1e"))):
        ins, _ = load_fixture(tag)
        om, rm = pair(onets.GraphAttentionTransformerOC20, RefOC20, seed, kw, rargs=(None, None, 1),
                      rkw=dict(kw, use_pbc=True, otf_graph=False))
        ro = rm(_oc20_data(ins)) if rm is not None else None
        oo = om(t(ins["z"]), t(ins["tags"]), t(ins["pos"]).double(), t(ins["batch"]), edge_index=t(ins["edge_index"]),
                offsets=t(ins["offsets"]).double())
        for out, store in [(x, st) for x, st in ((ro, R), (oo, O)) if x is not None]:
            out = out if isinstance(out, tuple) else (out,)
            store[tag] = dict(zip(("energy", "aux"), (x.detach().numpy() for x in out)))

    # ---- DeNS [ref: Equiformer_MD17_DeNS.forward :238-354]
    ins, _ = load_fixture("dens_small")
    om, rm = pair(onets.Equiformer_MD17_DeNS, RefDeNS, 18, dict(mg.SMALL_DENS))
    for m, store in runs(rm, om):
        data = SimpleNamespace(z=t(ins["z"]), pos=t(ins["pos"]).double(), batch=t(ins["batch"]),
                               force=t(ins["force"]).double(), noise_mask=t(ins["noise_mask"]))
        e, dy = m(data)
        store["dens_small"] = dict(energy=e.detach().numpy(), dy=dy.detach().numpy())
    return R, O


def check_all(reference="/root/reference", shims=None, write=False, log=print):
    """Compare fixtures and oracle with the reference-executed outputs.  -> {(tag, key): (fixture err, oracle err)}"""
    R, O = reference_outputs(reference, shims, log)
    errs = {}
    for tag, got in R.items():
        ins, outs = load_fixture(tag)
        assert set(outs) == set(got), (tag, sorted(outs), sorted(got))
        for k in sorted(outs):
            errs[(tag, k)] = (rel(outs[k], got[k]), rel(O[tag][k], got[k]))
            log("  %-18s %-14s fixture vs reference %.3e   oracle vs reference %.3e" % ((tag, k) + errs[(tag, k)]))
        if write:
            arrs = {"in::" + k: v for k, v in ins.items()}
            arrs.update({"out::" + k: np.asarray(v) for k, v in got.items()})
            np.savez_compressed(os.path.join(HERE, tag + ".npz"), **arrs)
    missing = sorted(f[:-4] for f in os.listdir(HERE) if f.endswith(".npz") and f[:-4] not in R and f != os.path.basename(PIN))
    assert not missing, "fixtures without a reference run: %s" % missing
    return errs


# ---- reference_pin.npz: what tests/test_reference_pin.py checks the oracle and the product against, recorded from the
# reference's own model code by `--pin` (the tests run without a reference checkout)
PIN = os.path.join(HERE, "reference_pin.npz")
FULL_SIZE = (("graph_attention_transformer_nonlinear_l2", 3_531_715),
             ("graph_attention_transformer_nonlinear_exp_l2_md17", 3_496_001),
             ("graph_attention_transformer_nonlinear_exp_l3_md17", 5_500_865))
OTF_CFG = dict(irreps_node_embedding="256x0e+128x1e", num_layers=2, irreps_sh="1x0e+1x1e", max_radius=5.0, number_of_basis=128,
               fc_neurons=[64, 64], irreps_feature="512x0e", irreps_head="32x0e+16x1e", num_heads=8, nonlinear_message=True,
               irreps_mlp_mid="768x0e+384x1e", alpha_drop=0.0, max_neighbors=500)
AUX_CFG = dict(irreps_node_embedding="32x0e+16x0o+16x1e+16x1o", num_layers=2, irreps_sh="1x0e+1x1o", max_radius=5.0,
               number_of_basis=32, fc_neurons=[64, 64], irreps_feature="64x0e+16x1e+16x1o",
               irreps_head="8x0e+4x0o+4x1e+4x1o", num_heads=4, nonlinear_message=True,
               irreps_mlp_mid="64x0e+16x0o+32x1e+16x1o", alpha_drop=0.0, use_auxiliary_task=True)


def factory_kwargs(name):
    if name == "equiformer_md17_dens":  # takes the constructor's keywords (md17/configs/equiformer_dens/*.yml)
        return dict(irreps_in="64x0e", irreps_equivariant_inputs="1x0e+1x1e+1x2e", max_radius=5.0, number_of_basis=32,
                    basis_type="exp", irreps_feature="512x0e+256x1e+128x2e", alpha_drop=0.0)
    return dict(irreps_in="64x0e" if "md17" in name else "5x0e", radius=5.0, num_basis=32 if "md17" in name else 128)


def param_table(model):
    """["name:d0xd1..."] in registration order"""
    return np.array(["%s:%s" % (n, "x".join(str(d) for d in p.shape)) for n, p in model.named_parameters()])


def param_digest(model):
    """sha256 over the names and the fp32 bytes of every parameter, in registration order (initial values bit for bit)"""
    import hashlib
    h = hashlib.sha256()
    for n, p in model.named_parameters():
        h.update(n.encode())
        h.update(np.ascontiguousarray(p.detach().float().numpy()).tobytes())
    return h.hexdigest()


def full_size_input(name):
    from equiformer_amd.synthetic import md17_aspirin_batch, qm9_like_batch
    return md17_aspirin_batch(1, seed=1) if "md17" in name else qm9_like_batch(2, 12, side=5.5, seed=2)


def run_full_size(model, name):
    d = full_size_input(name)
    if "md17" in name:
        e, f = model(node_atom=d["z"], pos=d["pos"].double(), batch=d["batch"])
        return dict(energy=e.detach().numpy(), forces=f.detach().numpy())
    return dict(energy=model(f_in=None, pos=d["pos"].double(), batch=d["batch"], node_atom=d["z"]).detach().numpy())


def otf_input():
    """two periodic structures (10 atoms each, triclinic cells) for the on-the-fly graph case"""
    rng = np.random.default_rng(3)
    n, B = 10, 2
    cell = torch.tensor([[[6.0, 0, 0], [1.0, 6.5, 0], [0, 0, 12.0]], [[7.0, 0, 0], [0, 6.0, 0], [0.5, 0, 11.0]]]).double()
    pos = torch.tensor(rng.uniform(0, 6.0, size=(B * n, 3))).double()
    return SimpleNamespace(pos=pos, batch=torch.arange(B).repeat_interleave(n), atomic_numbers=torch.tensor(rng.integers(1, 84, B * n)),
                           tags=torch.tensor(rng.integers(0, 3, B * n)), cell=cell, natoms=torch.tensor([n] * B))


def otf_oracle():
    """the oracle's OC20 model of the on-the-fly case, weights filled by name (tests/golden/weights.py), fp32 values"""
    from oracle import nets as onets
    return fill_deterministic(onets.GraphAttentionTransformerOC20(**{k: v for k, v in OTF_CFG.items() if k != "max_neighbors"}), 5)


def aux_oracle():
    """the oracle's OC20 model with the E(3) auxiliary head, weights filled by name, fp32 values"""
    from oracle import nets as onets
    return fill_deterministic(onets.GraphAttentionTransformerOC20(**AUX_CFG), 1)


def write_pin(reference="/root/reference", shims=None, log=print):
    """Run the reference's own model code and record, in PIN: the outputs behind every golden fixture, every registered
    factory's parameter table / initial-value digest / no-weight-decay set, and the outputs of the full-width and OC20 cases."""
    R, _ = reference_outputs(reference, shims, log)
    rnets = sys.modules["nets"]
    arrs = {}
    for tag, outs in R.items():
        for k, v in outs.items():
            arrs["out::%s::%s" % (tag, k)] = np.asarray(v)
    rreg = sys.modules["nets.registry"]  # (`nets.registry` the ATTRIBUTE is ocpmodels' registry object after the star-imports)
    names = sorted(rreg._model_entrypoints)
    arrs["reg::names"] = np.array(names)
    for name in names:
        torch.manual_seed(7)
        r = rnets.model_entrypoint(name)(**factory_kwargs(name))
        arrs["reg::%s::params" % name] = param_table(r)
        arrs["reg::%s::digest" % name] = np.array(param_digest(r))
        arrs["reg::%s::no_wd" % name] = np.array(sorted(r.no_weight_decay()))
        log("  registry %s: %d parameters" % (name, len(arrs["reg::%s::params" % name])))
    for name, count in FULL_SIZE:
        torch.manual_seed(3)
        r = rnets.model_entrypoint(name)(**factory_kwargs(name))
        arrs["full::%s::count" % name] = np.array(sum(p.numel() for p in r.parameters()))
        arrs["full::%s::digest" % name] = np.array(param_digest(r))
        for k, v in run_full_size(as_double(r), name).items():
            arrs["full::%s::%s" % (name, k)] = v
    from nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20 as RefOC20
    r = RefOC20(None, None, 1, use_pbc=True, otf_graph=True, **OTF_CFG)
    copy_by_name(otf_oracle(), r)  # the oracle's deterministic weights (the product draws this model's init in another order)
    data = otf_input()
    arrs["otf::energy"] = as_double(r)(data).detach().numpy()
    for k in ("edge_index", "cell_offsets", "neighbors"):  # the periodic graph the reference's own search produced
        arrs["otf::" + k] = getattr(data, k).numpy()
    r = RefOC20(None, None, 1, use_pbc=True, otf_graph=False, **AUX_CFG)
    arrs["aux::params"] = param_table(r)
    copy_by_name(aux_oracle(), r)
    ins, _ = load_fixture("oc20_aux_small")
    e, a = as_double(r)(_oc20_data(ins))
    arrs["aux::energy"], arrs["aux::aux"] = e.detach().numpy(), a.detach().numpy()
    np.savez_compressed(PIN, **arrs)
    log("wrote %s (%d arrays)" % (PIN, len(arrs)))


def load_pin():
    z = np.load(PIN)
    return {k: z[k] for k in z.files}


def check_pinned(log=print):
    """check_all() against the reference outputs recorded in PIN: -> {(tag, key): (fixture err, oracle err)}"""
    pin = load_pin()
    _, O = reference_outputs(log=log, with_reference=False)
    errs = {}
    for key in sorted(k for k in pin if k.startswith("out::")):
        _, tag, k = key.split("::")
        _, outs = load_fixture(tag)
        errs[(tag, k)] = (rel(outs[k], pin[key]), rel(O[tag][k], pin[key]))
        log("  %-18s %-14s fixture vs reference %.3e   oracle vs reference %.3e" % ((tag, k) + errs[(tag, k)]))
    for tag, outs in O.items():
        _, fouts = load_fixture(tag)
        assert set(fouts) == set(outs) == {k for t, k in errs if t == tag}, (tag, sorted(fouts), sorted(outs))
    missing = sorted(f[:-4] for f in os.listdir(HERE) if f.endswith(".npz") and f[:-4] not in O and f != os.path.basename(PIN))
    assert not missing, "fixtures without a reference run: %s" % missing
    return errs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference", help="checkout of atomicarchitects/equiformer")
    ap.add_argument("--write", action="store_true", help="overwrite the out:: arrays with the reference's outputs")
    ap.add_argument("--real-deps", action="store_true", help="never use oracle/refshim (the real environment is installed)")
    ap.add_argument("--pin", action="store_true", help="record the reference's outputs, parameter tables and initial-value "
                    "digests in reference_pin.npz (what tests/test_reference_pin.py checks)")
    a = ap.parse_args()
    if a.pin:
        write_pin(a.reference, shims=False if a.real_deps else None)
        return
    errs = check_all(a.reference, shims=False if a.real_deps else None, write=a.write)
    worst = max(max(v) for v in errs.values())
    print("worst relative difference vs the reference's own model code: %.3e (tolerance %.0e)" % (worst, TOL))
    if not a.write and worst > TOL:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
