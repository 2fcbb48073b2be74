"""E(3) (parity-aware) models on the FUSED SeparableFCTP kernels: planners keyed on (degree, parity) segments serve every
tensor product of the OC20 l1_256_e3 configuration and of small E(3) force models.  HIP against the fp64 CPU oracle at the
bars of tests/test_gpu_e3.py (energies 1e-4, parameter gradients 2e-4, inversion 1e-5), and against the un-fused path."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import nets as onets

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
sys.path.insert(0, os.path.dirname(__file__))
from weights import fill_deterministic  # noqa: E402

from test_gpu_e3 import _dev, _grad_check, _rel  # noqa: E402

OC20_E3 = dict(irreps_node_embedding="256x0e+64x0o+64x1e+64x1o", irreps_sh="1x0e+1x1o", irreps_head="32x0e+8x0o+8x1e+8x1o",
               irreps_pre_attn="256x0e+64x0o+64x1e+64x1o", irreps_mlp_mid="768x0e+192x0o+192x1e+192x1o")
MD17_E3_32 = dict(irreps_node_embedding="32x0e+32x0o+32x1e+32x1o", num_layers=2, irreps_sh="1x0e+1x1o", fc_neurons=[64, 64],
                  irreps_feature="64x0e", irreps_head="8x0e+8x0o+8x1e+8x1o", num_heads=4, nonlinear_message=True,
                  irreps_mlp_mid="64x0e+32x0o+32x1e+32x1o", alpha_drop=0.0)


class _Count:
    """counts the calls of the fused entry points of equiformer_amd.ops while active"""

    def __enter__(self):
        from equiformer_amd import ops
        self.ops, self.n, self.saved = ops, {"sep_fctp": 0, "sep_fctp_gated": 0}, {}
        for name in self.n:
            fn = getattr(ops, name)
            self.saved[name] = fn

            def wrapped(*a, _fn=fn, _name=name, **k):
                self.n[_name] += 1
                return _fn(*a, **k)
            setattr(ops, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.ops, name, fn)


def test_linear_message_attention_constructs_on_e3_irreps():
    from equiformer_amd.nets.layers import GraphAttention
    irr = OC20_E3["irreps_node_embedding"]
    ga = GraphAttention(irr, "1x0e", "1x0e+1x1o", irr, [64, 64], OC20_E3["irreps_head"], 8, nonlinear_message=False,
                        alpha_drop=0.0, proj_drop=0.0)
    assert ga.lin_sfc_spec.supported and ga.sep.dtp.table.has_odd


def _oc20(num_layers, **kw):
    from equiformer_amd import nets
    ref = fill_deterministic(onets.oc20_l1_256_nonlinear(num_layers=num_layers, **OC20_E3, **kw), 61).double().eval()
    mod = nets.model_entrypoint("oc20_l1_256_e3_nonlinear")(num_layers=num_layers, otf_graph=False, **kw)
    mod.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return ref, mod.to(_dev()).eval()


def _data(pos, batch, Z, tags, ei, off, dev):
    return SimpleNamespace(pos=pos.to(dev), batch=batch.to(dev), atomic_numbers=Z.to(dev), tags=tags.to(dev),
                           edge_index=ei.to(dev), offsets=off.to(dev))


def test_oc20_e3_two_blocks_fused_against_oracle_and_unfused():
    from test_gpu_oc20_heads import _slab
    dev = _dev()
    ref, mod = _oc20(2)
    ga = mod.blocks[0].ga
    assert ga.act_sfc_spec.supported and ga.sep_value.sfc_spec.supported and mod.edge_deg_embed.sfc_spec.supported
    pos, batch, Z, tags, ei, off = _slab(2, 24, seed=7)
    g = torch.Generator().manual_seed(3)
    target = torch.randn(2, generator=g, dtype=torch.float64)
    er = ref(Z, tags, pos.double(), batch, edge_index=ei, offsets=off.double())
    with _Count() as cnt:
        e = mod(_data(pos, batch, Z, tags, ei, off, dev))
    # per block: sep_act (+ alpha) and sep_value (plain or with the gate folded in); the edge-degree embedding
    assert cnt.n["sep_fctp"] + cnt.n["sep_fctp_gated"] == 2 * 2 + 1, cnt.n
    assert _rel(e, er) < 1e-4
    worst = _grad_check(ref, mod, (er.squeeze() - target).abs().mean(), (e.squeeze() - target.float().to(dev)).abs().mean(), 2e-4)
    with torch.no_grad():
        e_inv = mod(_data(-pos, batch, Z, tags, ei, -off, dev))
        assert _rel(e_inv, e) < 1e-5
        mod.set_fused(False)
        with _Count() as cnt0:
            e_unf = mod(_data(pos, batch, Z, tags, ei, off, dev))
        assert cnt0.n == {"sep_fctp": 0, "sep_fctp_gated": 0}
    assert _rel(e, e_unf) < 1e-4
    e_u = mod(_data(pos, batch, Z, tags, ei, off, dev))
    gu = torch.autograd.grad((e_u.squeeze() - target.float().to(dev)).abs().mean(), list(mod.parameters()), allow_unused=True)
    mod.set_fused(True)
    e_f = mod(_data(pos, batch, Z, tags, ei, off, dev))
    gf = torch.autograd.grad((e_f.squeeze() - target.float().to(dev)).abs().mean(), list(mod.parameters()), allow_unused=True)
    scale = max(a.abs().max().item() for a in gu if a is not None)
    worst_u = max((a - b).abs().max().item() / max(b.abs().max().item(), 1e-3 * scale) for a, b in zip(gf, gu) if b is not None)
    print("oc20 e3 fused: energy rel %.2e, inversion %.1e, worst gradient vs oracle %s %.2e, vs un-fused %.2e"
          % (_rel(e, er), _rel(e_inv, e), *worst, worst_u))
    assert worst_u < 2e-4


def test_oc20_e3_four_blocks_energies():
    """an error in 0o / 1e needs three tensor products to reach the energy (tests/test_gpu_e3.py): four blocks, no drop path"""
    from test_gpu_oc20_heads import _slab
    dev = _dev()
    ref, mod = _oc20(4, drop_path_rate=0.0)
    pos, batch, Z, tags, ei, off = _slab(2, 24, seed=8)
    with torch.no_grad():
        er = ref(Z, tags, pos.double(), batch, edge_index=ei, offsets=off.double())
        e = mod(_data(pos, batch, Z, tags, ei, off, dev))
        mod.set_fused(False)
        e_unf = mod(_data(pos, batch, Z, tags, ei, off, dev))
    print("oc20 e3 fused, 4 blocks: energy rel %.2e (un-fused %.2e)" % (_rel(e, er), _rel(e_unf, er)))
    assert _rel(e, er) < 1e-4 and _rel(e, e_unf) < 1e-4


def test_e3_md17_force_loss_through_the_fused_operators():
    """create_graph through the fused kernels: the second-order terms of the multilinear operator are its first-order launches
    with one argument substituted, planned by the same segment-keyed planners"""
    from equiformer_amd.nets.graph_attention_transformer_md17 import GraphAttentionTransformerMD17
    from equiformer_amd.synthetic import md17_aspirin_batch
    dev = _dev()
    kw = dict(irreps_in="64x0e", max_radius=5.0, number_of_basis=32, basis_type="exp", **MD17_E3_32)
    ref = fill_deterministic(onets.GraphAttentionTransformerMD17(**kw), 52).double().train()
    mod = fill_deterministic(GraphAttentionTransformerMD17(**kw), 52).to(dev).train()
    assert mod.blocks[0].ga.act_sfc_spec.supported and mod.blocks[0].ga.sep_value.sfc_spec.supported
    d = md17_aspirin_batch(2, seed=3)
    g = torch.Generator().manual_seed(1)
    a = torch.randn(2, 1, generator=g, dtype=torch.float64)
    B = torch.randn(42, 3, generator=g, dtype=torch.float64)
    Er, Fr = ref(d["z"], d["pos"].double(), d["batch"])
    with _Count() as cnt:
        E, F = mod(d["z"].to(dev), d["pos"].to(dev), d["batch"].to(dev))
    assert cnt.n["sep_fctp"] + cnt.n["sep_fctp_gated"] == 2 * 2 + 1, cnt.n
    assert F.requires_grad and _rel(E, Er) < 1e-4 and _rel(F, Fr) < 1e-4
    worst = _grad_check(ref, mod, (a * Er).sum() + (B * Fr).sum(),
                        (a.float().to(dev) * E).sum() + (B.float().to(dev) * F).sum(), 2e-4)
    print("e3 md17 fused: E rel %.2e, F rel %.2e, worst second-order gradient %s %.2e" % (_rel(E, Er), _rel(F, Fr), *worst))


def test_oc20_e3_linear_message_model_against_oracle():
    """nonlinear_message=False on E(3) irreps: ONE fused operator per block whose 0e weight columns are split into the value part
    (main consumer) and the attention-logit part (second consumer) -- with a 0o segment in the row, the split must count 0e
    channels only.  Energies and all parameter gradients against the oracle, fused against un-fused."""
    from test_gpu_oc20_heads import _slab
    dev = _dev()
    ref, mod = _oc20(2, nonlinear_message=False)
    assert mod.blocks[0].ga.nonlinear_message is False and mod.blocks[0].ga.lin_sfc_spec.supported
    pos, batch, Z, tags, ei, off = _slab(2, 24, seed=9)
    target = torch.randn(2, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    er = ref(Z, tags, pos.double(), batch, edge_index=ei, offsets=off.double())
    with _Count() as cnt:
        e = mod(_data(pos, batch, Z, tags, ei, off, dev))
    assert cnt.n["sep_fctp"] == 2 + 1, cnt.n
    assert _rel(e, er) < 1e-4
    worst = _grad_check(ref, mod, (er.squeeze() - target).abs().mean(), (e.squeeze() - target.float().to(dev)).abs().mean(), 2e-4)
    print("oc20 e3 linear message: energy rel %.2e, worst gradient vs oracle %s %.2e" % (_rel(e, er), *worst))


def test_oc20_e3_captured_step_trains_as_eager():
    """CapturedTrainStep on the 2-block OC20 E(3) model, as tests/test_gpu_periodic_capture.py::
    test_exact_shape_captured_periodic_step_trains_as_eager does for SE(3): three sets of jittered positions that keep (N, E),
    3 eager steps, the capture, 5 replays against 8 eager steps in which the model builds its own graph -- the fused E(3)
    launches (packed weight planes, per-segment pointer arrays built on the host) under graph capture.  Bars of that test; the
    learning rate is the 2e-4 of the OC20 configuration (a 256-wide model: at the 1e-3 of the 64-wide SE(3) test the two
    trajectories, which differ by the summation order of the atomically accumulated weight gradients, end 1.998e-5 apart in the
    loss, on the 2e-5 bar itself)."""
    import periodic_inputs as pi
    from test_gpu_periodic_capture import _assert_trains_as_eager
    from equiformer_amd import nets
    from equiformer_amd.capture import CapturedTrainStep
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW
    dev = _dev()
    base = pi.dense_cells()
    variants = [base["pos"].to(dev)] + [pi.dense_cells(jitter=0.05, jitter_seed=j)["pos"].to(dev) for j in (1, 2)]
    cell, batch = base["cell"].to(dev), base["batch"].to(dev)
    gen = torch.Generator().manual_seed(4)
    z = torch.randint(1, 84, (36,), generator=gen).to(dev)
    tags = torch.randint(0, 3, (36,), generator=gen).to(dev)
    ys = [torch.randn(3, generator=gen).to(dev) for _ in variants]
    results = []
    LR = 2e-4
    for use_graph in (False, True):
        m = nets.model_entrypoint("oc20_l1_256_e3_nonlinear")(num_layers=2, number_of_basis=32, otf_graph=True, use_pbc=True,
                                                              max_neighbors=pi.DENSE_CAP, alpha_drop=0.0, drop_path_rate=0.0)
        m = fill_deterministic(m, 21).to(dev).train()
        assert m.blocks[0].ga.act_sfc_spec.supported and m.blocks[0].ga.sep_act.dtp.table.has_odd
        opt = FlatAdamW(m.parameters(), lr=LR, weight_decay=1e-2)
        pos, y = variants[0].clone(), ys[0].clone()  # the static input tensors
        data = SimpleNamespace(pos=pos, batch=batch, atomic_numbers=z, tags=tags, cell=cell, natoms=torch.tensor([12, 12, 12]))

        def forward_loss(g):
            return (m(data, graph=g, offsets=g.offsets).squeeze(-1) - y).abs().mean()

        def build(into):
            return EdgeGraph.from_radius_pbc(pos, cell, batch, pi.R, pi.DENSE_CAP, num_graphs=3, into=into)[0]
        cs = CapturedTrainStep(opt, forward_loss, min_eager=3)
        losses = []
        with _Count() as cnt:
            for it in range(8):
                pos.copy_(variants[it % 3]), y.copy_(ys[it % 3])
                for gr in opt.param_groups:
                    gr["lr"] = LR * (1.0 + 0.1 * it)
                if use_graph:
                    loss = cs.step(build)
                else:
                    opt.zero_grad(set_to_none=True)
                    loss = (m(data).squeeze(-1) - y).abs().mean()
                    loss.backward()
                    opt.step()
                losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        if use_graph:
            assert cs.replays == 5 and cs.eager_steps == 3 and len(cs._graphs) == 1, (cs.replays, cs.eager_steps)
            assert cnt.n["sep_fctp"] + cnt.n["sep_fctp_gated"] == 4 * 5, cnt.n  # 3 eager steps + the capture, 5 fused calls each
        results.append(dict(losses=losses, p=opt.flat_p.detach().clone(), m=opt.flat_m.detach().clone(), step=opt._step))
    _assert_trains_as_eager(results[0], results[1], 8, LR)
