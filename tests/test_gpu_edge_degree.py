"""The collapsed edge-degree embedding (csrc/edgedeg.hip, ops.edgedeg_fold / edgedeg_scatter) on the GPU.

Operator level: kernels and Functions against the fp64 restatement of the WHOLE operator (tests/fp64_edge_degree.py `full`,
pinned to the oracle by tests/test_edge_degree_identity.py) for the QM9, MD17 L3 and OC20 irreps, on graphs with one edge,
ragged segments, nodes without incoming edges and a 130-edge segment, in every matrix mode, with the per-mode relative
max-norm bounds of tests/test_gpu_sfcx.py (fp32 held to the split6 bound).  The same inputs also go through the fused
SeparableFCTP (`use_collapsed = False`) and both errors are printed side by side.
Model level: collapsed against not and against the fp64 oracle, a captured train step, OC20, and MD17 staying fused.
Wall time of this file on an MI355X, one run each (pytest's figure): 6.5 s at the parent commit, 7.4 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py).
"""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

import fp64_edge_degree as ref
from oracle import e3 as oe3
from poison import poisoned_ops  # noqa: E402,F401  (the fixture of the tests that run on poisoned, guarded allocations)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"split": 1e-4, "bf16": 3e-2, "split6": 5e-6, "fp32": 5e-6}  # tests/test_gpu_sfcx.py TOL; fp32 at the split6 bound
IRREPS = {"qm9": ("128x0e+64x1e+32x2e", 2), "md17_l3": ("128x0e+64x1e+64x2e+32x3e", 3), "oc20": ("256x0e+128x1e", 1)}
NB = 32
AVG = 15.57930850982666


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _edges(kind, g):
    """(N, src, dst) of the test graphs"""
    if kind == "one":
        return 1, torch.zeros(1, dtype=torch.long), torch.zeros(1, dtype=torch.long)
    if kind == "small":
        N, E = 5, 37
        return N, torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)
    if kind == "blocks":
        N, E = 70, 1000
        return N, torch.randint(0, N, (E,), generator=g), torch.randint(0, N, (E,), generator=g)
    if kind == "isolated":  # nodes 0, 3, 4, 8 and the last two have no incoming edge
        N, E = 12, 30
        allowed = torch.tensor([1, 2, 5, 6, 7, 9])
        return N, torch.randint(0, N, (E,), generator=g), allowed[torch.randint(0, 6, (E,), generator=g)]
    if kind == "long":  # node 1: 130 incoming edges (more than two passes of a 64-wide wave)
        N = 4
        dst = torch.cat([torch.full((130,), 1), torch.tensor([0, 0, 3, 3, 3, 2, 2])]).long()
        return N, torch.randint(0, N, (dst.numel(),), generator=g), dst
    raise ValueError(kind)


def _sh_irreps(lmax):
    return "+".join("1x%de" % l for l in range(lmax + 1))


def _setup(name, kind, seed=3):
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.nets.layers import EdgeDegreeEmbeddingNetwork
    dev = _dev()
    irreps, lmax = IRREPS[name]
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    m = EdgeDegreeEmbeddingNetwork(irreps, _sh_irreps(lmax), [NB, 64, 64], AVG)
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if "bias" in n_ or n_ == "rad.offset":
                p.copy_(torch.randn(p.shape, generator=g) * 0.5)
    m = m.to(dev)
    N, src, dst = _edges(kind, g)
    E = dst.numel()
    sh64 = oe3.spherical_harmonics(lmax, torch.randn(E, 3, generator=g, dtype=torch.float64))
    es = torch.randn(E, NB, generator=g)
    graph, order = EdgeGraph.from_edges(src.to(dev), dst.to(dev), N)
    sh = sh64.float().to(dev)[order].contiguous()
    es = es.to(dev)[order].contiguous()
    gout = torch.randn(N, m.D, generator=g).to(dev)
    return m, graph, sh, es, gout


def _fp64(m, graph, sh, es, gout, h=None):
    """fp64 restatement of the whole operator on the GPU's own inputs: output and every gradient"""
    P = ref.params_of(m)
    M = ref.coupling(m.dw.table, sh.double())
    h64 = None if h is None else h.detach().double().requires_grad_(True)
    out = ref.full(P, m.dw.table, m.proj.spec.pairs, m.D, M, es.double(), graph.dst.long(), graph.N, AVG, h=h64)
    leaves = list(P.values()) + ([h64] if h64 is not None else [])
    grads = torch.autograd.grad((out * gout.double()).sum(), leaves, allow_unused=True)
    g = dict(zip(P, grads[:len(P)]))
    return out.detach(), g, (grads[-1] if h64 is not None else None)


def _module_run(m, graph, sh, es, gout, collapsed):
    from equiformer_amd.nets.layers import EdgeContext
    m.use_collapsed = collapsed
    m.zero_grad(set_to_none=True)
    ectx = EdgeContext(graph, sh, es, hidden_only=[m.rad] if m.collapses(sh) else [])
    out = m(gout, ectx)
    (out * gout).sum().backward()
    return out.detach(), {k: (None if p.grad is None else p.grad.clone()) for k, p in m.named_parameters()}


@pytest.mark.usefixtures("poisoned_ops")
@pytest.mark.parametrize("kind", ["one", "small", "blocks", "isolated", "long"])
@pytest.mark.parametrize("name", sorted(IRREPS))
def test_operator_against_fp64(name, kind):
    from equiformer_amd import ops
    m, graph, sh, es, gout = _setup(name, kind)
    spec = m.collapsed_spec
    assert spec.supported and m.collapses(sh)
    r_out, r_g, _ = _fp64(m, graph, sh, es, gout)
    with torch.no_grad():
        h = m.rad(es, hidden_only=True)
    h_out, h_g, h_dh = _fp64(m, graph, sh, es, gout, h=h)
    for mode in ("split", "bf16", "split6", "fp32"):
        with ops.matrix_mode(mode):
            # the Functions on their own, the hidden activation a leaf: its gradient is checked too
            hl = h.clone().requires_grad_(True)
            M = ops.dtp_coupling(sh, m.dw.table)
            At, a = ops.edgedeg_fold(m.rad.net[-1].weight, m.rad.offset, m.exp.tp.weight, m.exp._bias(), m.proj.tp.weight, spec)
            out = ops.edgedeg_scatter(ops.dense_linear(hl, At, a), M, m.proj._bias(), graph, spec, AVG ** -0.5)
            names = ["rad.net.6.weight", "rad.offset", "exp.tp.weight", "exp.bias.0", "proj.tp.weight", "proj.bias.0"]
            leaves = [dict(m.named_parameters())[n] for n in names]
            grads = torch.autograd.grad((out * gout).sum(), leaves + [hl])
            errs = {"out": _rel(out, h_out), "dh": _rel(grads[-1], h_dh)}
            for n, gr in zip(names, grads):
                errs[n] = _rel(gr, h_g[n])
                assert bool((gr[h_g[n] == 0.0] == 0.0).all()), (mode, n)  # the rows no l1 = 0 path reads: exact zeros
            print("%s %s %s functions: %s" % (name, kind, mode, {k: "%.1e" % v for k, v in errs.items()}))
            assert max(errs.values()) < TOL[mode], (mode, errs)
            # the module, both paths, against the fp64 operator with the radial MLP included
            both = {}
            for collapsed in (True, False):
                o, g_ = _module_run(m, graph, sh, es, gout, collapsed)
                e = {"out": _rel(o, r_out)}
                for n in r_g:
                    assert g_[n] is not None, (mode, collapsed, n)  # every parameter has a .grad
                    e[n] = _rel(g_[n], r_g[n])
                both[collapsed] = e
                if collapsed:
                    o2, _ = _module_run(m, graph, sh, es, gout, True)
                    assert torch.equal(o, o2)  # no atomics: bit-reproducible
                    for n in r_g:
                        assert bool((g_[n][r_g[n] == 0.0] == 0.0).all()), (mode, n)
            print("%s %s %s module, collapsed | fused: %s" % (name, kind, mode, {
                k: "%.1e | %.1e" % (both[True][k], both[False][k]) for k in both[True]}))
            assert max(both[True].values()) < TOL[mode], (mode, both[True])
    m.use_collapsed = True


@pytest.mark.usefixtures("poisoned_ops")
def test_argument_errors_and_refusals():
    from equiformer_amd import lib, ops
    m, graph, sh, es, gout = _setup("qm9", "small")
    spec = m.collapsed_spec
    z = torch.zeros(graph.E, spec.Z, device=sh.device)
    bad = lib.EqfEdgeDeg()
    with pytest.raises(lib.HipLibraryError):
        lib.call("eqf_edgedeg_scatter_fwd", ops._p(z), ops._p(z), ops._p(graph.row_ptr), None, bad, 1.0, ops._p(z), graph.N,
                 graph.E, ops._stream())
    with pytest.raises(lib.HipLibraryError):
        lib.call("eqf_edgedeg_fold_fwd", None, None, None, None, None, spec.c_ref, None, None, ops._stream())
    # a coupling that needs a gradient (force training) is refused, and the module does not collapse then
    shg = sh.clone().requires_grad_(True)
    assert not m.collapses(shg)
    with pytest.raises(ops.HipOnlyError):
        ops.edgedeg_scatter(z, ops.dtp_coupling(shg, m.dw.table), m.proj._bias(), graph, spec, 1.0)


def test_radial_bank_leaves_the_hidden_only_module_out():
    """The other modules' outputs are bit-equal to the run with every last layer banked; the hidden activation handed out is
    the one of the module on its own; gradients agree (the weight gradients are atomically accumulated: 2e-5)."""
    from equiformer_amd.nets.layers import RadialBank, RadialProfile
    dev = _dev()
    torch.manual_seed(5)
    mods = [RadialProfile([NB, 64, 64, n]).to(dev) for n in (960, 96, 64, 480)]
    es = torch.randn(333, NB, device=dev)
    bank = RadialBank(mods)
    assert bank.ok and bank.LAST_BANKED
    cots = [torch.randn(333, n, device=dev) for n in (960, 64, 64, 480)]  # (module 1: a cotangent for its hidden activation)

    def run(hidden_only):
        for mm in mods:
            mm.zero_grad(set_to_none=True)
        outs = bank.forward(es, hidden_only)
        vals = [outs[id(mm)] for mm in mods]
        if not hidden_only:
            vals[1] = mods[1](es, hidden_only=True)  # unbanked hidden activation
        sum((v * c).sum() for v, c in zip(vals, cots)).backward()
        return [v.detach() for v in vals], {(i, n): p.grad.clone() for i, mm in enumerate(mods)
                                            for n, p in mm.named_parameters() if p.grad is not None}

    full, g_full = run(())
    part, g_part = run([mods[1]])
    for k in (0, 2, 3):
        assert torch.equal(part[k], full[k]), k
    assert part[1].shape == (333, 64)
    assert torch.equal(part[1], full[1]), _rel(part[1], full[1])
    # (module 1's last layer and offset: no gradient when it is hidden-only, a zero one when its unused output was banked)
    assert set(g_full) - set(g_part) == {(1, "net.6.weight"), (1, "offset")} and set(g_part) <= set(g_full)
    for k in g_part:
        assert _rel(g_part[k], g_full[k]) < 2e-5, k


def _qm9_models():
    from equiformer_amd import nets
    from oracle import nets as onets
    torch.manual_seed(0)
    o = onets.graph_attention_transformer_nonlinear_l2("5x0e", 5.0).eval()
    mod = nets.model_entrypoint("graph_attention_transformer_nonlinear_l2")(irreps_in="5x0e", radius=5.0)
    mod.load_state_dict(o.state_dict())
    return o.double(), mod.to(_dev()).eval()


def _count_collapsed(monkeypatch):
    from equiformer_amd import ops
    calls = []
    real = ops.edgedeg_scatter
    monkeypatch.setattr(ops, "edgedeg_scatter", lambda *a: (calls.append(1), real(*a))[1])
    return calls


def test_qm9_model_collapsed_against_fused_and_fp64_oracle(monkeypatch):
    from equiformer_amd.synthetic import qm9_like_batch
    dev = _dev()
    o, mod = _qm9_models()
    d = qm9_like_batch(4, 18, side=6.5, seed=1)
    yr = o(None, d["pos"].double(), d["batch"], d["z"])
    (yr.squeeze() - d["y"].double()).abs().mean().backward()
    calls = _count_collapsed(monkeypatch)
    res = {}
    for collapsed in (True, False):
        mod.edge_deg_embed.use_collapsed = collapsed
        mod.zero_grad(set_to_none=True)
        n0 = len(calls)
        y = mod(None, d["pos"].to(dev), d["batch"].to(dev), d["z"].to(dev))
        (y.squeeze() - d["y"].to(dev)).abs().mean().backward()
        assert (len(calls) - n0 == 1) == collapsed
        assert all(p.grad is not None for p in mod.parameters())
        res[collapsed] = (y.detach().cpu(), {n: p.grad.cpu().clone() for n, p in mod.named_parameters()})
    errs = {}
    for collapsed, (y, g) in res.items():
        e = _rel(y, yr)
        ge = max((_rel(g[n], q.grad), n) for n, q in o.named_parameters() if q.grad is not None and q.grad.abs().max() > 0)
        print("collapsed" if collapsed else "fused", "worst parameter gradient: %.2e %s" % ge)
        errs[collapsed] = (e, ge[0])
    ab_e = _rel(res[True][0], res[False][0])
    ab_g = max(_rel(res[True][1][n], res[False][1][n]) for n in res[True][1] if res[False][1][n].abs().max() > 0)
    print("QM9 model, 4 molecules, vs fp64 oracle (energy, worst parameter gradient): collapsed %.2e %.2e | fused %.2e %.2e; "
          "collapsed vs fused %.2e %.2e" % (errs[True] + errs[False] + (ab_e, ab_g)))
    assert errs[True][0] < 1e-4 and errs[True][1] < 1e-4  # the bound of tests/test_gpu_fullsize.py
    assert ab_e < 1e-4 and ab_g < 1e-4
    # the rows of the embedding no l1 = 0 path reads: exact zeros, as in the oracle
    for n in ("edge_deg_embed.rad.net.6.weight", "edge_deg_embed.rad.offset", "edge_deg_embed.proj.tp.weight"):
        zero = dict(o.named_parameters())[n].grad == 0.0
        assert int(zero.sum()) > 0 and bool((res[True][1][n][zero] == 0.0).all()), n
    mod.edge_deg_embed.use_collapsed = True


def test_captured_train_step_with_the_collapsed_embedding(monkeypatch):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.capture import CapturedTrainStep
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    from equiformer_amd.optim import FlatAdamW
    from equiformer_amd.synthetic import qm9_like_batch
    dev = _dev()
    m = GraphAttentionTransformer(irreps_in="5x0e", max_radius=5.0, number_of_basis=32, **dict(mg.SMALL_L2, alpha_drop=0.0))
    m = fill_deterministic(m, 21).to(dev).train()
    assert m.edge_deg_embed.use_collapsed and m.edge_deg_embed.collapsed_spec.supported
    d = {k: v.to(dev) for k, v in qm9_like_batch(6, 12, side=5.5, seed=9).items()}
    opt = FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)
    for gr in opt.param_groups:  # (the weights stay: every step computes the same loss)
        gr["lr"], gr["weight_decay"] = 0.0, 0.0
    calls = _count_collapsed(monkeypatch)

    def forward_loss(g):
        return (m(None, d["pos"], d["batch"], d["z"], graph=g).squeeze() - d["y"]).abs().mean()

    def build(into):
        return EdgeGraph.from_radius(d["pos"], d["batch"], 5.0, num_graphs=6, into=into)
    cs = CapturedTrainStep(opt, forward_loss, min_eager=2)
    losses = [float(cs.step(build)) for _ in range(5)]
    assert cs.replays == 3 and len(calls) >= 3  # two eager steps and the capture ran the collapsed operator
    for v in losses[2:]:
        assert abs(v - losses[0]) <= 1e-6 * abs(losses[0]), losses


def test_oc20_forward_collapsed_against_fused(monkeypatch):
    from test_gpu_oc20_heads import _slab
    from equiformer_amd import nets
    dev = _dev()
    torch.manual_seed(0)
    mod = nets.model_entrypoint("oc20_l1_256_nonlinear")(otf_graph=False).to(dev).eval()
    pos, batch, Z, tags, ei, off = _slab(2, 24, seed=7)
    data = SimpleNamespace(pos=pos.to(dev), batch=batch.to(dev), atomic_numbers=Z.to(dev), tags=tags.to(dev),
                           edge_index=ei.to(dev), offsets=off.to(dev))
    calls = _count_collapsed(monkeypatch)
    es = {}
    with torch.no_grad():
        for collapsed in (True, False):
            mod.edge_deg_embed.use_collapsed = collapsed
            n0 = len(calls)
            es[collapsed] = mod(data)
            assert (len(calls) - n0 == 1) == collapsed
    print("oc20_l1_256_nonlinear, 2 structures: energy collapsed vs fused %.2e" % _rel(es[True], es[False]))
    assert _rel(es[True], es[False]) < 1e-4


def test_md17_keeps_the_fused_operator(monkeypatch):
    """forces differentiate through the spherical harmonics: the coupling needs a gradient, also at second order"""
    from equiformer_amd.nets.graph_attention_transformer_md17 import _md17
    from equiformer_amd.synthetic import md17_aspirin_batch
    dev = _dev()
    torch.manual_seed(0)
    mod = _md17("64x0e", 5.0, 32, None, None, None, num_layers=1).to(dev).train()
    assert mod.edge_deg_embed.use_collapsed and mod.edge_deg_embed.collapsed_spec.supported
    d = md17_aspirin_batch(1, seed=1)
    calls = _count_collapsed(monkeypatch)
    E, F = mod(d["z"].to(dev), d["pos"].to(dev), d["batch"].to(dev))
    (E.sum() + (F * F).sum()).backward()
    assert len(calls) == 0
    assert all(p.grad is not None for p in mod.edge_deg_embed.parameters())
