"""Equivariant dropout drawn on the device (equiformer_amd/dropout.py, csrc/dropout.hip eqf_irreps_dropout) on the GPU:

1. the operator, both modes, is bit-equal to x * `keep_mask` expanded to the row layout -- forward, gradient, create_graph second
   derivative -- at ragged shapes; the seed may be split between the by-value argument and the device word;
2. models in training mode under `device_draws` against the fp64 oracle, whose dropout is emulated by hooks that multiply by
   `keep_mask` in e3nn's order (the oracle ignores out_drop and builds its blocks with proj_drop 0);
3. the padded view of a batch drops on its real rows what the unpadded batch drops;
4. the captured IS2RS step trains as the eager loop under `device_draws(step_seed(s, k))`, with another mask per replay, and so
   does a BucketedTrainStep on molecules with proj_drop;
5. the default seed is one draw from the CPU generator.
Bounds: those of tests/test_gpu_droppath.py (outputs 1e-4, probed gradient 2e-4), of test_md17_force_loss_second_order_gradients
(1e-4 on every parameter) and of tests/test_gpu_is2rs_step.py / tests/test_gpu_bucketed_capture.py (losses 2e-5 max(1, |loss|),
moments 5e-4, parameters above noise 1e-4), unchanged.
Wall time of this file on an MI355X, one run each (pytest's figure): 7.7 s at the parent commit, 7.2 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py)."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import periodic_inputs as pi  # noqa: E402
from poison import poisoned_ops  # noqa: E402,F401  (the fixture of the tests that run on poisoned, guarded allocations)
import test_gpu_bucketed_capture as tb  # noqa: E402  (the QM9 batches, losses and trajectory bounds)
import test_gpu_droppath as td  # noqa: E402  (the 8-step slab protocol)
import test_gpu_is2rs_step as t6  # noqa: E402  (the slab batch, the loss normalisation and the trajectory bounds)
import test_gpu_oc20_heads as th  # noqa: E402  (the explicit-edge slabs)

DEV = torch.device("cuda:0")
P = 0.4
R = pi.R


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- 1. operator
# rows x irreps: fewer quads than lanes; one row of one quad; more quads per row than a wavefront has lanes (65 + 1 + 2); seven
# components; odd-parity segments (a 0o segment is no scalar); more rows than one launch has wavefronts (2 048 workgroups x 4)
SHAPES = {"37x(8x0e+4x1e)": (37, "8x0e+4x1e"), "1x(4x0e)": (1, "4x0e"), "9x(260x0e+4x1e+8x2e)": (9, "260x0e+4x1e+8x2e"),
          "5x(4x0e+4x3e)": (5, "4x0e+4x3e"), "37x(8x0e+4x0o+4x1e+4x1o)": (37, "8x0e+4x0o+4x1e+4x1o"), "8229x(4x0e)": (8229, "4x0e")}


@pytest.mark.usefixtures("poisoned_ops")
@pytest.mark.parametrize("scalars_only", [False, True])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_operator_is_the_product_with_keep_mask_at_every_order(shape, scalars_only):
    from equiformer_amd import dropout
    from equiformer_amd.layout import RowLayout
    rows, irreps = SHAPES[shape]
    lay = RowLayout(irreps)
    seed, call = 7, 2  # keep_mask(7, 2, ., ., 0.4)[0] starts 0, 0, 1, 1: entry (0, 0) is dropped
    mask = dropout.keep_mask(seed, call, rows, irreps, P, scalars_only, expand="cf")
    dropped = mask == 0
    assert mask.shape == (rows, lay.dim) and bool(dropped[0, 0]) and bool(dropped.any()) and bool((mask > 1).any())
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, lay.dim, generator=g)
    x[0, 0] = float("nan")  # a NaN in a dropped entry stays a NaN: a multiply, not a select
    x = x.to(DEV).requires_grad_(True)
    dy = torch.randn(rows, lay.dim, generator=g).to(DEV).requires_grad_(True)
    w = torch.randn(rows, lay.dim, generator=g).to(DEV)
    md = mask.to(DEV)
    y = dropout.irreps_dropout(x, lay, P, seed, call, scalars_only=scalars_only)
    assert torch.isnan(y[0, 0]) and torch.equal(_bits(y), _bits(x.detach() * md))
    flat = y.detach().flatten()[1:]
    assert bool((flat[dropped.flatten()[1:].to(DEV)] == 0).all())  # (+-0: the product with the factor 0)
    if scalars_only:  # everything but the 0e segments passes bit for bit
        first = lay.segs[0][0]
        assert (lay.segs[0][1], lay.par[0]) == (0, 1) and bool((mask[:, first:] == 1).all())
        assert torch.equal(_bits(y[:, first:]), _bits(x[:, first:]))
    (dx,) = torch.autograd.grad(y, x, dy, create_graph=True)
    assert torch.equal(_bits(dx), _bits(dy.detach() * md))
    (ddy,) = torch.autograd.grad((dx * w).sum(), dy)
    assert torch.equal(_bits(ddy), _bits(w * md))
    # plain first-order backward as well
    x3 = x.detach().clone().requires_grad_(True)
    dropout.irreps_dropout(x3, irreps, P, seed, call, scalars_only=scalars_only).backward(dy.detach())
    assert torch.equal(_bits(x3.grad), _bits(dx))
    # another call index: another mask
    m3 = dropout.keep_mask(seed, 3, rows, irreps, P, scalars_only, expand="cf")
    assert not torch.equal(m3, mask)
    x0 = torch.nan_to_num(x.detach())
    assert torch.equal(_bits(dropout.irreps_dropout(x0, lay, P, seed, 3, scalars_only=scalars_only)), _bits(x0 * m3.to(DEV)))


@pytest.mark.usefixtures("poisoned_ops")
def test_operator_edges_row_count_no_rows_refused_width_and_split_seed():
    from equiformer_amd import dropout, lib, ops
    irreps = "8x0e+4x1e"
    x = torch.randn(37, 20, generator=torch.Generator().manual_seed(1)).to(DEV)

    def mask(seed, call=1, rows=37):
        return dropout.keep_mask(seed, call, rows, irreps, P, expand="cf").to(DEV)

    # the factor of a row does not depend on the number of rows
    assert torch.equal(dropout.irreps_dropout(x[:20].contiguous(), irreps, P, 7, 1), dropout.irreps_dropout(x, irreps, P, 7, 1)[:20])
    # rows = 0: nothing launched, an empty result with a gradient
    x0 = torch.zeros(0, 20, device=DEV, requires_grad=True)
    y0 = dropout.irreps_dropout(x0, irreps, P, 7, 0)
    assert y0.shape == (0, 20)
    y0.sum().backward()
    assert x0.grad.shape == (0, 20)
    # a multiplicity of 6: refused by status before any launch, the output buffer untouched
    x6 = torch.randn(37, 6, device=DEV)
    out = torch.full((37, 6), 3.5, device=DEV)
    six = lib.make_irreps([(6, 0)])
    import ctypes
    with pytest.raises(lib.HipLibraryError):
        lib.call("eqf_irreps_dropout", ops._p(x6), ops._p(out), 37, ctypes.byref(six), 0, P, 1.0 / (1.0 - P), 7, None, 0, ops._stream())
    with pytest.raises(lib.HipLibraryError):
        dropout.irreps_dropout(x6, "6x0e", P, 7, 0)
    torch.cuda.synchronize()
    assert bool((out == 3.5).all())
    # one total seed, by value or split between the by-value part and the device word (mod 2^64, the word read as unsigned)
    total = 2 ** 63 + 12345  # (beyond int64's positive range)

    def word(v):
        v &= (1 << 64) - 1
        return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v], dtype=torch.int64, device=DEV)

    want = dropout.irreps_dropout(x, irreps, P, total, 1)
    assert torch.equal(want, x * mask(total))
    splits = [(0, total), (total - 99, 99), (5, total - 5), ((1 << 64) - 3, total + 3), (total + 10, (1 << 64) - 10)]
    for by_value, w in splits:
        assert (by_value + w) % (1 << 64) == total
        got = dropout.irreps_dropout(x, irreps, P, by_value, 1, seed_word=word(w))
        assert torch.equal(got, want), (by_value, w)
    assert any(by_value + w >= (1 << 64) for by_value, w in splits), "no split wraps"
    assert not torch.equal(dropout.irreps_dropout(x, irreps, P, total + 1, 1), want)
    # the word is read when the kernel runs: rewriting it changes the next launch, the backward of an earlier forward follows it
    wd = word(total)
    xr = x.clone().requires_grad_(True)
    y = dropout.irreps_dropout(xr, irreps, P, 0, 1, seed_word=wd)
    assert torch.equal(y, want)
    (dx,) = torch.autograd.grad(y, xr, torch.ones_like(y), retain_graph=True)
    assert torch.equal(dx, mask(total))
    wd.copy_(word(total + 1))
    assert torch.equal(dropout.irreps_dropout(x, irreps, P, 0, 1, seed_word=wd), x * mask(total + 1))
    (dx1,) = torch.autograd.grad(y, xr, torch.ones_like(y))
    assert torch.equal(dx1, mask(total + 1)) and not torch.equal(dx1, dx)
    with pytest.raises(ops.HipOnlyError):
        dropout.irreps_dropout(x, irreps, P, 0, 1, seed_word=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ops.HipOnlyError):
        dropout.irreps_dropout(x, irreps, P, 0, 1, seed_word=torch.zeros(1, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------------------------------------------------------- 2. models
class _OracleDropout:
    """Dropout on the fp64 oracle by hooks: forward hooks on the blocks' attention and feed-forward modules (proj_drop), counting
    the calls in execution order, and forward pre-hooks on the head -- and on the skip connection beside an attention head, which
    reads the same dropped features -- for out_drop, which takes the next call once per forward.  The factors are `keep_mask`
    expanded to e3nn's [mul][2l+1] order; every mask used is kept for the test to look at."""

    def __init__(self, ref, mod, seed, head="head"):
        from equiformer_amd import dropout
        self.seed, self.n, self.out_call, self.masks, self.keep_mask = seed, 0, None, [], dropout.keep_mask
        for rb, mb in zip(ref.blocks, mod.blocks):
            for r_sub, m_sub in ((getattr(rb, rb.attn_name), mb.attention), (rb.ffn, mb.ffn)):
                if m_sub.proj_drop is not None:
                    r_sub.register_forward_hook(self._proj(m_sub.proj_drop))
        if mod.out_dropout is not None:
            names = [head] + (["head_skip_connect"] if hasattr(ref, "head_skip_connect") else [])
            for name in names:
                getattr(ref, name).register_forward_pre_hook(self._out(mod.out_dropout))

    def reset(self):
        self.n, self.out_call = 0, None
        del self.masks[:]

    def _mask(self, call, x, m):
        f = self.keep_mask(self.seed, call, x.shape[0], m.irreps, m.drop_prob, m.scalars_only, expand="e3nn")
        self.masks.append(f)
        return f.to(x.dtype)

    def _proj(self, m):
        def hook(module, inputs, output):
            if not module.training:
                return None
            self.n += 1
            return output * self._mask(self.n - 1, output, m)
        return hook

    def _out(self, m):
        def hook(module, args):
            if not module.training:
                return None
            if self.out_call is None:
                self.out_call, self.n = self.n, self.n + 1
            return (args[0] * self._mask(self.out_call, args[0], m),) + tuple(args[1:])
        return hook

    def assert_mixed(self):
        assert self.masks
        for f in self.masks:
            assert bool((f == 0).any()) and bool((f > 1).any()), "a mask without a dropped and a kept entry"


def _under_draws(mod, run, seed, n_calls):
    """one training-mode forward under device_draws(seed): the CPU generator untouched, the dropout counter at n_calls; the same
    seed again gives the same bits, another seed other outputs"""
    from equiformer_amd import droppath
    state = torch.get_rng_state()
    with droppath.device_draws(seed) as d:
        out = run()
        assert (d.dropout_calls, d.calls) == (n_calls, 0), (d.dropout_calls, d.calls)
    assert torch.equal(torch.get_rng_state(), state), "device draws consumed the CPU generator"
    with droppath.device_draws(seed):
        again = run()
    with droppath.device_draws(seed + 1):
        other = run()
    for a, b in zip(again, out):
        assert torch.equal(a.detach(), b.detach())
    assert not torch.equal(other[0].detach(), out[0].detach())
    return out


OC20_CASES = {"aux": dict(use_auxiliary_task=True), "aux_l1_feature": dict(use_auxiliary_task=True, irreps_feature="64x0e+32x1e"),
              "attn_aux": dict(use_attention_head=True, use_auxiliary_task=True)}


@pytest.mark.parametrize("kind", sorted(OC20_CASES))
def test_oc20_out_drop_matches_the_hooked_oracle(kind):
    """SMALL_OC20, out_drop 0.4 on the scalar channels: the energy head (and an attention head with its skip connection) reads the
    dropped features, the auxiliary head the un-dropped ones."""
    import make_golden as mg
    seed = 7
    cfg = dict(mg.SMALL_OC20, number_of_basis=32, out_drop=P, **OC20_CASES[kind])
    ref, mod = th._models(cfg)
    inp = th._slab(4, 16, seed=9)
    ref.eval(); mod.eval()
    _, (e_eval, v_eval) = th._run(ref, mod, inp)
    ref.train(); mod.train()
    hooks = _OracleDropout(ref, mod, seed)
    out_r = ref(inp[2], inp[3], inp[0].double(), inp[1], edge_index=inp[4], offsets=inp[5].double())
    assert hooks.n == 1 and len(hooks.masks) == (2 if kind == "attn_aux" else 1)
    hooks.assert_mixed()
    if kind == "aux_l1_feature":  # the scalars variant: the 32x1e columns keep the factor 1
        assert bool((hooks.masks[0][:, 64:] == 1).all()) and bool((hooks.masks[0][:, :64] == 0).any())
    data = SimpleNamespace(pos=inp[0].to(DEV), batch=inp[1].to(DEV), atomic_numbers=inp[2].to(DEV), tags=inp[3].to(DEV),
                           edge_index=inp[4].to(DEV), offsets=inp[5].to(DEV))
    out = _under_draws(mod, lambda: mod(data), seed, 1)
    print("%s, out_drop vs hooked oracle: energy %.2e, vectors %.2e, train vs eval %.2e"
          % (kind, th._rel(out[0], out_r[0]), th._rel(out[1], out_r[1]), th._rel(out[0], e_eval)))
    assert th._rel(out[0], out_r[0]) < 1e-4 and th._rel(out[1], out_r[1]) < 1e-4
    assert th._rel(out[0], e_eval) > 1e-3  # something was really dropped
    p_r = ref.blocks[0].ga.sep_act.lin.tp.weight
    p = mod.blocks[0].ga.sep_act.lin.tp.weight
    (gr,) = torch.autograd.grad(out_r[0].sum() + out_r[1].sum(), [p_r])
    (gg,) = torch.autograd.grad(out[0].sum() + out[1].sum(), [p])
    print("   probed parameter gradient %.2e" % th._rel(gg, gr))
    assert th._rel(gg, gr) < 2e-4
    if kind != "attn_aux":
        # the auxiliary head reads the un-dropped features: with the same weights its vectors are those of the out_drop = 0 model
        from equiformer_amd import droppath
        from equiformer_amd.nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20
        plain = GraphAttentionTransformerOC20(None, None, 1, **dict(cfg, out_drop=0.0))
        plain.load_state_dict(mod.state_dict(), strict=True)
        plain = plain.to(DEV).train()
        with droppath.device_draws(seed) as d:
            e_plain, v_plain = plain(data)
            assert d.dropout_calls == 0
        assert torch.equal(_bits(v_plain), _bits(out[1])) and not torch.equal(e_plain, out[0])
    else:
        assert th._rel(out[1], v_eval) > 1e-3, "the attention head's vectors read the dropped features"


def _qm9_pair(ocls, cls, cfg, seed=21):
    from weights import fill_deterministic
    kw = dict(irreps_in="5x0e", max_radius=5.0, number_of_basis=32, **cfg)
    ref = fill_deterministic(ocls(**kw), seed).double().train()
    mod = cls(**kw)
    mod.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return ref, mod.to(DEV).train()


def _qm9_case(ref, mod, n_calls, probe):
    from equiformer_amd.synthetic import qm9_like_batch
    seed = 7
    d = qm9_like_batch(3, 12, side=5.5, seed=8)
    hooks = _OracleDropout(ref, mod, seed)
    yr = ref(None, d["pos"].double(), d["batch"], d["z"])
    assert hooks.n == n_calls == len(hooks.masks)
    hooks.assert_mixed()
    pos, batch, z = d["pos"].to(DEV), d["batch"].to(DEV), d["z"].to(DEV)
    mod.eval()
    y_eval = mod(None, pos, batch, z)
    mod.train()
    (y,) = _under_draws(mod, lambda: (mod(None, pos, batch, z),), seed, n_calls)
    (gr,) = torch.autograd.grad(yr.sum(), [probe(ref)])
    (gg,) = torch.autograd.grad(y.sum(), [probe(mod)])
    print("energies vs hooked oracle %.2e, probed gradient %.2e, train vs eval %.2e" % (th._rel(y, yr), th._rel(gg, gr), th._rel(y, y_eval)))
    assert th._rel(y, yr) < 1e-4 and th._rel(gg, gr) < 2e-4
    assert th._rel(y, y_eval) > 1e-3


def test_qm9_out_drop_and_proj_drop_match_the_hooked_oracle():
    """SMALL_L2 with both rates at 0.4: a dropout behind every block's attention and feed-forward network and one in front of the
    head -- 2 num_layers + 1 calls"""
    import make_golden as mg
    from oracle import nets as onets
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    cfg = dict(mg.SMALL_L2, out_drop=P, proj_drop=P)
    ref, mod = _qm9_pair(onets.GraphAttentionTransformer, GraphAttentionTransformer, cfg)
    _qm9_case(ref, mod, 2 * cfg["num_layers"] + 1, lambda m: m.blocks[0].ga.sep_act.lin.tp.weight)


def test_dot_product_attention_proj_drop_matches_the_hooked_oracle():
    import make_golden as mg
    from oracle import nets as onets
    from equiformer_amd.nets.dp_attention_transformer import DotProductAttentionTransformer
    cfg = dict(mg.SMALL_DP_L2, proj_drop=P)
    ref, mod = _qm9_pair(onets.DotProductAttentionTransformer, DotProductAttentionTransformer, cfg)
    _qm9_case(ref, mod, 2 * cfg["num_layers"], lambda m: m.blocks[0].dpa.proj.tp.weight)


def test_md17_force_loss_differentiates_through_out_drop():
    """test_md17_force_loss_second_order_gradients on SMALL_L2 with out_drop 0.4: the forces come from a create_graph backward
    through the dropout, the gradients of L = <a, E> + <B, F> from the second-order pass -- both the same launch with the saved
    seed.  Against the oracle's double backward, 1e-4 on every parameter."""
    import make_golden as mg
    from oracle import nets as onets
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer_md17 import GraphAttentionTransformerMD17
    from equiformer_amd.synthetic import md17_aspirin_batch
    seed = 7
    kw = dict(irreps_in="64x0e", max_radius=5.0, number_of_basis=32, basis_type="exp", **dict(mg.SMALL_L2, out_drop=P))
    ref = fill_deterministic(onets.GraphAttentionTransformerMD17(**kw), 12).double().train()
    mod = fill_deterministic(GraphAttentionTransformerMD17(**kw), 12).to(DEV).train()
    d = md17_aspirin_batch(2, seed=3)
    g = torch.Generator().manual_seed(1)
    a = torch.randn(2, 1, generator=g, dtype=torch.float64)
    B = torch.randn(42, 3, generator=g, dtype=torch.float64)
    hooks = _OracleDropout(ref, mod, seed)
    Er, Fr = ref(d["z"], d["pos"].double(), d["batch"])
    assert hooks.n == 1
    hooks.assert_mixed()
    gr = torch.autograd.grad((a * Er).sum() + (B * Fr).sum(), list(ref.parameters()), allow_unused=True)
    z, pos, batch = d["z"].to(DEV), d["pos"].to(DEV), d["batch"].to(DEV)
    mod.eval()
    with torch.no_grad():
        E_eval, _ = mod(z, pos, batch)
    mod.train()
    E, F = _under_draws(mod, lambda: mod(z, pos, batch), seed, 1)
    assert F.requires_grad, "training-mode forces must carry a graph"
    L = (a.float().to(DEV) * E).sum() + (B.float().to(DEV) * F).sum()
    gg = torch.autograd.grad(L, list(mod.parameters()), allow_unused=True)
    print("md17 with out_drop: energy %.2e, forces %.2e, train vs eval %.2e" % (th._rel(E, Er), th._rel(F, Fr), th._rel(E, E_eval)))
    assert th._rel(E, Er) < 1e-4 and th._rel(F, Fr) < 1e-4 and th._rel(E, E_eval) > 1e-3
    worst = ("", 0.0)
    for (n, _), x, r in zip(ref.named_parameters(), gg, gr):
        if r is None or r.abs().max() == 0:
            continue
        assert x is not None, n
        e = th._rel(x, r)
        if e > worst[1]:
            worst = (n, e)
    print("   worst second-order gradient error: %s %.3e" % worst)
    assert worst[1] < 1e-4, worst


# ------------------------------------------------------------------------------------------------ 3. padded equals unpadded
FEATURE = "64x0e+32x1e"  # the slab model's feature: the scalars variant drops 64 of its 96 irreps


def _slab_model():
    """tests/test_gpu_is2rs_step.py's model with out_drop 0.4 (no stochastic depth), the same initial weights at every call"""
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20
    cfg = dict(mg.SMALL_OC20, number_of_basis=32, alpha_drop=0.0, out_drop=P, irreps_feature=FEATURE, use_auxiliary_task=True)
    m = GraphAttentionTransformerOC20(None, None, 1, otf_graph=True, use_pbc=True, max_neighbors=pi.SLAB_CAP, **cfg)
    return fill_deterministic(m, 21).to(DEV).train()


_PADDED = {}


def _padded_and_unpadded(seed=7):
    """the protocol of tests/test_gpu_droppath.py: one forward of the slab model on the unpadded batch and on the padded bucket
    view under device_draws(seed), the padded one under seed + 1 as well; the entries the dropout zeroed.  Computed once."""
    from equiformer_amd import dropout, droppath
    from equiformer_amd.capture import bucket_of
    from equiformer_amd.graph import EdgeGraph
    if _PADDED:
        return _PADDED
    m = _slab_model()
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in t6._slab_batch().items()}
    B, N = d["num_graphs"], d["pos"].shape[0]
    zeroed = []
    hook = m.out_dropout.register_forward_hook(lambda mod, inp, out: zeroed.append(out == 0))
    assert isinstance(m.out_dropout, dropout.EquivariantScalarsDropout)
    with torch.no_grad():
        with droppath.device_draws(seed):
            e0, v0 = m(SimpleNamespace(**d))
        plan = EdgeGraph.radius_pbc_plan(d["pos"], d["cell"], d["batch"], R, pi.SLAB_CAP, B)
        cap = bucket_of(B, plan.N, plan.E, *td.PAD_STEPS)[1:]
        assert plan.E < cap[1] < 4000  # (batch and bucket on one side of the kernel-dispatch thresholds)
        g, _, _ = EdgeGraph.from_radius_pbc(d["pos"], d["cell"], d["batch"], R, pi.SLAB_CAP, num_graphs=B, capacity=cap,
                                            z=d["atomic_numbers"])
        assert g.N > N and int(g.batch.max()) == B
        view = SimpleNamespace(pos=g.pos, batch=g.batch, atomic_numbers=g.z, offsets=g.offsets,
                               tags=torch.zeros(cap[0], dtype=torch.int64, device=DEV))
        view.tags[:N] = d["tags"]
        with droppath.device_draws(seed):
            e1, v1 = m(view, graph=g, offsets=g.offsets)
        with droppath.device_draws(seed + 1):
            e2, _ = m(view, graph=g, offsets=g.offsets)
    hook.remove()
    assert len(zeroed) == 3
    _PADDED.update(B=B, N=N, Np=g.N, e0=e0, v0=v0, e1=e1, v1=v1, e2=e2, z0=zeroed[0], z1=zeroed[1], seed=seed)
    return _PADDED


def test_padded_view_drops_on_its_real_rows_what_the_unpadded_batch_drops():
    """The entries out_drop zeroes on the real rows of the padded view are those it zeroes on the unpadded batch, and those
    `keep_mask` names -- the phantom rows have draws of their own; the outputs of the real rows agree within the bound of
    test_oc20_model_parity_under_padding (1e-4)."""
    from equiformer_amd import dropout
    r = _padded_and_unpadded()
    B, N = r["B"], r["N"]
    want = dropout.keep_mask(r["seed"], 0, r["Np"], FEATURE, P, scalars_only=True, expand="cf") == 0
    assert bool(want[:N].any()) and not bool(want[:N, :64].all()) and not bool(want[:, 64:].any())
    assert bool(want[N:].any()), "the phantom rows draw for themselves"
    assert r["z0"].shape == (N, want.shape[1]) and r["z1"].shape == want.shape
    assert torch.equal(r["z0"].cpu(), want[:N]) and torch.equal(r["z1"][:N].cpu(), want[:N])
    assert r["e1"].shape[0] == B + 1 and not torch.equal(r["e2"][:B], r["e1"][:B])
    print("padded vs unpadded under one seed: energies %.3e, vectors %.3e" % (t6._rel(r["e1"][:B], r["e0"]), t6._rel(r["v1"][:N], r["v0"])))
    assert t6._rel(r["e1"][:B], r["e0"]) < 1e-4 and t6._rel(r["v1"][:N], r["v0"]) < 1e-4


def test_padded_energies_are_bit_equal_to_unpadded():
    """Padded against unpadded under one seed, both on the same side of the 4 000-edge dispatch threshold (the same kernels):
    the energies of the real structures and the auxiliary vectors of the real atoms are bit-equal."""
    r = _padded_and_unpadded()
    e1, e0 = r["e1"][:r["B"]], r["e0"]
    print("padded vs unpadded energies: %s / %s, rel %.3e" % (e1.flatten().tolist(), e0.flatten().tolist(), t6._rel(e1, e0)))
    assert torch.equal(_bits(e1), _bits(e0)), (e1.flatten().tolist(), e0.flatten().tolist())
    assert torch.equal(_bits(r["v1"][:r["N"]]), _bits(r["v0"]))


# ---------------------------------------------------------------------------------------------------------- 4. captured steps
def _step_masks(seed, steps, rows, irreps, scalars_only):
    from equiformer_amd import dropout
    from equiformer_amd.is2rs import step_seed
    return [dropout.keep_mask(step_seed(seed, k), 0, rows, irreps, P, scalars_only) for k in range(steps)]


def test_captured_step_with_out_drop_equals_eager_loop(monkeypatch):
    """The 8-step protocol of test_captured_step_with_stochastic_depth_equals_eager_loop on the slab model with out_drop 0.4:
    3 eager padded steps, one capture, 5 replays against 8 eager unpadded steps under device_draws(step_seed(s, k))."""
    s = 4242
    N = t6._slab_batch()["pos"].shape[0]
    masks = _step_masks(s, 8, N, FEATURE, True)
    assert all(not torch.equal(a, b) for i, a in enumerate(masks[3:]) for b in masks[3:][i + 1:]), "replayed steps share a mask"
    assert all(bool((f[:, :64] == 0).any()) and bool((f[:, :64] > 1).any()) for f in masks)
    monkeypatch.setattr(td, "_slab_model", _slab_model)
    e = td._train_slab(8, False, s)
    b = td._train_slab(8, True, s)
    ts = b["ts"]
    assert (ts.eager_steps, ts.captures, ts.replays) == (3, 1, 5), (ts.eager_steps, ts.captures, ts.replays)
    print("losses eager %s\n    captured %s" % (e["losses"], b["losses"]))
    t6._assert_trains_as_eager(e, b, 8, t6.LR)


def test_replays_draw_fresh_masks(monkeypatch):
    """Learning rate 0, no perturbation, a constant loss weight: the replays of one batch differ by their masks only.  Each loss
    equals the eager unpadded loss under that step's seed within 2e-5.  `drop_path_seed` is left to its default, the step's seed."""
    s, steps = 99, 6
    monkeypatch.setattr(td, "_slab_model", _slab_model)
    kw = dict(lr=0.0, interpolate=False, weight=1.0, decay=False, explicit=False)
    b = td._train_slab(steps, True, s, min_eager=1, **kw)
    ts = b["ts"]
    assert (ts.eager_steps, ts.captures, ts.replays) == (1, 1, steps - 1)
    e = td._train_slab(steps, False, s, **kw)
    print("losses eager %s\n    captured %s" % (e["losses"], b["losses"]))
    assert len({round(x, 6) for x in b["losses"][1:]}) >= 2, "every replay returned one loss: a frozen mask"
    for k, (x, y) in enumerate(zip(e["losses"], b["losses"])):
        assert abs(x) < 10 and abs(x - y) <= 2e-5, (k, x, y)


def _qm9_train(bucketed, d, s, steps, lr, **rates):
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd import droppath
    from equiformer_amd.capture import BucketedTrainStep
    from equiformer_amd.dens import step_seed
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    from equiformer_amd.optim import FlatAdamW
    m = GraphAttentionTransformer(irreps_in="5x0e", max_radius=tb.R, number_of_basis=32, **dict(mg.SMALL_L2, alpha_drop=0.0, **rates))
    m = fill_deterministic(m, 21).to(DEV).train()
    opt = FlatAdamW(m.parameters(), lr=lr, weight_decay=1e-2)
    bs = BucketedTrainStep(opt, tb._padded_loss(m), tb.R, node_step=tb.NODE_STEP, edge_step=tb.EDGE_STEP, min_eager=1,
                           drop_path_seed=s) if bucketed else None
    losses = []
    for k in range(steps):
        if bucketed:
            loss = bs.step(d)
        else:
            opt.zero_grad(set_to_none=True)
            with droppath.device_draws(step_seed(s, k)):
                loss = tb._unpadded_loss(m, d)
                loss.backward()
            opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return dict(losses=losses, p=opt.flat_p.detach().clone(), m=opt.flat_m.detach().clone(), step=opt._step, bs=bs)


def test_bucketed_step_on_molecules_with_proj_drop_equals_eager_loop():
    """SMALL_L2 on a QM9-like batch, proj_drop 0.4, min_eager=1: one eager padded step, the capture, 3 replays against 4 eager
    unpadded steps; the bounds of tests/test_gpu_bucketed_capture.py."""
    s, steps, lr = 31, 4, 1e-3
    d = tb._varying(1)[0]
    masks = _step_masks(s, steps, d["pos"].shape[0], "64x0e+32x1e+32x2e", False)
    assert all(not torch.equal(a, b) for i, a in enumerate(masks[1:]) for b in masks[1:][i + 1:]), "replayed steps share a mask"
    e, b = _qm9_train(False, d, s, steps, lr, proj_drop=P), _qm9_train(True, d, s, steps, lr, proj_drop=P)
    bs = b["bs"]
    assert (bs.eager_steps, bs.captures, bs.replays) == (1, 1, 3), (bs.eager_steps, bs.captures, bs.replays)
    print("losses eager %s\n    captured %s" % (e["losses"], b["losses"]))
    assert len({round(x, 6) for x in b["losses"]}) > 1
    tb._assert_trains_as_eager(e, b, steps, lr)


# ------------------------------------------------------------------------------------------------------------ 5. default seed
def test_default_seed_is_one_draw_taken_by_the_first_dropping_forward():
    """drop_path_seed=None: the base seed comes from torch's CPU generator when the first dropout runs under the instance; a
    model with out_drop 0 leaves the generator alone (alpha_drop is 0 here: nothing else draws)."""
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.capture import BucketedTrainStep
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    from equiformer_amd.optim import FlatAdamW
    d = tb._varying(1)[0]

    def run(rate, steps=3):
        m = GraphAttentionTransformer(irreps_in="5x0e", max_radius=tb.R, number_of_basis=32,
                                      **dict(mg.SMALL_L2, alpha_drop=0.0, out_drop=rate))
        m = fill_deterministic(m, 21).to(DEV).train()
        opt = FlatAdamW(m.parameters(), lr=0.0, weight_decay=0.0)
        bs = BucketedTrainStep(opt, tb._padded_loss(m), tb.R, node_step=tb.NODE_STEP, edge_step=tb.EDGE_STEP, min_eager=1)
        torch.manual_seed(11)
        losses = [float(bs.step(d)) for _ in range(steps)]
        return bs, losses, torch.get_rng_state()

    torch.manual_seed(11)
    for _ in range(3 + 1):  # the attention-dropout seed word: one draw per step and one more at the capture, as before
        torch.randint(0, 2 ** 62, (1,))
    plain_state = torch.get_rng_state()
    torch.randint(0, 2 ** 62, (1,))
    one_more = torch.get_rng_state()
    bs0, _, state0 = run(0.0)
    assert torch.equal(state0, plain_state), "a model without dropout consumed the generator"
    assert bs0._drop_path._drawn is None
    bs1, losses1, state1 = run(P)
    assert bs1._drop_path._drawn is not None and len(set(losses1)) > 1, losses1
    assert torch.equal(state1, one_more), "the base seed is one draw, taken once"
