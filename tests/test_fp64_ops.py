"""The float64 restatements of tests/fp64_ops.py against what the project already trusts on the CPU: the oracle modules
(e3nn layout), torch.nn.functional and the layout permutations of equiformer_amd.layout -- on the same ragged inputs
that tests/test_gpu_op_edges.py feeds the HIP kernels.  Agreement is at 1e-12 of the result's scale.  No GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ops as fo  # noqa: E402
from equiformer_amd import so3  # noqa: E402
from equiformer_amd.layout import RowLayout  # noqa: E402
from oracle import e3  # noqa: E402
from oracle import nets as onets  # noqa: E402

TOL = 1e-12


def _close(got, want, tol=TOL):
    scale = max(1.0, float(want.detach().abs().max())) if want.numel() else 1.0
    assert got.shape == want.shape
    return want.numel() == 0 or float((got - want).detach().abs().max()) < tol * scale


def _randn(shape, seed):
    return fo.f32r(torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64))


@pytest.mark.parametrize("irr", ["128x0e+64x1e+32x2e", "32x0e+16x1e+16x2e+8x3e", "8x0e+2x0o+4x1o"])
def test_layout_permutations(irr):
    lay, seg = RowLayout(irr), fo.Segs(irr)
    assert seg.dim == lay.dim and seg.offsets == lay.offsets and seg.segs == lay.segs and seg.par == lay.par
    assert torch.equal(seg.perm_from_e3nn(), lay.perm_from_e3nn())
    inv = lay.perm_to_e3nn()
    assert torch.equal(seg.perm_from_e3nn()[inv], torch.arange(lay.dim))
    assert fo.Segs(lay).segs == lay.segs  # from an object with .segs / .par


def test_per_row_rel_is_per_row():
    ref = torch.tensor([[100.0, 50.0], [1.0, 0.5], [0.0, 0.0]], dtype=torch.float64)
    got = ref.clone()
    got[1, 0] += 1e-3                                         # 1e-3 of its own row, 1e-5 of the tensor
    assert abs(fo.per_row_rel(got, ref) - 1e-3) < 1e-12
    got = ref.clone()
    got[2, 1] = 1e-3                                          # a zero row: measured against the floor 1e-3 * 100
    assert abs(fo.per_row_rel(got, ref) - 1e-2) < 1e-12
    got = ref.clone()
    got[0, 1] += 1.0                                          # per slice of a row: 1 / 50, not 1 / 100
    assert abs(fo.per_row_rel(got, ref, slices=[slice(0, 1), slice(1, 2)]) - 0.02) < 1e-12
    assert fo.per_row_rel(ref, ref) == 0.0 and fo.per_row_rel(ref * 0, ref * 0) == 0.0
    v, e = torch.tensor([4.0, 0.5, 2.0], dtype=torch.float64), torch.tensor([0.0, 0.05, 0.0], dtype=torch.float64)
    assert abs(fo.per_row_rel(v + e, v) - 0.1) < 1e-12                              # 1-D: one element per row
    assert abs(fo.per_row_rel(v + e, v, slices=[slice(None)]) - 0.0125) < 1e-12     # 1-D with slices: one row


def test_ragged_graph_degrees():
    g = fo.ragged_graph(fo.ATTN_DEGREES, 7, 1)
    rp = g.row_ptr.long()
    assert (rp[1:] - rp[:-1]).tolist() == fo.ATTN_DEGREES and g.E == sum(fo.ATTN_DEGREES) and g.N == len(fo.ATTN_DEGREES)
    assert torch.equal(g.dst.long(), fo.seg_of_ptr(g.row_ptr))
    assert int(g.src.max()) < 7 and int(g.src.long().bincount().max()) > 1  # repeats
    perm = g.src_perm.long()
    assert torch.equal(g.src.long()[perm], torch.sort(g.src.long()).values)


@pytest.mark.parametrize("family", fo.LN_FAMILIES)
@pytest.mark.parametrize("irr", fo.LN_IRREPS)
def test_layer_norm_matches_oracle(irr, family):
    """values and all gradients, also for a row with two 0e segments (64x0e+32x1e+16x0e), which RowLayout refuses"""
    seg = fo.Segs(irr)
    ref = onets.EquivariantLayerNormV2(e3.Irreps(irr)).double()
    w = (_randn(ref.affine_weight.shape, 1) * 0.5 + 1.0).requires_grad_(True)
    b = _randn(ref.affine_bias.shape, 2).requires_grad_(True)
    ref.affine_weight.data, ref.affine_bias.data = w.detach().clone(), b.detach().clone()
    p = seg.perm_from_e3nn()
    xc = fo.ln_input(family, 17, seg, 3).requires_grad_(True)
    x2 = fo.ln_input("randn", 17, seg, 4).requires_grad_(True)
    inv = torch.empty_like(p)
    inv[p] = torch.arange(p.numel())
    xe = (xc + x2).detach()[:, inv].requires_grad_(True)
    want = ref(xe)
    got, s = fo.add_layer_norm(xc, x2, w, b, seg)
    assert _close(got, want[:, p]) and torch.equal(s.detach(), (xc + x2).detach())
    assert _close(fo.layer_norm(xc + x2, w, b, seg), want[:, p])
    go = _randn(want.shape, 5)
    gw = torch.autograd.grad(want, [xe, ref.affine_weight, ref.affine_bias], go)
    gg = torch.autograd.grad(got, [xc, x2, w, b], go[:, p])
    assert _close(gg[0], gw[0][:, p]) and torch.equal(gg[0], gg[1])
    assert _close(gg[2], gw[1]) and _close(gg[3], gw[2])


@pytest.mark.parametrize("irr", ["128x0e+64x1e+32x2e", "384x0e+192x1e+192x2e+96x3e", "16x0e+8x1e"])
def test_gate_matches_oracle(irr):
    ref = onets.make_gate(e3.Irreps(irr))
    scalars, gates, gated = onets.irreps2gate(e3.Irreps(irr))
    S, G = scalars.dim, gates.dim
    gseg = fo.Segs(repr(gated).replace(" ", ""))
    sin = fo.Segs([(S + G, 0, 1)] + [(m, l, p) for (m, l), p in zip(gseg.segs, gseg.par)])
    sout = fo.Segs([(S, 0, 1)] + [(m, l, p) for (m, l), p in zip(gseg.segs, gseg.par)])
    pin, pout = sin.perm_from_e3nn(), sout.perm_from_e3nn()
    xe = (_randn((9, sin.dim), 6) * 30.0).requires_grad_(True)  # the sigmoids saturate on both sides
    xc = xe.detach()[:, pin].requires_grad_(True)
    want = ref(xe)
    got = fo.gate(xc, S, gseg, fo.normalize2mom(torch.nn.functional.silu), fo.normalize2mom(torch.sigmoid))
    assert _close(got, want[:, pout])
    go = _randn(want.shape, 7)
    (gw,), (gg,) = torch.autograd.grad(want, [xe], go), torch.autograd.grad(got, [xc], go[:, pout])
    assert _close(gg, gw[:, pin])


def test_constants_and_scalar_activations():
    assert abs(fo.c_smooth_leaky_relu() - e3.normalize2mom_const(onets.SmoothLeakyReLU(0.2))) < TOL
    assert abs(fo.c_smooth_leaky_relu() - so3.C_SMOOTH_LEAKY_RELU_02) < TOL
    assert abs(fo.normalize2mom(torch.nn.functional.silu) - so3.C_SILU) < TOL
    assert abs(fo.normalize2mom(torch.sigmoid) - so3.C_SIGMOID) < TOL
    x = _randn((1025,), 8) * 10.0
    x[:3] = torch.tensor([0.0, 30.0, -30.0])
    assert _close(fo.smooth_leaky_relu(x), onets.SmoothLeakyReLU(0.2)(x))
    assert _close(fo.scaled_silu(x, so3.C_SILU), onets.ScaledAct(torch.nn.functional.silu)(x))


@pytest.mark.parametrize("H,Kh", [(3, 32), (16, 32), (2, 8)])
def test_alpha_logits_match_oracle(H, Kh):
    a = (_randn((17, H * Kh), 9) * 2.0).requires_grad_(True)
    adot = _randn((1, H, Kh), 10).requires_grad_(True)
    act = onets.SmoothLeakyReLU(0.2)
    want = torch.einsum("bik,aik->bi", act(a.view(-1, H, Kh)) * e3.normalize2mom_const(act), adot)
    got = fo.alpha_logits(a, adot, H, Kh)
    assert _close(got, want)
    go = _randn(want.shape, 11)
    for x, y in zip(torch.autograd.grad(got, [a, adot], go, retain_graph=True), torch.autograd.grad(want, [a, adot], go)):
        assert _close(x, y)


@pytest.mark.parametrize("C,groups", [(1, 1), (3, 3), (30, 1), (50, 3), (64, 1)])
def test_ln_silu_matches_torch(C, groups):
    x = _randn((33, C * groups), 12).requires_grad_(True)
    gam = (_randn((C * groups,), 13) * 0.5 + 1.0).requires_grad_(True)
    bet = _randn((C * groups,), 14).requires_grad_(True)
    F = torch.nn.functional
    want = torch.cat([F.silu(F.layer_norm(x[:, k * C:(k + 1) * C], (C,), gam[k * C:(k + 1) * C], bet[k * C:(k + 1) * C],
                                          1e-5)) for k in range(groups)], dim=1)
    got = fo.ln_silu(x, gam, bet, 1e-5, groups)
    assert _close(got, want)
    go = _randn(want.shape, 15)
    for a, b in zip(torch.autograd.grad(got, [x, gam, bet], go, retain_graph=True),
                    torch.autograd.grad(want, [x, gam, bet], go)):
        assert _close(a, b)


def test_embedding_matches_oracle():
    irr, T = "128x0e+64x1e+32x2e", 40
    ref = onets.NodeEmbeddingNetwork(e3.Irreps(irr), T).double()
    ref.atom_type_lin.bias[0].data = _randn((128,), 16)
    z = torch.randint(0, T, (65,), generator=torch.Generator().manual_seed(17))
    want, _, _ = ref(z)
    W = ref.atom_type_lin.tp.weight.view(T, 128)
    got = fo.embedding(z, W, ref.atom_type_lin.bias[0], fo.Segs(irr).dim)
    assert _close(got, want)  # only 0e columns are populated: the two layouts coincide
    go = _randn(want.shape, 18)
    for a, b in zip(torch.autograd.grad(got, list(ref.parameters()), go, retain_graph=True),
                    torch.autograd.grad(want, list(ref.parameters()), go)):
        assert _close(a, b)


@pytest.mark.parametrize("head_irr,H", fo.ATTN_HEADS)
@pytest.mark.parametrize("regime", ["randn", "peak"])
def test_attention_matches_oracle(head_irr, H, regime):
    """softmax per destination + aggregation per head on the ragged graph, with and without a keep mask"""
    graph = fo.ragged_graph(fo.ATTN_DEGREES, 9, 19)
    seg = fo.all_heads_layout(head_irr, H)
    assert fo.head_groups(head_irr) * 4 * H == seg.dim
    dst, N, E = graph.dst.long(), graph.N, graph.E
    oh = e3.Irreps(head_irr)
    p = seg.perm_from_e3nn()
    logit = fo.attn_logits(regime, E, H, graph.row_ptr, 20).requires_grad_(True)
    ve = _randn((E, seg.dim), 21).requires_grad_(True)
    vc = ve.detach()[:, p].requires_grad_(True)
    keep = (torch.rand(E, H, generator=torch.Generator().manual_seed(22)) >= 0.25).double() / 0.75
    for k in (None, keep):
        alpha = onets.segment_softmax(logit, dst, N)
        wgt = alpha if k is None else alpha * k
        want = onets.heads2vec(onets.scatter_sum(onets.vec2heads(ve, oh, H) * wgt.unsqueeze(-1), dst, N), oh)
        got, al = fo.attn_aggregate(logit, vc, graph.row_ptr, H, seg, k)
        assert _close(got, want[:, p]) and _close(al, alpha)
        go = _randn(want.shape, 23)
        gw = torch.autograd.grad(want, [logit, ve], go)
        gg = torch.autograd.grad(got, [logit, vc], go[:, p])
        assert _close(gg[0], gw[0]) and _close(gg[1], gw[1][:, p])


@pytest.mark.parametrize("D", [1, 6, 480])
def test_segment_and_gather_restatements(D):
    ptr = torch.tensor([0] + fo.SEG_LENGTHS).cumsum(0)
    seg_of = fo.seg_of_ptr(ptr)
    n, nseg = int(ptr[-1]), len(fo.SEG_LENGTHS)
    assert seg_of.bincount(minlength=nseg).tolist() == fo.SEG_LENGTHS
    x = _randn((n, D), 24)
    assert _close(fo.segment_sum(x, ptr, 0.25), onets.scatter_sum(x, seg_of, nseg) * 0.25)
    y = _randn((nseg, D), 25)
    want = torch.stack([0.5 * y[int(s)] for s in seg_of])
    assert _close(fo.segment_bcast(y, seg_of, 0.5), want)
    s = _randn((nseg,), 26)
    assert _close(fo.segment_scale(x, s, seg_of), torch.stack([x[q] * s[int(seg_of[q])] for q in range(n)]))
    graph = fo.ragged_graph(fo.SEG_LENGTHS, 7, 27)
    a, b = _randn((graph.N, D), 28), _randn((graph.N, D), 29)
    src, dst = graph.src.long(), graph.dst.long()
    assert _close(fo.gather_add(a, b, src, dst), torch.stack([a[int(i)] + b[int(j)] for i, j in zip(src, dst)]))
    assert _close(fo.gather_add(a, None, src, dst), torch.stack([a[int(i)] for i in src]))


def test_fold_weight_restatement():
    lens = [1, 2, 63, 64, 65, 200, 1]
    row_start = torch.tensor([0] + lens).cumsum(0)
    w_of_row = torch.randperm(len(lens), generator=torch.Generator().manual_seed(30))
    W, w = _randn((int(row_start[-1]),), 31), _randn((len(lens),), 32)
    want = torch.cat([W[row_start[r]:row_start[r + 1]] * w[w_of_row[r]] for r in range(len(lens))])
    assert _close(fo.fold_weight(W, w, row_start, w_of_row), want)
