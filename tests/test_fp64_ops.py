"""The float64 restatements of tests/fp64_ops.py against what the project already trusts on the CPU: the oracle modules
(e3nn layout), torch.nn.functional and the layout permutations of equiformer_amd.layout -- on the same ragged inputs
that tests/test_gpu_op_edges.py feeds the HIP kernels.  Agreement is at 1e-12 of the result's scale.  No GPU.

Last two parts: the dot-product attention restatements (kv_split, kv_merge, dp_logits) against the oracle's own pieces on the
head layouts of tests/dp_edge_cases.py, and negative controls for tests/test_gpu_dp_edges.py and tests/test_gpu_dtp_edges.py: a
restatement that is wrong in the way a kernel could be (heads exchanged, another segment's scale, keys for values, a wrong
out_ch, the neighbouring channel's weight) must miss, on the GPU tests' inputs, the bound those tests apply, by >= 10 x."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_edge_cases as dpc  # noqa: E402
import dtp_edge_cases as dtc  # noqa: E402
import fp64_ops as fo  # noqa: E402
import fp64_tp as tp  # noqa: E402
from equiformer_amd import ops, so3  # noqa: E402
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


# ------------------------------------------------------------------------------------------------- dot-product attention
def _dp_oracle(q_e3, kv_e3, dst, head_irr, H):
    """the oracle's own pieces (oracle.nets.DotProductAttention.forward): vec2heads on irreps_head * H and * 2H, the narrow,
    the ScaleFactor and the einsum"""
    oh = e3.Irreps(head_irr)
    chan = 1.0 / (oh.num_irreps ** 0.5)
    scale = torch.cat([torch.full((mul * ir.dim,), chan / ir.dim ** 0.5, dtype=torch.float64) for mul, ir in oh])
    q = onets.vec2heads(q_e3, oh, H) * scale
    kv = onets.vec2heads(kv_e3, oh, 2 * H)
    k, v = kv[:, :H], kv[:, H:]
    return torch.einsum("bik,bik->bi", q[dst], k), onets.heads2vec(k, oh), onets.heads2vec(v, oh)


@pytest.mark.parametrize("head_irr,H", dpc.HEADS)
def test_dp_restatements_match_oracle(head_irr, H):
    """kv_split, its inverse and dp_logits: values, gradients and second derivatives on the ragged graph's first rows"""
    seg, seg2 = fo.all_heads_layout(head_irr, H), fo.all_heads_layout(head_irr, 2 * H)
    lay, lay2 = RowLayout(dpc.irreps_str(seg)), RowLayout(dpc.irreps_str(seg2))  # the layouts the kernels are given
    assert lay.segs == seg.segs and all(m % H == 0 and (m // H) % 4 == 0 for m, _ in lay.segs) and H <= 8
    assert dpc.groups(head_irr, H) * 4 == seg.dim and lay2.dim == 2 * seg.dim
    graph = dpc.graph("ragged")
    E = 200
    dst = graph.dst.long()[:E]
    N = int(dst.max()) + 2
    p, p2 = seg.perm_from_e3nn(), seg2.perm_from_e3nn()
    inv, inv2 = torch.empty_like(p), torch.empty_like(p2)
    inv[p], inv2[p2] = torch.arange(p.numel()), torch.arange(p2.numel())
    d = dpc.inputs(head_irr, H, N, E)
    qc, kvc = d["q"].clone().requires_grad_(True), d["kv"].clone().requires_grad_(True)
    qe, kve = d["q"][:, inv].clone().requires_grad_(True), d["kv"][:, inv2].clone().requires_grad_(True)
    lw, kw, vw = _dp_oracle(qe, kve, dst, head_irr, H)
    k, v = fo.kv_split(kvc, seg, H)
    lg = fo.dp_logits(qc, k, dst, seg, H)
    assert torch.equal(k.detach(), kw.detach()[:, p]) and torch.equal(v.detach(), vw.detach()[:, p])
    assert _close(lg, lw)
    assert torch.equal(fo.kv_merge(k, v, seg, H).detach(), kvc.detach())
    zero = torch.zeros_like(k)
    assert torch.equal(fo.kv_merge(k, None, seg, H).detach(), fo.kv_merge(k, zero, seg, H).detach())
    assert torch.equal(fo.kv_split(fo.kv_merge(None, v, seg, H), seg, H)[0].detach(), zero.detach())
    gw = torch.autograd.grad([lw, kw, vw], [qe, kve], [d["cl"], d["ck"][:, inv], d["cv"][:, inv]], create_graph=True)
    gg = torch.autograd.grad([lg, k, v], [qc, kvc], [d["cl"], d["ck"], d["cv"]], create_graph=True)
    assert _close(gg[0], gw[0][:, p]) and _close(gg[1], gw[1][:, p2])
    hw = torch.autograd.grad((gw[0] * d["a"][:, inv]).sum() + (gw[1] * d["b"][:, inv2]).sum(), [qe, kve])
    hg = torch.autograd.grad((gg[0] * d["a"]).sum() + (gg[1] * d["b"]).sum(), [qc, kvc])
    assert _close(hg[0], hw[0][:, p]) and _close(hg[1], hw[1][:, p2])


def _dp_eval(head_irr, H, dtype, q=None, kv=None, swap=None):
    """(logit, k, v, dq, dk) of the restatement on the GPU test's ragged inputs"""
    seg = fo.all_heads_layout(head_irr, H)
    graph = dpc.graph("ragged")
    dst = graph.dst.long()
    d = dpc.inputs(head_irr, H, graph.N, graph.E)
    q = (d["q"] if q is None else q).to(dtype).requires_grad_(True)
    k, v = fo.kv_split((d["kv"] if kv is None else kv).to(dtype), seg, H)
    k = k.detach().requires_grad_(True)
    kk = k if swap is None else swap(k)
    lg = fo.dp_logits(q, kk, dst, seg, H)
    dq, dk = torch.autograd.grad(lg, [q, k], d["cl"].to(dtype))
    return dict(logit=lg.detach(), k=k.detach(), v=v.detach(), dq=dq, dk=dk)


@pytest.mark.parametrize("head_irr,H", [h for h in dpc.HEADS if h[1] > 1 and len(fo.Segs(h[0]).segs) > 1])
def test_dp_wrong_restatements_miss_the_gpu_bound(head_irr, H):
    """negative controls for tests/test_gpu_dp_edges.py, on its ragged inputs: two heads exchanged in one segment, the scale of
    one segment on another, keys and values exchanged in one segment -- each leaves a per-row error far above the bound
    max(1e-5, 4 x float32 yardstick) that test applies to the quantity"""
    seg = fo.all_heads_layout(head_irr, H)
    graph = dpc.graph("ragged")
    d = dpc.inputs(head_irr, H, graph.N, graph.E)
    ref, y32 = _dp_eval(head_irr, H, torch.float64), _dp_eval(head_irr, H, torch.float32)
    lim = {n: dpc.bound(fo.per_row_rel(y32[n], ref[n])) for n in ("logit", "dq")}
    lim["dk"] = lim["k"] = lim["v"] = dpc.bound()
    assert all(v < 1e-4 for v in lim.values()), lim  # the yardstick leaves the bounds near the plain 1e-5
    last = len(seg.segs) - 1
    wrong = {"heads": _dp_eval(head_irr, H, torch.float64, swap=lambda k: dpc.swap_heads(k, seg, H, last, 0, H - 1)),
             "scale": _dp_eval(head_irr, H, torch.float64, q=dpc.rescale_segment(d["q"], seg, H, last, 0)),
             "kv": _dp_eval(head_irr, H, torch.float64, kv=dpc.swap_kv(d["kv"], seg, last))}
    seen = {(w, n): fo.per_row_rel(wrong[w][n], ref[n]) / lim[n]
            for w, n in (("heads", "logit"), ("heads", "dq"), ("heads", "dk"), ("scale", "logit"), ("scale", "dk"),
                         ("kv", "k"), ("kv", "v"), ("kv", "logit"))}
    print(seen)
    assert all(v >= 10.0 for v in seen.values()), seen


# ------------------------------------------------------------------------------------------------- un-fused tensor product
def test_dtp_edge_tables_are_what_the_gpu_test_says():
    """the properties tests/test_gpu_dtp_edges.py relies on, from the tables and the source constants"""
    import re
    w = {n: dtc.table(n).weight_numel for n in dtc.TABLES}
    assert w["narrow"] == 72 and w["two_blocks"] == 480 and w["two_blocks"] > 256 >= w["narrow"]
    t = dtc.table("l3")
    assert sum(m for m, _ in t.layout_in.segs) > 256 and max(p["l1"] for p in t.paths) == 3
    assert dtc.table("parity").has_odd and all(dtc.table(n).in_covered for n in dtc.TABLES if n != "uncovered")
    t = dtc.table("uncovered")
    assert not t.in_covered and {p["in_off"] for p in t.paths} == {0} and t.layout_in.offsets == [0, 8]
    src = open(os.path.join(os.path.dirname(os.path.abspath(dtc.__file__)), "..", "equiformer_amd", "csrc", "gemm.hip")).read()
    assert int(re.search(r"constexpr int ROWS_PAIRS = (\d+);", src).group(1)) == dtc.ROWS_PAIRS
    assert int(re.search(r"constexpr int MAX_MTILE = (\d+);", src).group(1)) == dtc.MAX_MTILE
    K = {n: [k for k, _ in dtc.table(n).layout_out.segs] for n in dtc.LIN_TABLES}
    assert K["k96"] == [96, 192, 192] and K["k288"] == [128, 256, 288] and len(K["deg3"]) == 4
    for n in dtc.LIN_TABLES:  # the spec accepts every consumer, and every tile the dispatch picks fits the loader and the LDS tile
        t = dtc.table(n)
        for N in dtc.LIN_N:
            assert ops.DtpLinearSpec.make(t, dtc.consumer(n, N)) is not None
            for (_, l3), par in zip(t.layout_out.segs, t.layout_out.par):
                for E in dtc.lin_edges(t.lmax_sh):
                    dtc.tile_of(t, l3, par, N, E)
    # the edges-per-tile values the GPU test is meant to straddle
    t = dtc.table("deg3")
    assert [dtc.tile_of(t, l, 1, 64, 9)[2] for l in range(4)] == [64, 21, 12, 9]
    assert [dtc.tile_of(t, l, 1, 32, 9) for l in range(4)] == [(64, 64, 64), (128, 32, 42), (128, 32, 25), (128, 32, 18)]
    assert {dtc.tn_tile_of(K, N) for K in (96, 192) for N in (32, 64)} == {(32, 32), (32, 64), (64, 32), (64, 64)}


@pytest.mark.parametrize("kind,use_w", [("out_ch", True), ("out_ch", False), ("w", True)])
def test_dtp_wrong_tables_miss_the_gpu_bound(kind, use_w):
    """negative controls for tests/test_gpu_dtp_edges.py on its inputs: a wrong out_ch of one path, and w of the neighbouring
    channel, against the bound max(plain, 4 x float32 yardstick) of every quantity they move"""
    t = dtc.table("two_blocks")
    bad = dtc.wrong_table(t, kind)
    for E in (2, 257):
        d = dtc.inputs("two_blocks", E)
        ins = [d["x"], d["M"]] + ([d["w"]] if use_w else [])
        names = ["out", "dx", "dM"] + (["dw"] if use_w else [])
        fn = lambda tab: (lambda x, M, w=None: tp.product(tab, x, M, w))  # noqa: E731
        ro, rg, yo, yg = fo.yardstick(fn(t), ins, [d["go"]])
        wo, wg = fo.evaluate(fn(bad), ins, [d["go"]], torch.float64)
        seen = {}
        for n, r, y, b in zip(names, ro + rg, yo + yg, wo + wg):
            lim = max(dtc.BOUNDS[n], dtc.YARD_FACTOR * fo.per_row_rel(y, r))
            assert lim < 1e-4, (n, lim)
            seen[n] = fo.per_row_rel(b, r) / lim
        print(kind, use_w, E, seen)
        moved = ["out", "dx", "dM"] + (["dw"] if (use_w and kind == "w") else [])
        assert all(seen[n] >= 10.0 for n in moved), seen
