"""The path-table restatements of the tensor-product family (tests/fp64_tp.py: coupling, un-fused product, fused
SeparableFCTP) pinned on the CPU in fp64 against the oracle modules (e3nn layout, through the e3nn <-> channel-fastest
permutations of tests/test_gpu_ops.py): values, first derivatives and the second derivatives of
L = sum <b, d<a, f>/d .> to 1e-10.

Second part, negative controls for tests/test_gpu_second_order_ops.py: for every operator whose double backward is composed
of several substitution terms, the fp64 second-order gradients are computed once in full and once with one term removed (its
first derivative detached before L is formed, so its cotangent never reaches the double backward).  The two must differ by at
least 10 x the loosest bar the GPU test applies to that quantity -- on the very inputs the GPU test uses -- so a composition
that dropped the term could not pass there."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ops as fo  # noqa: E402
import fp64_tp as tp  # noqa: E402
import second_order_cases as cases  # noqa: E402
from second_order_ref import TOL, _second_order  # noqa: E402
from equiformer_amd import ops, so3  # noqa: E402
from equiformer_amd.layout import DtpTable, RowLayout  # noqa: E402
from oracle import e3  # noqa: E402
from oracle import nets as onets  # noqa: E402

torch.set_default_dtype(torch.float32)


def _close(got, want, tol):
    assert got.shape == want.shape
    assert (got - want).abs().max() <= tol * max(1.0, float(want.detach().abs().max())), float((got - want).abs().max())


def _pin(f_oracle, f_rest, ins_e3, lays, lay_out, seed):
    """ins_e3: oracle inputs (fp64, e3nn layout); lays[i]: RowLayout of input i (None: the same columns on both sides).
    Values, first derivatives wrt every input and d L / d (inputs, a) for L = sum_k <b_k, d<a, f>/d x_k>."""
    perm = [None if l is None else l.perm_from_e3nn() for l in lays]
    pout = lay_out.perm_from_e3nn()
    xe = [t.clone().requires_grad_(True) for t in ins_e3]
    xc = [(t if p is None else t[:, p]).clone().requires_grad_(True) for t, p in zip(ins_e3, perm)]
    ye, yc = f_oracle(*xe), f_rest(*xc)
    _close(yc, ye[:, pout], 1e-12)
    g = torch.Generator().manual_seed(seed)
    ae = torch.randn(ye.shape, generator=g, dtype=torch.float64).requires_grad_(True)
    ac = ae.detach()[:, pout].clone().requires_grad_(True)
    ge = torch.autograd.grad(ye, xe, ae, create_graph=True)
    gc = torch.autograd.grad(yc, xc, ac, create_graph=True)
    cf = lambda t, p: t if p is None else t[:, p]  # noqa: E731
    for a, b, p in zip(gc, ge, perm):
        _close(a, cf(b, p), 1e-11)
    be = [torch.randn(t.shape, generator=g, dtype=torch.float64) for t in ge]
    he = torch.autograd.grad(sum((b * t).sum() for b, t in zip(be, ge)), xe + [ae])
    hc = torch.autograd.grad(sum((cf(b, p) * t).sum() for b, t, p in zip(be, gc, perm)), xc + [ac])
    for a, b, p in zip(hc, he, perm + [pout]):
        _close(a, cf(b, p), 1e-10)


@pytest.mark.parametrize("case", sorted(cases.DTP))
def test_coupling_constants_are_the_kernels_table(case):
    """tp.coupling multiplies by so3.path_table in float64; table.cg, which the kernels read, is that table in float32"""
    table = DtpTable(*cases.DTP[case], cases.DTP[case][0])
    for p in table.paths:
        n = (2 * p["l1"] + 1) * (2 * p["l2"] + 1) * (2 * p["l3"] + 1)
        want = torch.from_numpy(so3.path_table(p["l1"], p["l2"], p["l3"])).reshape(-1).float()
        assert torch.equal(table.cg_host[p["cg_off"]:p["cg_off"] + n], want)


@pytest.mark.parametrize("use_w", [True, False])
@pytest.mark.parametrize("case", sorted(cases.DTP))
def test_product_and_coupling_against_the_oracle(case, use_w):
    """T(x, M(sh), w) == oracle.nets.DepthwiseTensorProduct(x, sh, w)  (w = None: unit weights)"""
    irr, sh_irr = cases.DTP[case]
    ref = onets.DepthwiseTensorProduct(irr, sh_irr, irr, bias=False).double()
    table = DtpTable(irr, sh_irr, irr)
    assert table.weight_numel == ref.tp.weight_numel and repr(table.irreps_out) == repr(ref.irreps_out.simplify())
    E = 6
    g = torch.Generator().manual_seed(11)
    x = torch.randn(E, table.layout_in.dim, generator=g, dtype=torch.float64)
    sh = torch.randn(E, (table.lmax_sh + 1) ** 2, generator=g, dtype=torch.float64)
    if use_w:
        w = torch.randn(E, table.weight_numel, generator=g, dtype=torch.float64)
        _pin(lambda a, b, c: ref(a, b, c), lambda a, b, c: tp.product(table, a, tp.coupling(table, b), c),
             [x, sh, w], [table.layout_in, None, None], table.layout_out, 12)
    else:
        ones = torch.ones(E, table.weight_numel, dtype=torch.float64)
        _pin(lambda a, b: ref(a, b, ones), lambda a, b: tp.product(table, a, tp.coupling(table, b), None),
             [x, sh], [table.layout_in, None], table.layout_out, 13)


@pytest.mark.parametrize("irr,sh_irr", [("32x0e+32x1e+32x2e", "1x0e+1x1e+1x2e"), ("32x0e+32x0o+32x1e+32x1o", "1x0e+1x1o")])
def test_fused_reference_against_the_oracle(irr, sh_irr):
    """reference(spec, x, M(sh), w, blocks(lin weight), bias) == oracle.nets.SeparableFCTP: its lin(dtp(x, sh, w)) with the
    per-edge weights w as an input (derivatives to second order), and the whole module, radial MLP included (values)"""
    torch.manual_seed(21)
    ref = onets.SeparableFCTP(irr, sh_irr, irr, [8, 16], use_activation=False).double()
    table, lay = DtpTable(irr, sh_irr, irr), RowLayout(irr)
    spec = ops.SfcSpec(table, lay, n2=0)
    g = torch.Generator().manual_seed(22)
    with torch.no_grad():
        ref.lin.bias[0].copy_(torch.randn(ref.lin.bias[0].shape, generator=g, dtype=torch.float64))
    weight, bias = ref.lin.tp.weight.detach(), ref.lin.bias[0].detach()
    assert weight.numel() == spec.weight_numel
    E = 5
    x = torch.randn(E, table.layout_in.dim, generator=g, dtype=torch.float64)
    sh = torch.randn(E, (table.lmax_sh + 1) ** 2, generator=g, dtype=torch.float64)
    es = torch.rand(E, 8, generator=g, dtype=torch.float64)
    w = ref.dtp_rad(es).detach()

    def rest(a, b, c):
        return tp.reference(spec, a, tp.coupling(table, b), c, tp.blocks(spec, weight), None, bias, None)[0]
    _pin(lambda a, b, c: ref.lin(ref.dtp(a, b, c)), rest, [x, sh, w], [table.layout_in, None, None], lay, 23)
    with torch.no_grad():
        _close(rest(x[:, table.layout_in.perm_from_e3nn()], sh, w), ref(x, sh, es)[:, lay.perm_from_e3nn()], 1e-12)


def test_second_consumer_of_the_reference_is_a_linear_on_the_0e_product():
    """out2 = T(x, M, w)[0e] . W2 + bias2, and out1 is the per-segment linear of T: `reference` against `product`"""
    c = cases.Fused("qm9_sep_act")
    x, M, w, weight, weight2, bias, bias2 = (t.detach() for t in c.split(c.inputs(7)))
    o1, o2 = tp.reference(c.spec, x, M, w, tp.blocks(c.spec, weight), weight2, bias, bias2)
    mid = tp.product(c.table, x, M, w)
    K0 = c.table.layout_out.segs[0][0]
    assert c.table.layout_out.segs[0][1] == 0 and c.table.layout_out.par[0] == 1
    _close(o2, mid[:, :K0] @ weight2.view(K0, c.n2) + bias2, 1e-13)
    _close(o1[:, :c.lay.segs[0][0]], mid[:, :K0] @ tp.blocks(c.spec, weight)[0] + bias, 1e-13)


# ------------------------------------------------------------------------------------------------- negative controls
def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _control(fn, inputs, names, diff, seed, bar, use=None):
    """for every member of `diff`: the largest change, over the second-order gradients, of dropping that member's cotangent,
    in units of the bar the GPU test applies to the quantity that changes; asserted >= 10"""
    _, full = _second_order(fn, inputs, diff, seed, use=use)
    out = {}
    for k in range(len(diff)):
        _, cut = _second_order(fn, inputs, diff, seed, use=use, drop=k)
        worst = 0.0
        for j, (f, c) in enumerate(zip(full, cut)):
            if f is None or float(f.abs().max()) == 0.0:
                continue
            c = torch.zeros_like(f) if c is None else c
            worst = max(worst, _rel(c, f) / bar(j))
        out[names[diff[k]]] = worst
    print(out)
    assert all(v >= 10.0 for v in out.values()), out
    return out


@pytest.mark.parametrize("E", cases.FUSED_E)
@pytest.mark.parametrize("case", sorted(cases.FUSED))
def test_every_substitution_term_of_the_fused_operator_is_visible(case, E):
    """_SepFctpBwdData.backward: dropping cx, cM or cw moves a second-order gradient by >= 10 x the loosest bar of the GPU test
    (bf16: 3e-2), at every E and with either set of output cotangents it runs"""
    c = cases.Fused(case)
    loosest = max(cases.FUSED_TOL.values())
    for use in ([None, [0]] if c.n2 else [None]):
        _control(c.ref, c.inputs(E), c.names, c.diff_sets()["xMw"], 100 + E, lambda j: loosest, use=use)


@pytest.mark.parametrize("case", sorted(cases.GATED))
def test_every_substitution_term_of_the_gated_operator_is_visible(case):
    c = cases.Gated(case)
    loosest = max(cases.FUSED_TOL[m] for m in ("split", "bf16"))
    for E in cases.FUSED_E:
        _control(c.ref, c.inputs(E), c.names, [0, 1, 2], 200 + E, lambda j: loosest)


@pytest.mark.parametrize("use_w", [True, False])
@pytest.mark.parametrize("case", sorted(cases.DTP))
def test_every_substitution_term_of_the_unfused_product_is_visible(case, use_w):
    """_DtpBwd.backward, bar 2e-5"""
    c = cases.Dtp(case, use_w)
    for E in cases.DTP_E:
        _control(c.ref, c.inputs(E), c.names, c.diff_sets()["xMw"], 300 + E, lambda j: TOL)


@pytest.mark.parametrize("irr", cases.ALN_IRREPS)
def test_both_cotangents_of_add_layer_norm_are_visible(irr):
    ins, lay = cases.aln_problem(irr)
    _control(lambda a, b, w, bias: fo.add_layer_norm(a, b, w, bias, lay), ins, ["a", "b", "weight", "bias"], [0, 1], 400,
             lambda j: TOL)


def test_both_cotangents_of_fold_weight_are_visible():
    W, w, row_start, w_of_row = cases.fold_problem()
    _control(lambda a, b: fo.fold_weight(a, b, row_start, w_of_row), [W, w], ["W", "w"], [0, 1], 500, lambda j: TOL)
