"""Every second-derivative HIP kernel (`eqf_*_bwd2`, equiformer_amd/csrc/second.hip) against the double backward of the
fp64 restatement of the same operator (tests/second_order_ref.py, itself pinned against the oracle modules by
tests/test_second_order_restatements.py).

For an operator y = f(x; theta):  L = <b, d<a, f(x; theta)> / d x>  is a scalar whose gradient wrt x, theta and a is
what `loss.backward()` asks of the operator when forces were taken with create_graph=True
[ref: nets/graph_attention_transformer_md17.py:318-325].  The HIP path gets there through
`torch.autograd.grad(..., create_graph=True)` on the ops.* autograd Functions; the reference value is the same
expression on the restatement in fp64 on the CPU.  Tolerance 2e-5 of the largest entry (fp32 kernels, sums over rows).
Wall time of this file on an MI355X, one run each (pytest's figure): 3.6 s at the parent commit, 3.5 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import second_order_ref as so  # noqa: E402
from second_order_ref import TOL, _compare, _dev, _rel, _second_order  # noqa: E402,F401  (the comparison scheme)
from poison import poisoned_ops  # noqa: E402,F401  (every launch of this file runs on poisoned, guarded allocations)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_ops")]


def _rows(n, d, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, d, generator=g, dtype=torch.float64) * scale).requires_grad_(True)


def test_scaled_silu_bwd2():
    from equiformer_amd import ops, so3
    x = _rows(37, 96, 1, 2.0)
    _compare(lambda t: ops.scaled_silu(t, so3.C_SILU), lambda t: so.scaled_silu(t, so3.C_SILU), [x], [0], 2)


@pytest.mark.parametrize("irr", ["24x0e+16x1e+8x2e", "384x0e+192x1e+96x2e", "64x0e+32x1e+32x2e+16x3e"])
def test_gate_bwd2(irr):
    from equiformer_amd import ops, so3
    from equiformer_amd.layout import RowLayout
    from oracle import e3
    from oracle import nets as onets
    scalars, gates, gated = onets.irreps2gate(e3.Irreps(irr))
    lay_gated = RowLayout(gated)
    Din = scalars.dim + gates.dim + gated.dim
    x = _rows(29, Din, 3, 1.5)
    S = scalars.dim
    _compare(lambda t: ops.gate(t, S, lay_gated, so3.C_SILU, so3.C_SIGMOID),
             lambda t: so.gate(t, S, lay_gated, so3.C_SILU, so3.C_SIGMOID), [x], [0], 4)


@pytest.mark.parametrize("C", [64, 32])
def test_lnsilu_bwd2(C):
    from equiformer_amd import ops
    g = torch.Generator().manual_seed(5)
    x = _rows(301, C, 6, 1.3)
    gamma = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    _compare(lambda t, ga, be: ops.ln_silu(t, ga, be, 1e-5), lambda t, ga, be: so.ln_silu(t, ga, be, 1e-5),
             [x, gamma, beta], [0], 7)


@pytest.mark.parametrize("C,G", [(64, 7), (32, 3)])
def test_lnsilu_group_bwd2(C, G):
    """the radial bank's LayerNorm + SiLU: G feature vectors side by side in a row, each with its own gamma / beta
    (eqf_lnsilu_group_bwd2, round 5) against the per-group restatement"""
    from equiformer_amd import ops
    g = torch.Generator().manual_seed(15)
    x = _rows(203, C * G, 16, 1.3)
    gamma = (torch.rand(C * G, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = torch.randn(C * G, generator=g, dtype=torch.float64).requires_grad_(True)

    def ref(t, ga, be):
        return torch.cat([so.ln_silu(t[:, k * C:(k + 1) * C], ga[k * C:(k + 1) * C], be[k * C:(k + 1) * C], 1e-5)
                          for k in range(G)], dim=1)
    _compare(lambda t, ga, be: ops.ln_silu(t, ga, be, 1e-5, groups=G), ref, [x, gamma, beta], [0], 17)


@pytest.mark.parametrize("wide", [True, False])
def test_grouped_linear_second_order(wide):
    """G nn.Linear layers on the column blocks of one input in one launch (the radial bank's second and third layers):
    differentiable grouped pieces under create_graph (ops._GroupedDgrad / _GroupedWgrad, round 5)"""
    from equiformer_amd import ops
    G, K = 5, 64
    Ns = [64] * G if wide else [96, 64, 128, 64, 32]
    g = torch.Generator().manual_seed(25)
    x = _rows(157, G * K, 26, 0.7)
    Ws = [(torch.randn(n, K, generator=g, dtype=torch.float64) * 0.2).requires_grad_(True) for n in Ns]
    bs = [torch.randn(n, generator=g, dtype=torch.float64).requires_grad_(True) for n in Ns]

    def hip(t, *p):
        return ops.grouped_linear(t, K, list(p[:G]), list(p[G:]), wide)

    def ref(t, *p):
        outs = [t[:, k * K:(k + 1) * K] @ p[k].t() + p[G + k] for k in range(G)]
        return torch.cat(outs, dim=1) if wide else tuple(outs)
    _compare(hip, ref, [x] + Ws + bs, [0], 27)


@pytest.mark.parametrize("irr", ["128x0e+64x1e+32x2e", "128x0e+64x1e+64x2e+32x3e", "32x0e+16x1e"])
def test_layernorm_bwd2(irr):
    from equiformer_amd import ops
    from equiformer_amd.layout import RowLayout
    lay = RowLayout(irr)
    g = torch.Generator().manual_seed(8)
    nw = sum(m for m, _ in lay.segs)
    nb = sum(m for m, l in lay.segs if l == 0)
    x = _rows(43, lay.dim, 9)
    w = (torch.rand(nw, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    b = torch.randn(nb, generator=g, dtype=torch.float64).requires_grad_(True)
    _compare(lambda t, ww, bb: ops.layer_norm(t, ww, bb, lay, 1e-5), lambda t, ww, bb: so.layer_norm(t, ww, bb, lay, 1e-5),
             [x, w, b], [0], 10)


@pytest.mark.parametrize("H,Kh", [(4, 32), (8, 32), (4, 16)])
def test_alpha_bwd2(H, Kh):
    from equiformer_amd import ops, so3
    g = torch.Generator().manual_seed(11)
    a = _rows(211, H * Kh, 12, 1.5)
    ad = torch.randn(H * Kh, generator=g, dtype=torch.float64).requires_grad_(True)
    c = so3.C_SMOOTH_LEAKY_RELU_02
    _compare(lambda t, d: ops.alpha_logits(t, d, H, Kh, c), lambda t, d: so.alpha_logits(t, d, H, Kh, c), [a, ad], [0], 13)


@pytest.mark.parametrize("head_irr,H", [("32x0e+16x1e+8x2e", 4), ("32x0e+16x1e+16x2e+8x3e", 4), ("32x0e+16x1e", 8)])
def test_attn_aggregate_bwd2(head_irr, H):
    from equiformer_amd import ops
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.irreps import Irreps
    from equiformer_amd.layout import RowLayout
    from equiformer_amd.synthetic import qm9_like_batch
    dev = _dev()
    d = qm9_like_batch(5, 14, side=4.0, seed=4)
    graph = EdgeGraph.from_radius(d["pos"].to(dev), d["batch"].to(dev), 5.0)
    lay = RowLayout(" + ".join("%dx%de" % (mul * H, ir.l) for mul, ir in Irreps(head_irr)))
    E = graph.E
    g = torch.Generator().manual_seed(14)
    logit = (torch.randn(E, H, generator=g, dtype=torch.float64) * 2.0).requires_grad_(True)
    value = torch.randn(E, lay.dim, generator=g, dtype=torch.float64).requires_grad_(True)
    from types import SimpleNamespace
    gcpu = SimpleNamespace(dst=graph.dst.cpu(), N=graph.N)
    _compare(lambda lo, va: ops.attn_aggregate(lo, va, graph, H, lay), lambda lo, va: so.attn_aggregate(lo, va, gcpu, H, lay),
             [logit, value], [0, 1], 15)


@pytest.mark.parametrize("head_irr,H", [("32x0e+16x1e+8x2e", 4), ("32x0e+16x1e+16x2e+8x3e", 4)])
def test_attn_aggregate_bwd2_ragged(head_irr, H):
    """eqf_attn_aggregate_bwd2 on ragged rows: in-degrees 0..9, 62..69 and 127..130 with empty rows first and last, for the
    heads of 30 float4 groups (half-wave first-order kernels) and 54 (full kernels)"""
    from types import SimpleNamespace
    from equiformer_amd import ops
    from equiformer_amd.irreps import Irreps
    from equiformer_amd.layout import RowLayout
    import fp64_ops as fo
    graph = fo.ragged_graph(fo.ATTN_DEGREES, 9, 30, device=_dev())
    lay = RowLayout(" + ".join("%dx%de" % (mul * H, ir.l) for mul, ir in Irreps(head_irr)))
    g = torch.Generator().manual_seed(31)
    logit = (torch.randn(graph.E, H, generator=g, dtype=torch.float64) * 2.0).requires_grad_(True)
    value = torch.randn(graph.E, lay.dim, generator=g, dtype=torch.float64).requires_grad_(True)
    gcpu = SimpleNamespace(dst=graph.dst.cpu(), N=graph.N)
    _compare(lambda lo, va: ops.attn_aggregate(lo, va, graph, H, lay), lambda lo, va: so.attn_aggregate(lo, va, gcpu, H, lay),
             [logit, value], [0, 1], 32)


def test_attn_aggregate_bwd2_with_dropout_is_consistent():
    """With alpha_drop > 0 there is no restatement to compare with (the mask is a hash of the seed); the second-order
    kernel must agree with finite differences of the first-order backward under the SAME seed."""
    from equiformer_amd import ops
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.layout import RowLayout
    from equiformer_amd.synthetic import qm9_like_batch
    dev = _dev()
    d = qm9_like_batch(3, 10, side=4.0, seed=5)
    graph = EdgeGraph.from_radius(d["pos"].to(dev), d["batch"].to(dev), 5.0)
    H, lay = 4, RowLayout("128x0e+64x1e")
    E = graph.E
    g = torch.Generator().manual_seed(16)
    logit = torch.randn(E, H, generator=g).to(dev).requires_grad_(True)
    value = torch.randn(E, lay.dim, generator=g).to(dev).requires_grad_(True)
    a = torch.randn(graph.N, lay.dim, generator=g).to(dev)
    bl = torch.randn(E, H, generator=g).to(dev)
    bv = torch.randn(E, lay.dim, generator=g).to(dev)

    def first(lo, va):
        out = ops.attn_aggregate(lo, va, graph, H, lay, 0.25, 1234)
        return torch.autograd.grad(out, [lo, va], a, create_graph=True)

    gl, gv = first(logit, value)
    L = (bl * gl).sum() + (bv * gv).sum()
    s_lo, s_va = torch.autograd.grad(L, [logit, value])
    # directional finite differences of L along random directions
    for which, s in ((0, s_lo), (1, s_va)):
        v = torch.randn(s.shape, generator=g).to(dev)
        eps = 1e-2
        vals = []
        for sgn in (1.0, -1.0):
            lo = (logit + sgn * eps * v).detach().requires_grad_(True) if which == 0 else logit.detach().requires_grad_(True)
            va = (value + sgn * eps * v).detach().requires_grad_(True) if which == 1 else value.detach().requires_grad_(True)
            g1, g2 = first(lo, va)
            vals.append(((bl * g1).sum() + (bv * g2).sum()).item())
        fd = (vals[0] - vals[1]) / (2 * eps)
        an = (s * v).sum().item()
        assert abs(fd - an) < 2e-2 * max(1.0, abs(an)), (which, fd, an)


def test_rbf_expnorm_bwd2():
    from equiformer_amd import ops
    from equiformer_amd.nets.layers import ExpNormalSmearing
    rbf = ExpNormalSmearing(cutoff_lower=0.0, cutoff_upper=5.0, num_rbf=32, trainable=False)
    g = torch.Generator().manual_seed(17)
    length = (torch.rand(257, generator=g, dtype=torch.float64) * 5.5 + 0.3).requires_grad_(True)
    means, betas = rbf.means.double(), rbf.betas.double()
    dev = _dev()
    _compare(lambda t: ops.rbf_expnorm(t, means.float().to(dev), betas.float().to(dev), rbf.alpha, 5.0),
             lambda t: so.rbf_expnorm(t, means, betas, rbf.alpha, 5.0), [length], [0], 18)


def test_rbf_gaussian_bwd2():
    from equiformer_amd import ops
    g = torch.Generator().manual_seed(19)
    R = 128
    length = (torch.rand(193, generator=g, dtype=torch.float64) * 4.5 + 0.4).requires_grad_(True)
    mean = torch.rand(1, R, generator=g, dtype=torch.float64).requires_grad_(True)
    std = (torch.rand(1, R, generator=g, dtype=torch.float64) * 0.9 + 0.1).requires_grad_(True)
    weight = torch.tensor([[1.1]], dtype=torch.float64).requires_grad_(True)
    bias = torch.tensor([[0.05]], dtype=torch.float64).requires_grad_(True)

    def ref(le, mu, sd, w, b):  # [ref: nets/gaussian_rbf.py:6-40]
        x = w * (le / 5.0).unsqueeze(-1) + b
        s = sd.abs() + 1e-5
        return torch.exp(-0.5 * ((x - mu) / s) ** 2) / ((2 * 3.14159) ** 0.5 * s)

    _compare(lambda le, mu, sd, w, b: ops.rbf_gaussian(le, mu, sd, w, b, 5.0), ref, [length, mean, std, weight, bias], [0], 20)


def test_rbf_bessel_fwd_bwd_bwd2():
    """Spherical Bessel basis (ocpmodels RadialBasis, restated in oracle/nets.py) : values, first and second derivatives
    wrt the edge length, the trainable frequencies and the output cotangent."""
    from equiformer_amd import ops
    from oracle import nets as onets
    ref = onets.RadialBasis(16, cutoff=5.0, rbf={"name": "spherical_bessel"}).double()
    g = torch.Generator().manual_seed(23)
    length = (torch.rand(211, generator=g, dtype=torch.float64) * 5.4 + 0.5).requires_grad_(True)  # some beyond the cutoff
    freq = (ref.rbf.frequencies.detach().double() * (1.0 + 0.01 * torch.randn(16, generator=g, dtype=torch.float64))).requires_grad_(True)

    def fref(le, fr):
        x = le / 5.0
        env = 1 + ref.a * x ** 5 + ref.b * x ** 6 + ref.c * x ** 7
        env = torch.where(x < 1, env, torch.zeros_like(x))
        return env[:, None] * (ref.rbf.norm_const / x[:, None] * torch.sin(fr * x[:, None]))

    with torch.no_grad():  # the closed form above IS the module
        assert (fref(length, ref.rbf.frequencies.double()) - ref(length)).abs().max() < 1e-12
    _compare(lambda le, fr: ops.rbf_bessel(le, fr, 5.0), fref, [length, freq], [0], 24)
    # first-order gradient wrt the frequencies (a parameter: no second derivative through it, that raises by design)
    dev = _dev()
    le, fr = length.detach().float().to(dev).requires_grad_(True), freq.detach().float().to(dev).requires_grad_(True)
    go = torch.randn(211, 16, generator=g, dtype=torch.float64)
    g_hip = torch.autograd.grad(ops.rbf_bessel(le, fr, 5.0), [le, fr], go.float().to(dev))
    g_ref = torch.autograd.grad(fref(length, freq), [length, freq], go)
    for x, r in zip(g_hip, g_ref):
        assert _rel(x, r) < TOL


@pytest.mark.parametrize("lmax", [1, 2, 3])
def test_edge_geometry_bwd2(lmax):
    from types import SimpleNamespace
    from equiformer_amd import ops
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.synthetic import qm9_like_batch
    dev = _dev()
    d = qm9_like_batch(4, 9, side=4.0, seed=6)
    graph = EdgeGraph.from_radius(d["pos"].to(dev), d["batch"].to(dev), 5.0)
    gcpu = SimpleNamespace(src=graph.src.cpu(), dst=graph.dst.cpu())
    pos = d["pos"].double().requires_grad_(True)

    def hip(p):
        _, length, sh = ops.edge_geometry(p, None, graph, lmax)
        return length, sh

    _compare(hip, lambda p: so.edge_geometry(p, None, gcpu, lmax), [pos], [0], 21)


# ------------------------------------------------------------------------------------------------- ragged shapes
# The shapes at which tests/test_gpu_op_edges.py pins the first-order twins, plus those csrc/second.hip itself branches on.
# Same scheme, same TOL.  Every shape is one the operator accepts; where first order refuses a layout, the refusal is asserted
# and eqf_*_bwd2 is not launched.
def _f32(t):
    return t.float().double()


def _randn64(shape, seed, scale=1.0):
    return _f32(torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale)


@pytest.mark.parametrize("n", [1, 5, 1023, 1025])
def test_scaled_silu_bwd2_ragged(n):
    """one element, and either side of a multiple of the 256-thread block"""
    from equiformer_amd import ops, so3
    import fp64_ops as fo
    x = _randn64((n, 1), 40 + n, 2.0).requires_grad_(True)
    _compare(lambda t: ops.scaled_silu(t, so3.C_SILU), lambda t: fo.scaled_silu(t, so3.C_SILU), [x], [0], 41)


GATES_RAGGED = {  # (S, gated irreps)
    "tiny": (8, "4x1e+4x2e+4x3e"),                      # Din = 80: far below one 256-thread column block
    "wide": (384, "192x1e+192x2e+96x3e"),               # Din = 3072 gates included: column blocks with a partial last one
    "e3_gated_0o": (16, "8x0o+8x1e+4x1o+4x2e"),         # tests/test_gpu_e3.py: the 0o segment is gated, not activated
}


@pytest.mark.parametrize("rows", [1, 5, 9])
@pytest.mark.parametrize("case", sorted(GATES_RAGGED))
def test_gate_bwd2_ragged(case, rows):
    """rows either side of the RB rows a thread of gate_bwd2_kernel walks (4; the first-order kernels: 8)"""
    from equiformer_amd import ops, so3
    from equiformer_amd.layout import RowLayout
    import fp64_ops as fo
    S, gated = GATES_RAGGED[case]
    lay = RowLayout(gated)
    Din = S + sum(m for m, _ in lay.segs) + lay.dim
    x = _randn64((rows, Din), 42, 1.5).requires_grad_(True)
    _compare(lambda t: ops.gate(t, S, lay, so3.C_SILU, so3.C_SIGMOID),
             lambda t: fo.gate(t, S, lay, so3.C_SILU, so3.C_SIGMOID), [x], [0], 43)


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("C", [1, 3, 30, 50, 64])
def test_lnsilu_bwd2_ragged(C, G, rows):
    """C < 64 leaves inactive lanes in every wave reduction of lnsilu_bwd2_kernel; C = 1 makes the variance exactly zero (every
    derivative wrt x and gamma is then exactly zero, on both sides).
    Inputs: a ramp over the channels of a group (-1.5 .. 1.5) plus 0.4 randn, so that no group is nearly constant.  The second
    derivative grows like rstd^3, and three plain randn values can lie arbitrarily close together: the first draw of this test
    (1.3 randn, C = 3, G = 3, 5 rows) held a group of variance 1.1e-3, on which the SAME restatement evaluated in float32 on the
    CPU is off by 1.2e-5 (1e-7 to 8e-7 on the other shapes) and the kernel by 6.8e-5 -- the conditioning of a three-value
    LayerNorm in float32, not the lanes this test is about."""
    from equiformer_amd import ops
    import fp64_ops as fo
    g = torch.Generator().manual_seed(44)
    ramp = torch.linspace(-1.5, 1.5, C, dtype=torch.float64).repeat(G) if C > 1 else torch.zeros(G, dtype=torch.float64)
    x = _f32(_randn64((rows, C * G), 45, 0.4) + ramp).requires_grad_(True)
    gamma = _f32(torch.rand(C * G, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    beta = _f32(torch.randn(C * G, generator=g, dtype=torch.float64)).requires_grad_(True)
    _compare(lambda t, ga, be: ops.ln_silu(t, ga, be, 1e-5, groups=G), lambda t, ga, be: fo.ln_silu(t, ga, be, 1e-5, groups=G),
             [x, gamma, beta], [0], 46)


def _ln_problem(irr, rows, seed):
    import fp64_ops as fo
    import second_order_cases as cases
    seg = fo.Segs(irr)
    g = torch.Generator().manual_seed(seed)
    nw = sum(m for m, _ in seg.segs)
    nb = sum(m for s, (m, _) in enumerate(seg.segs) if seg.scalar(s))
    x = _randn64((rows, seg.dim), seed + 1).requires_grad_(True)
    w = _f32(torch.rand(nw, generator=g, dtype=torch.float64) + 0.5).requires_grad_(True)
    b = _f32(torch.randn(nb, generator=g, dtype=torch.float64)).requires_grad_(True)
    return seg, cases.op_layout(irr), x, w, b


@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("irr", ["8x0e+4x1e", "64x0e+32x1e+16x0e", "16x0e+8x0o+8x1e+4x1o+4x2e"])
def test_layernorm_bwd2_ragged(irr, rows):
    """segments shorter than a wave, two scalar segments, a 0o segment (the l = -1 branch of make_segtab2: no mean, no bias);
    1 and 5 rows: a partial workgroup of WPB = 4 waves"""
    from equiformer_amd import ops
    import fp64_ops as fo
    seg, lay, x, w, b = _ln_problem(irr, rows, 47)
    _compare(lambda t, ww, bb: ops.layer_norm(t, ww, bb, lay, 1e-5), lambda t, ww, bb: fo.layer_norm(t, ww, bb, seg, 1e-5),
             [x, w, b], [0], 48)


def test_layernorm_bwd2_more_affine_weights_than_the_lds_accumulator():
    """1056 affine weights > GW_S = 1024: layernorm_bwd2_kernel adds straight into g_w (via_lds == false).  First order runs on
    the layout first; were it to refuse it, that refusal is the result and the second-order kernel is not launched."""
    from equiformer_amd import lib, ops
    import fp64_ops as fo
    seg, lay, x, w, b = _ln_problem("1024x0e+32x1e", 3, 49)
    dev = _dev()
    xs, ws, bs = (t.detach().float().to(dev).requires_grad_(True) for t in (x, w, b))
    try:
        y = ops.layer_norm(xs, ws, bs, lay, 1e-5)
        torch.autograd.grad(y.sum(), [xs, ws, bs])
        torch.cuda.synchronize()
    except lib.HipLibraryError:
        with pytest.raises(lib.HipLibraryError):
            ops.layer_norm(xs, ws, bs, lay, 1e-5)
        return
    _compare(lambda t, ww, bb: ops.layer_norm(t, ww, bb, lay, 1e-5), lambda t, ww, bb: fo.layer_norm(t, ww, bb, seg, 1e-5),
             [x, w, b], [0], 50)


@pytest.mark.parametrize("E", [1, 9, 67])
@pytest.mark.parametrize("H,Kh", [(3, 32), (5, 16), (6, 32), (16, 32), (8, 64), (2, 8)])
def test_alpha_bwd2_ragged(H, Kh, E):
    """the (H, Kh) of test_alpha_logits_edges: H Kh no multiple of the 256-thread block, heads of 8 to 64 lanes; E = 1, 9 and 67:
    below, just above and many times the CH = 8 edges a thread of alpha_bwd2_kernel walks"""
    from equiformer_amd import ops, so3
    import fp64_ops as fo
    a = _randn64((E, H * Kh), 51, 1.5).requires_grad_(True)
    ad = _randn64((H * Kh,), 52).requires_grad_(True)
    c = so3.C_SMOOTH_LEAKY_RELU_02
    _compare(lambda t, d: ops.alpha_logits(t, d, H, Kh, c), lambda t, d: fo.alpha_logits(t, d, H, Kh, c), [a, ad], [0], 53)


def _lengths(E, cutoff, seed):
    """edge lengths over (0.3, cutoff + 0.5), with values within 1e-3 below the cutoff and values beyond it in fixed places
    (not AT it: the indicator is discontinuous there)"""
    g = torch.Generator().manual_seed(seed)
    le = torch.rand(E, generator=g, dtype=torch.float64) * (cutoff + 0.2) + 0.3
    special = torch.tensor([cutoff - 1e-3, cutoff + 1e-3, cutoff - 3e-4, cutoff + 0.4], dtype=torch.float64)
    if E > 1:
        n = min(E - 1, special.numel())
        le[1:1 + n] = special[:n]
    return _f32(le).requires_grad_(True)


@pytest.mark.parametrize("E", [1, 5, 65])
def test_rbf_expnorm_bwd2_ragged(E):
    """one wave per edge, four edges per block"""
    from equiformer_amd import ops
    from equiformer_amd.nets.layers import ExpNormalSmearing
    rbf = ExpNormalSmearing(cutoff_lower=0.0, cutoff_upper=5.0, num_rbf=32, trainable=False)
    means, betas = rbf.means.double(), rbf.betas.double()
    dev = _dev()
    _compare(lambda t: ops.rbf_expnorm(t, means.float().to(dev), betas.float().to(dev), rbf.alpha, 5.0),
             lambda t: so.rbf_expnorm(t, means, betas, rbf.alpha, 5.0), [_lengths(E, 5.0, 54)], [0], 55)


@pytest.mark.parametrize("E", [1, 65])
@pytest.mark.parametrize("R", [1, 50, 256])
def test_rbf_gaussian_bwd2_ragged(R, E):
    """R = 1, 50, 256: one lane, a partial wave, the kernel's limit (R > 256 is refused); E either side of the CH = 64 edges a
    block of the parameter kernel reduces"""
    from equiformer_amd import ops
    g = torch.Generator().manual_seed(56)
    mean = _f32(torch.rand(1, R, generator=g, dtype=torch.float64)).requires_grad_(True)
    std = _f32(torch.rand(1, R, generator=g, dtype=torch.float64) * 0.9 + 0.1).requires_grad_(True)
    weight = _f32(torch.tensor([[1.1]], dtype=torch.float64)).requires_grad_(True)
    bias = _f32(torch.tensor([[0.05]], dtype=torch.float64)).requires_grad_(True)

    def ref(le, mu, sd, w, b):  # [ref: nets/gaussian_rbf.py:6-40]
        x = w * (le / 5.0).unsqueeze(-1) + b
        s = sd.abs() + 1e-5
        return torch.exp(-0.5 * ((x - mu) / s) ** 2) / ((2 * 3.14159) ** 0.5 * s)

    _compare(lambda le, mu, sd, w, b: ops.rbf_gaussian(le, mu, sd, w, b, 5.0), ref,
             [_lengths(E, 5.0, 57), mean, std, weight, bias], [0], 58)


def test_rbf_gaussian_refuses_more_than_256_basis_functions():
    """the first-order backward already does (its forward is element-wise and has no limit), with or without create_graph:
    nothing reaches eqf_rbf_gaussian_bwd2 with R > 256"""
    from equiformer_amd import lib, ops
    dev = _dev()
    z = lambda *s: torch.rand(*s, device=dev) + 0.1  # noqa: E731
    for create_graph in (False, True):
        le = z(3).requires_grad_(True)
        out = ops.rbf_gaussian(le, z(1, 257), z(1, 257), z(1, 1), z(1, 1), 5.0)
        with pytest.raises(lib.HipLibraryError):
            torch.autograd.grad(out.sum(), le, create_graph=create_graph)


@pytest.mark.parametrize("E", [1, 65])
def test_rbf_bessel_bwd2_ragged(E):
    """E either side of the EPB = 64 edges of a block"""
    from equiformer_amd import ops
    from oracle import nets as onets
    ref = onets.RadialBasis(16, cutoff=5.0, rbf={"name": "spherical_bessel"}).double()
    freq = _f32(ref.rbf.frequencies.detach().double() * (1.0 + 0.01 * _randn64((16,), 59))).requires_grad_(True)

    def fref(le, fr):
        x = le / 5.0
        env = 1 + ref.a * x ** 5 + ref.b * x ** 6 + ref.c * x ** 7
        env = torch.where(x < 1, env, torch.zeros_like(x))
        return env[:, None] * (ref.rbf.norm_const / x[:, None] * torch.sin(fr * x[:, None]))

    _compare(lambda le, fr: ops.rbf_bessel(le, fr, 5.0), fref, [_lengths(E, 5.0, 60), freq], [0], 61)


@pytest.mark.parametrize("which", ["one_edge", "ragged"])
@pytest.mark.parametrize("lmax", [1, 2, 3])
def test_edge_geometry_bwd2_ragged(lmax, which):
    """a graph of one edge, and a ragged one: the in-degrees of fo.SEG_LENGTHS (0 .. 130), sources among the first seven nodes,
    so that three nodes are nobody's source and get an exactly zero source sum.  fo.ragged_graph itself draws self-loops
    (four with this seed): edges of length zero, where the spherical harmonics have no derivative -- a source equal to its
    destination is moved to the next of the seven."""
    from types import SimpleNamespace
    from equiformer_amd import ops
    from equiformer_amd.graph import EdgeGraph
    import fp64_ops as fo
    dev = _dev()
    if which == "one_edge":
        graph, _ = EdgeGraph.from_edges(torch.tensor([2]).to(dev), torch.tensor([0]).to(dev), 3)
    else:
        g = torch.Generator().manual_seed(62)
        dst = torch.repeat_interleave(torch.arange(len(fo.SEG_LENGTHS)), torch.tensor(fo.SEG_LENGTHS))
        src = torch.randint(0, 7, (dst.numel(),), generator=g)
        src = torch.where(src == dst, (src + 1) % 7, src)
        shuffle = torch.randperm(dst.numel(), generator=g)
        graph, _ = EdgeGraph.from_edges(src[shuffle].to(dev), dst[shuffle].to(dev), len(fo.SEG_LENGTHS))
        assert int((graph.src == graph.dst).sum()) == 0
    gcpu = SimpleNamespace(src=graph.src.cpu(), dst=graph.dst.cpu())
    pos = _randn64((graph.N, 3), 63, 2.0).requires_grad_(True)

    def hip(p):
        _, length, sh = ops.edge_geometry(p, None, graph, lmax)
        return length, sh

    _compare(hip, lambda p: so.edge_geometry(p, None, gcpu, lmax), [pos], [0], 64)
