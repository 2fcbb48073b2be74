"""The double backward that equiformer_amd/ops.py COMPOSES by hand -- first-order kernels re-launched with one argument
substituted, partial results accumulated in place -- operator by operator against fp64 autograd of a plain restatement
(tests/fp64_tp.py, tests/fp64_ops.py, tests/second_order_ref.py), in the scheme of tests/test_gpu_second_order.py:

    L = sum_k <b_k, d<a, f(inputs)> / d x_k>   over the inputs x_k of `diff`,

compared: the first derivatives, and d L / d (every differentiable input, a).  `diff` decides which cotangents the double
backward sees and so which of its branches run.  A failing test names the autograd Function whose backward it covers:

    test_sep_fctp_*            _SepFctpBwdData (and the create_graph branch of _SepFctp)
    test_sep_fctp_gated_*      the create_graph branch of _SepFctpGated: re-materialised gate, _GateBwd, _SepFctpBwdData
    test_dtp_*                 _DtpBwd                        test_dtp_coupling_*   _CouplingBwd
    test_irreps_linear_* / test_linear_pair_* / test_dense_linear_*     _LinearDgrad, _LinearWgrad
    test_fold_weight_*         _FoldWeight (ATen index_add branch)
    test_gather_add_*          _GatherAddBwd                  test_segment_scale_*  _SegmentScale
    test_add_layer_norm_*      the create_graph branch of _AddLayerNorm
    test_edge_geometry_*       _EdgeGeomBwd with periodic offsets
    test_guard_*               what is declared first-order-only raises instead of returning a value

tests/test_tp_restatements.py shows on the CPU, for the inputs used here, that removing any single substitution term of
_SepFctpBwdData.backward or _DtpBwd.backward moves a compared quantity by at least 10 x its loosest bar.

Bars (max-abs difference over the largest entry of the fp64 value): fp32-arithmetic operators 2e-5; linears 2e-5 x the
per-mode factor of tests/test_gpu_ops.py::MODE_TOL (fp32 1, split 4); fused SeparableFCTP the per-mode bars of
tests/test_gpu_sfcx.py::TOL (split 1e-4, bf16 3e-2, split6 and exact fp32 5e-6) for every quantity.  (A second-order output that
is the sum of three launches of those kernels could claim three times the bar; the measured errors never come near it, so the
plain bar is applied to the sums as well.)

Worst errors measured on the MI355X, per operator family (profiles/second_order_ops/errors.txt holds every operator, mode and
quantity; this module writes such a file when EQF_SECOND_ORDER_ERRORS names one):
    sep_fctp        fp32 1.1e-6 (L / a1, md17_l3)   split6 6.6e-7   split 1.4e-5 (L / weight, qm9_sep_act)   bf16 5.5e-3 (same)
    sep_fctp_gated  split 8.7e-6 (L / weight)       bf16 5.8e-3 (L / x_raw, E(3) gate)
    linears         fp32 7.2e-7 (d W, irreps_linear)   split 1.4e-5 (L / W, 8x0e+4x1e -> 8x0e+4x1e+4x2e; bar 8e-5)
    dtp, coupling   2.5e-7          fold, gather_add, segment_scale, add_layer_norm   3.6e-7          edge_geometry, periodic   4.9e-7
Wall time of this file on an MI355X, one run each (pytest's figure): 4.9 s at the parent commit, 7.7 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py).
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fp64_ops as fo  # noqa: E402
import fp64_tp as tp  # noqa: E402
import second_order_cases as cases  # noqa: E402
import second_order_ref as so  # noqa: E402
from second_order_ref import TOL, _compare, _dev, _rel  # noqa: E402
from equiformer_amd import ops  # noqa: E402
from equiformer_amd.layout import RowLayout  # noqa: E402
from poison import poisoned_ops  # noqa: E402,F401  (every launch of this file runs on poisoned, guarded allocations)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_ops")]

LIN_TOL = {"fp32": 1.0, "split": 4.0}  # tests/test_gpu_ops.py::MODE_TOL
_worst = {}   # (operator, mode, quantity) -> worst error of this run
_refs = {}    # fp64 results shared between the arithmetic modes of a case
_objs = {}


def _case(cls, *key):
    k = (cls.__name__,) + key
    if k not in _objs:
        _objs[k] = cls(*key)
    return _objs[k]


def _recorder(op, mode, diff_names, wrt_names):
    def rec(kind, k, err):
        q = ("d " + diff_names[k]) if kind == "first" else ("L / " + wrt_names[k])
        key = (op, mode, q)
        _worst[key] = max(_worst.get(key, 0.0), err)
    return rec


# ------------------------------------------------------------------------------------------------- fused SeparableFCTP
def _fused_run(c, op, hip, mode, E, dname, diff, use, seed, gated=False):
    tol = cases.FUSED_TOL[mode]
    ins = c.inputs(E)
    wrt = list(c.names) + (["a1", "a2"] if use is None and getattr(c, "n2", 0) else ["a1"])
    ctx = ops.input_grads_only if dname == "M" else None
    tag = "%s diff=%s%s" % (op, dname, "" if use is None else " out1 only")
    _compare(hip, c.ref, ins, diff, seed, tol=tol, first_ctx=ctx, use=use,
             record=_recorder(tag, mode, [c.names[i] for i in diff], wrt), ref=(_refs, (op, E, dname, str(use))))


@pytest.mark.parametrize("mode", ["fp32", "split", "split6", "bf16"])
@pytest.mark.parametrize("case", sorted(cases.FUSED))
def test_sep_fctp_double_backward(case, mode):
    """_SepFctpBwdData.backward: diff [x, M, w] runs all three substitutions (g_M accumulated in place by two launches, g_W by
    three), [M] alone inside ops.input_grads_only() is what a force pass asks (pos -> sh -> M is the only route), [x] alone the
    third.  With a second consumer: both output cotangents, and out1's alone (d2 is then zero-filled).  wide_l2: the data
    gradient is the exact-fp32 kernel while forward and weight gradient are split-precision (x_mask == 5), so one g_M is
    accumulated across two back ends.  The biases require grad: no second-order term may reach them."""
    c = _case(cases.Fused, case)
    assert c.spec.supported

    def hip(*ins):
        x, M, w, weight, weight2, bias, bias2 = c.split(ins)
        with ops.matrix_mode(mode):
            return ops.sep_fctp(x, M, w, weight, bias, c.spec, weight2, bias2)
    for E in cases.FUSED_E:
        with ops.matrix_mode(mode):
            m = ops._sfc_mode(c.spec, E)
        if mode == "fp32":
            assert m is None
        else:  # a silent fall-through to the exact kernels is not coverage of the split-precision path
            assert m is not None and c.spec.x_mask(m, E) & 1
            if case == "wide_l2":
                assert c.spec.x_mask(m, E) == 5
        for dname, diff in c.diff_sets().items():
            for use in ([None, [0]] if c.n2 else [None]):
                _fused_run(c, "sep_fctp " + case, hip, mode, E, dname, diff, use, 100 + E)


@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("case", sorted(cases.GATED))
def test_sep_fctp_gated_double_backward(case, mode):
    """the create_graph branch of _SepFctpGated.backward: the gate output is re-materialised by the gate operator, the data
    gradient is _SepFctpBwdData on it and _GateBwd takes it back to x_raw; reference: fp64_ops.gate composed with the
    restatement of the fused operator"""
    c = _case(cases.Gated, case)

    def hip(x_raw, M, w, weight, bias):
        with ops.matrix_mode(mode):
            return ops.sep_fctp_gated(x_raw, M, w, weight, bias, c.spec, c.gate)
    for E in cases.FUSED_E:
        with ops.matrix_mode(mode):
            assert ops._sfc_mode(c.spec, E) is not None
            assert ops.sep_fctp_gated_ok(c.spec, c.t["x_raw"].shape[1], c.gate[0], c.gated, E=E)
        for dname, diff in c.diff_sets().items():
            _fused_run(c, "sep_fctp_gated " + case, hip, mode, E, dname, diff, None, 200 + E)


# ------------------------------------------------------------------------------------------------- un-fused product, coupling
@pytest.mark.parametrize("use_w", [True, False], ids=["w", "now"])
@pytest.mark.parametrize("case", sorted(cases.DTP))
def test_dtp_double_backward(case, use_w):
    """_DtpBwd.backward (the forces of the E(3) models go through it): all three substitutions, [M] alone inside
    input_grads_only, [w] alone"""
    c = _case(cases.Dtp, case, use_w)
    for E in cases.DTP_E:
        for dname, diff in c.diff_sets().items():
            ctx = ops.input_grads_only if dname == "M" else None
            wrt = c.names + ["a"]
            _compare(lambda *ins: ops.dtp(ins[0], ins[1], ins[2] if use_w else None, c.table), c.ref, c.inputs(E), diff, 300 + E,
                     first_ctx=ctx, record=_recorder("dtp %s%s diff=%s" % (case, "" if use_w else " no w", dname), "fp32",
                                                     [c.names[i] for i in diff], wrt))


@pytest.mark.parametrize("case", sorted(cases.DTP))
def test_dtp_coupling_double_backward(case):
    """_CouplingBwd: the operator is linear, so d L / d sh is zero and d L / d a is the coupling of b (_coupling_fwd)"""
    c = _case(cases.Dtp, case, True)
    for E in cases.DTP_E:
        sh = c.sh[:E].clone().requires_grad_(True)
        _compare(lambda s: ops.dtp_coupling(s, c.table), lambda s: tp.coupling(c.table, s), [sh], [0], 310 + E,
                 record=_recorder("dtp_coupling " + case, "fp32", ["sh"], ["sh", "a"]))


# ------------------------------------------------------------------------------------------------- linears
FULL, SMALL = "8x0e+4x1e+4x2e", "8x0e+4x1e"  # tests/test_gpu_linear_unified.py
LIN_LAYOUTS = {"same": (FULL, FULL), "down": (FULL, SMALL), "up": (SMALL, FULL)}


def _lin_ref(spec, x, W, b):
    """per pair of the plan: out[seg] = x[seg] . W_pair on every component, bias on the 0e segment, other columns zero"""
    n = x.shape[0]
    out = x.new_zeros(n, spec.out_layout.dim)
    cols = []
    for (l, in_off, K, out_off, N, w_off) in spec.pairs:
        d = 2 * l + 1
        y = x[:, in_off:in_off + d * K].reshape(n, d, K) @ W[w_off:w_off + K * N].view(K, N)
        if b is not None and spec.has_bias(l, out_off):
            y = y + b
        cols.append((out_off, y.reshape(n, d * N)))
    pieces, at = [], 0
    for off, y in sorted(cols, key=lambda q: q[0]):
        if off > at:
            pieces.append(out[:, at:off])
        pieces.append(y)
        at = off + y.shape[1]
    if at < out.shape[1]:
        pieces.append(out[:, at:])
    return torch.cat(pieces, dim=1)


def _lin_problem(spec, rows, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: fo.f32r(torch.randn(*s, generator=g, dtype=torch.float64) * scale).requires_grad_(True)  # noqa: E731
    return r(rows, spec.in_layout.dim), r(spec.weight_numel, scale=0.3), r(spec.bias_dim)


@pytest.mark.parametrize("mode", sorted(LIN_TOL))
@pytest.mark.parametrize("rows", [5, 130])
@pytest.mark.parametrize("layouts", sorted(LIN_LAYOUTS))
def test_irreps_linear_double_backward(layouts, rows, mode):
    """diff [x] inside input_grads_only: _LinearDgrad alone.  diff [x, W, bias] outside it: _LinearWgrad.backward as well
    (g_x = dgrad(dy, c), g_dy = fwd(x, c)) with the torch-made bias gradient beside it.  `down`: the input columns no pair
    reads get an exactly zero gradient in the create_graph path too."""
    li, lo = (RowLayout(s) for s in LIN_LAYOUTS[layouts])
    spec = ops.LinearSpec(li, lo)
    x, W, b = _lin_problem(spec, rows, 320 + rows)
    tol = TOL * LIN_TOL[mode]

    def hip(xx, WW, bb):
        with ops.matrix_mode(mode):
            return ops.irreps_linear(xx, WW, bb, spec)
    for dname, diff, ctx in (("x", [0], ops.input_grads_only), ("xWb", [0, 1, 2], None)):
        with ops.matrix_mode(mode):  # (a linear multiplies in the mode of the moment, in backward too)
            _compare(hip, lambda xx, WW, bb: _lin_ref(spec, xx, WW, bb), [x, W, b], diff, 330, tol=tol, first_ctx=ctx,
                     record=_recorder("irreps_linear %s diff=%s" % (layouts, dname), mode, ["x", "W", "bias"][:len(diff)],
                                      ["x", "W", "bias", "a"]))
    if not spec.in_covered:
        dev = _dev()
        xs, Ws, bs = (t.detach().float().to(dev).requires_grad_(True) for t in (x, W, b))
        a = torch.randn(rows, lo.dim, device=dev).requires_grad_(True)
        read = torch.zeros(li.dim, dtype=torch.bool)
        for (l, in_off, K, _, _, _) in spec.pairs:
            read[in_off:in_off + (2 * l + 1) * K] = True
        with ops.matrix_mode(mode):
            (dx,) = torch.autograd.grad(hip(xs, Ws, bs), xs, a, create_graph=True)
            assert (~read).any() and float(dx.detach()[:, ~read.to(dev)].abs().max()) == 0.0
            (g_a,) = torch.autograd.grad((dx * torch.randn_like(dx)).sum(), a)
        assert torch.isfinite(g_a).all()


@pytest.mark.parametrize("mode", sorted(LIN_TOL))
@pytest.mark.parametrize("rows", [5, 130])
def test_linear_pair_double_backward(rows, mode):
    """two linears of one input in one launch per direction: both members' cotangents, and the second member's alone (the
    first dy is then zero-filled)"""
    li = RowLayout(FULL)
    s1, s2 = ops.LinearSpec(li, RowLayout(FULL)), ops.LinearSpec(li, RowLayout(SMALL))
    x, W1, b1 = _lin_problem(s1, rows, 340 + rows)
    _, W2, b2 = _lin_problem(s2, rows, 341 + rows)
    tol = TOL * LIN_TOL[mode]

    def hip(xx, w1, bb1, w2, bb2):
        with ops.matrix_mode(mode):
            return ops.irreps_linear_pair(xx, w1, bb1, s1, w2, bb2, s2)

    def ref(xx, w1, bb1, w2, bb2):
        return _lin_ref(s1, xx, w1, bb1), _lin_ref(s2, xx, w2, bb2)
    names = ["x", "W1", "b1", "W2", "b2"]
    for use in (None, [1]):
        wrt = names + (["a1", "a2"] if use is None else ["a2"])
        every = [0, 1, 2, 3, 4] if use is None else [0, 3, 4]  # (the first member's parameters are no part of the second's graph)
        for dname, diff, ctx in (("x", [0], ops.input_grads_only), ("all", every, None)):
            with ops.matrix_mode(mode):  # (a linear multiplies in the mode of the moment, in backward too)
                _compare(hip, ref, [x, W1, b1, W2, b2], diff, 350, tol=tol, first_ctx=ctx, use=use,
                         record=_recorder("irreps_linear_pair diff=%s%s" % (dname, "" if use is None else " second only"), mode,
                                          [names[i] for i in diff], wrt))


@pytest.mark.parametrize("mode", sorted(LIN_TOL))
@pytest.mark.parametrize("rows", [5, 130])
@pytest.mark.parametrize("K,N", [(96, 64), (7, 5)])
def test_dense_linear_double_backward(K, N, rows, mode):
    g = torch.Generator().manual_seed(360 + K)
    r = lambda *s, scale=1.0: fo.f32r(torch.randn(*s, generator=g, dtype=torch.float64) * scale).requires_grad_(True)  # noqa: E731
    x, W, b = r(rows, K), r(N, K, scale=K ** -0.5), r(N)

    def hip(xx, WW, bb):
        with ops.matrix_mode(mode):
            return ops.dense_linear(xx, WW, bb)
    for dname, diff, ctx in (("x", [0], ops.input_grads_only), ("xWb", [0, 1, 2], None)):
        with ops.matrix_mode(mode):
            _compare(hip, lambda xx, WW, bb: xx @ WW.t() + bb, [x, W, b], diff, 361, tol=TOL * LIN_TOL[mode], first_ctx=ctx,
                     record=_recorder("dense_linear %dx%d diff=%s" % (K, N, dname), mode, ["x", "W", "bias"][:len(diff)],
                                      ["x", "W", "bias", "a"]))


# ------------------------------------------------------------------------------------------------- the smaller operators
def test_fold_weight_double_backward():
    """_FoldWeight: under create_graph dW is another fold and dw an ATen index_add, where first order is one kernel; both
    must give the fp64 value"""
    W, w, row_start, w_of_row = cases.fold_problem()
    dev = _dev()
    rs_d, wr_d = row_start.to(dev), w_of_row.to(dev)
    _compare(lambda a, c: ops.fold_weight(a, c, rs_d, wr_d), lambda a, c: fo.fold_weight(a, c, row_start, w_of_row), [W, w],
             [0, 1], 500, record=_recorder("fold_weight", "fp32", ["W", "w"], ["W", "w", "a"]))
    # the two branches of the first derivative against each other's reference: the kernel (no graph) as well
    Ws, ws = (t.detach().float().to(dev).requires_grad_(True) for t in (W, w))
    go = fo.f32r(torch.randn(W.shape, generator=torch.Generator().manual_seed(501), dtype=torch.float64))
    want = torch.autograd.grad(fo.fold_weight(W, w, row_start, w_of_row), [W, w], go)
    for create_graph in (False, True):
        got = torch.autograd.grad(ops.fold_weight(Ws, ws, rs_d, wr_d), [Ws, ws], go.float().to(dev), create_graph=create_graph)
        assert _rel(got[0], want[0]) < TOL and _rel(got[1], want[1]) < TOL, create_graph


@pytest.mark.parametrize("with_b", [True, False])
@pytest.mark.parametrize("D", [8, 480])
def test_gather_add_double_backward(D, with_b):
    """_GatherAddBwd on the ragged graph (segment lengths 0 .. 130, sources among the first seven nodes): linear, so d L / d a
    is the gather of the cotangents"""
    graph = fo.ragged_graph(fo.SEG_LENGTHS, 7, 370, device=_dev())
    src, dst = graph.src.cpu(), graph.dst.cpu()
    g = torch.Generator().manual_seed(371)
    ins = [fo.f32r(torch.randn(graph.N, D, generator=g, dtype=torch.float64)).requires_grad_(True) for _ in range(1 + with_b)]
    _compare(lambda *t: ops.gather_add(t[0], t[1] if with_b else None, graph),
             lambda *t: fo.gather_add(t[0], t[1] if with_b else None, src, dst), ins, list(range(len(ins))), 372,
             record=_recorder("gather_add D=%d%s" % (D, "" if with_b else " no b"), "fp32", ["a", "b"], ["a", "b"][:len(ins)] + ["c"]))


def test_segment_scale_double_backward():
    """_SegmentScale is its own backward at every order"""
    dev = _dev()
    ptr = torch.tensor([0] + fo.SEG_LENGTHS).cumsum(0)
    seg_of = fo.seg_of_ptr(ptr).to(torch.int32)
    g = torch.Generator().manual_seed(380)
    x = fo.f32r(torch.randn(int(ptr[-1]), 8, generator=g, dtype=torch.float64)).requires_grad_(True)
    s = fo.f32r(torch.rand(len(fo.SEG_LENGTHS), generator=g, dtype=torch.float64) + 0.5)
    s_d, seg_d = s.float().to(dev), seg_of.to(dev)
    _compare(lambda t: ops.segment_scale(t, s_d, seg_d), lambda t: fo.segment_scale(t, s, seg_of), [x], [0], 381,
             record=_recorder("segment_scale", "fp32", ["x"], ["x", "a"]))


@pytest.mark.parametrize("both", [True, False], ids=["both_outputs", "sum_only"])
@pytest.mark.parametrize("irr", cases.ALN_IRREPS)
def test_add_layer_norm_double_backward(irr, both, monkeypatch):
    """the create_graph branch of _AddLayerNorm.backward (differentiable norm backward + a differentiable add), diff [a, b].
    With only the sum used the normalised branch has no cotangent: the backward is the identity, its second derivative is zero,
    and neither takes a launch."""
    ins, seg = cases.aln_problem(irr)
    lay = cases.op_layout(irr)
    hip = lambda a, b, w, bias: ops.add_layer_norm(a, b, w, bias, lay)  # noqa: E731
    ref = lambda a, b, w, bias: fo.add_layer_norm(a, b, w, bias, seg)[::-1]  # noqa: E731  (the operator returns (sum, y))
    if both:
        _compare(hip, ref, ins, [0, 1], 400, record=_recorder("add_layer_norm " + irr, "fp32", ["a", "b"],
                                                              ["a", "b", "weight", "bias", "a_sum", "a_y"]))
        return
    _compare(hip, ref, ins, [0, 1], 400, use=[0])
    dev = _dev()
    a, b, w, bias = (t.detach().float().to(dev).requires_grad_(True) for t in ins)
    s, _ = hip(a, b, w, bias)
    launches = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *args: (launches.append(name), real(name, *args))[1])
    c = torch.randn_like(s).requires_grad_(True)
    ga, gb = torch.autograd.grad(s, [a, b], c, create_graph=True)
    L = (ga * torch.randn_like(ga)).sum() + (gb * torch.randn_like(gb)).sum()
    second = torch.autograd.grad(L, [a, b, w, c], allow_unused=True)
    assert launches == [], launches
    assert torch.equal(ga, c) and torch.equal(gb, c)
    assert all(t is None for t in second[:3]) and second[3] is not None


@pytest.mark.parametrize("lmax", [1, 3])
def test_edge_geometry_with_offsets_double_backward(lmax):
    """_EdgeGeomBwd on a periodic graph: three cells (one triclinic), atoms [7, 5, 9], edges across the cell faces carry a
    non-zero Cartesian offset that enters vec but not its derivative wrt pos"""
    from types import SimpleNamespace
    from equiformer_amd.graph import EdgeGraph
    dev = _dev()
    g0 = torch.Generator().manual_seed(21)
    cell = torch.tensor([[[6.0, 0.0, 0.0], [1.5, 5.5, 0.0], [0.8, -1.1, 7.0]],
                         [[4.0, 0.0, 0.0], [0.0, 9.0, 0.0], [0.0, 0.0, 12.0]],
                         [[11.0, 0.0, 0.0], [0.0, 11.0, 0.0], [0.0, 0.0, 25.0]]])
    natoms = [7, 5, 9]
    frac = torch.rand(sum(natoms), 3, generator=g0)
    pos = torch.cat([frac[:7] @ cell[0], frac[7:12] @ cell[1], frac[12:] @ cell[2]])
    batch = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(natoms)])
    graph, offsets, _ = EdgeGraph.from_radius_pbc(pos.to(dev), cell.to(dev), batch.to(dev), 5.0)
    assert graph.E > 0 and float(offsets.abs().max()) > 0 and graph.E <= 2048
    off64 = offsets.cpu().double()
    gcpu = SimpleNamespace(src=graph.src.cpu(), dst=graph.dst.cpu())
    assert float((pos[gcpu.src.long()] - pos[gcpu.dst.long()] + offsets.cpu()).norm(dim=1).min()) > 0.1
    p64 = pos.double().requires_grad_(True)

    def hip(p):
        _, length, sh = ops.edge_geometry(p, offsets, graph, lmax)
        return length, sh
    _compare(hip, lambda p: so.edge_geometry(p, off64, gcpu, lmax), [p64], [0], 410,
             record=_recorder("edge_geometry pbc lmax=%d" % lmax, "fp32", ["pos"], ["pos", "a_len", "a_sh"]))


# ------------------------------------------------------------------------------------------------- guards
def _raises_on_differentiation(t, wrt):
    """a loss made of t raises when it is differentiated (ops._Guard, or autograd's once_differentiable error), by
    loss.backward() as a training step does and by autograd.grad wrt the operator's own inputs; it does not return a value"""
    assert t.requires_grad, "handed out as a constant: whatever differentiates it silently loses the term"
    expect = (NotImplementedError, RuntimeError)
    with pytest.raises(expect) as e:
        (t * torch.randn_like(t)).sum().backward(retain_graph=True)
    assert "not implemented" in str(e.value) or "once_differentiable" in str(e.value), str(e.value)
    if wrt:
        with pytest.raises(expect) as e:
            torch.autograd.grad((t * torch.randn_like(t)).sum(), wrt, allow_unused=True)
        assert "not implemented" in str(e.value), str(e.value)


def _fused_small():
    c = _case(cases.Fused, "qm9_sep_value")
    dev = _dev()
    return c, [t.detach().float().to(dev).requires_grad_(True) for t in c.inputs(37)]


@pytest.mark.parametrize("constant_cotangent", [False, True])
def test_guard_sep_fctp_weight_gradient(constant_cotangent):
    """the weight gradient a create_graph backward of sep_fctp returns is a first-order result: differentiating through it raises.
    It is bilinear in the cotangent and the data inputs, so it is guarded when EITHER is part of a graph -- with a constant
    cotangent and a differentiable x it used to come back as a constant (ops._guard looked at the cotangent only)."""
    c, ins = _fused_small()
    x, M, w, weight, weight2, bias, bias2 = c.split(ins)
    out = ops.sep_fctp(x, M, w, weight, bias, c.spec, weight2, bias2)
    a = torch.randn_like(out)
    if not constant_cotangent:
        a.requires_grad_(True)
    dx, gW = torch.autograd.grad(out, [x, weight], a, create_graph=True)
    assert dx.requires_grad
    _raises_on_differentiation(gW, [x, M])


def test_guard_sep_fctp_weight_gradient_is_a_constant_only_when_it_is_one():
    """nothing differentiable in sight (constant cotangent, data inputs that do not require grad): the plain tensor"""
    c, ins = _fused_small()
    x, M, w, weight, weight2, bias, bias2 = c.split(ins)
    out = ops.sep_fctp(x.detach(), M.detach(), None, weight, bias, c.spec)
    (gW,) = torch.autograd.grad(out, [weight], torch.randn_like(out), create_graph=True)
    assert not gW.requires_grad


def test_guard_graph_norm():
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.synthetic import qm9_like_batch
    dev = _dev()
    d = qm9_like_batch(3, 6, side=4.0, seed=2)
    graph = EdgeGraph.from_radius(d["pos"].to(dev), d["batch"].to(dev), 5.0)
    lay = RowLayout("8x0e+4x1e+2x2e")  # (a layout of tests/test_gpu_graph_norm.py)
    g = torch.Generator().manual_seed(420)
    r = lambda *s: torch.randn(*s, generator=g).to(dev).requires_grad_(True)  # noqa: E731
    x, ms, w, b = r(graph.N, lay.dim), r(8), r(14), r(8)
    y = ops.graph_norm(x, ms, w, b, lay, graph)
    for a in (torch.randn_like(y).requires_grad_(True), torch.randn_like(y)):
        (dx,) = torch.autograd.grad(y, x, a, create_graph=True)
        _raises_on_differentiation(dx, [x])


def test_guard_alpha_dot_gradient():
    from equiformer_amd import so3
    dev = _dev()
    g = torch.Generator().manual_seed(421)
    a = torch.randn(9, 4 * 32, generator=g).to(dev).requires_grad_(True)
    ad = torch.randn(4 * 32, generator=g).to(dev).requires_grad_(True)
    logit = ops.alpha_logits(a, ad, 4, 32, so3.C_SMOOTH_LEAKY_RELU_02)
    for c in (torch.randn_like(logit).requires_grad_(True), torch.randn_like(logit)):
        da, dd = torch.autograd.grad(logit, [a, ad], c, create_graph=True)
        _raises_on_differentiation(dd, [a])


def test_guard_dtp_linear():
    """dtp_linear is first-order only: its backward is once_differentiable"""
    from equiformer_amd.layout import DtpTable
    dev = _dev()
    irr, sh = "128x0e+64x1e+32x2e", "1x0e+1x1e+1x2e"  # (tests/test_gpu_ops.py runs the operator on this layout)
    table, lay = DtpTable(irr, sh, irr), RowLayout(irr)
    spec = ops.DtpLinearSpec.make(table, lay)
    assert spec is not None
    g = torch.Generator().manual_seed(422)
    r = lambda *s: torch.randn(*s, generator=g).to(dev).requires_grad_(True)  # noqa: E731
    E = 37
    x, M, w = r(E, table.layout_in.dim), r(E, table.m_numel), r(E, table.weight_numel)
    weight, bias = r(spec.weight_numel), r(spec.bias_dim)
    out = ops.dtp_linear(x, M, w, weight, bias, spec)
    (dx,) = torch.autograd.grad(out, x, torch.randn_like(out).requires_grad_(True), create_graph=True)
    # (autograd's marker sits between dx and the cotangent only: it fires in loss.backward(), which walks to every leaf, not
    # in an autograd.grad that asks for the derivative wrt x alone -- that one reports x as unused)
    _raises_on_differentiation(dx, None)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(dx.sum(), [x])


# ------------------------------------------------------------------------------------------------- the measured errors
def test_zz_report_measured_errors():
    """(last in the file) every comparison above recorded its error before asserting; with EQF_SECOND_ORDER_ERRORS=<file> the
    worst per operator, mode and quantity are written there -- profiles/second_order_ops/errors.txt is such a file"""
    path = os.environ.get("EQF_SECOND_ORDER_ERRORS")
    lines = ["%-58s %-7s %-14s %.2e" % (op, mode, q, v) for (op, mode, q), v in sorted(_worst.items())]
    if path:
        with open(path, "w") as f:
            f.write("# worst |hip - fp64| / max |fp64| per operator, arithmetic mode and compared quantity\n")
            f.write("# (d x: first derivative wrt x;  L / x: gradient of L = sum <b, d<a, f>/d .> wrt x)\n")
            f.write("\n".join(lines) + "\n")
    assert all(v == v for v in _worst.values())
