"""The row, segment and attention HIP kernels (csrc/rowops.hip, csrc/edge.hip) against the float64 restatements of
tests/fp64_ops.py at ragged edges: mixed in-degrees around the wavefront, every launch shape of the attention kernels, the
fallback kernels that the comfortable shapes of tests/test_gpu_ops.py never launch, row counts around every chunk size.

Metric: `fp64_ops.per_row_rel` -- the error of a row (of a segment of a row for the layer norm) over the largest
reference entry of THAT row, floored at 1e-3 of the tensor's largest entry; nothing is skipped.  Every test compares the
forward and every gradient.  Bounds are those tests/test_gpu_ops.py states for the operator, now per row.  Where plain
fp32 arithmetic cannot meet such a bound on an input family (cancellation: near one-hot softmax rows, a mean much larger
than the spread, sums of many signed terms) the bound is max(project bound, 4 x the error of the SAME restatement
evaluated in float32 on the CPU on the same inputs), computed here from the reference alone; the factor 4 covers
__expf and another summation order.  Every test prints "FIG <case> <quantity> err=... yard=... bound=..." lines
(pytest -rA or -s shows them): err is the kernel's figure, yard the float32 restatement's.

Measured on an MI355X: the worst case of each quantity (largest err / bound), err = the kernel, yard = the float32
restatement on the same inputs ("-": plain bound), from the FIG lines of one run:
  attention       out 6.1e-7, alpha 6.9e-7, d_value 7.2e-7 (bound 1e-5); d_logit 8.7e-5, yard 3.3e-5 -> bound 1.3e-4
                  (G = 54, "+80"); the yardstick of d_logit reaches 4.7e-5 on plain "randn" logits (G = 65)
  with dropout    out 5.7e-7, d_value 6.6e-7; d_logit 8.7e-6, yard 1.1e-5 -> 4.4e-5
  "peak" logits   out and d_value: yard 0 and 2e-23, the plain bounds hold
  alpha logits    logit 2.3e-6 (5e-6), d_a 3.1e-7 (3e-5); d_alpha_dot 2.7e-5, yard 1.2e-5 -> 4.8e-5 (H = 3, Kh = 32)
  layer norm      randn+100: y 5.7e-6, yard 4.3e-6 -> 1.7e-5; dx 1.1e-5, yard 7.9e-6 -> 3.2e-5; d_weight 9.6e-6, yard
                  5.3e-6 -> 2.1e-5; d_bias 3.3e-7 (2e-5); the other families stay under the plain bounds
  add + LN        xsum 4.5e-8 (2e-7); randn+100: y 5.3e-6, yard 2.0e-6 -> 8.1e-6; da = db 1.7e-5, yard 6.8e-6 -> 2.7e-5;
                  d_weight 7.9e-6, yard 5.4e-6 -> 2.2e-5
  gate            y 1.4e-7 (3e-6), dx 3.9e-6 (5e-6)
  SiLU            y 6.8e-7 (2e-6), dx 3.1e-6 (5e-6)
  LN + SiLU       y 1.1e-6 (5e-6); dx 1.7e-5, yard 4.1e-6 (C = 3: plain bound 2e-5); d_gamma 4.4e-7, d_beta 2.0e-7
  embedding       y 5.9e-8 (1e-6), dW 1.1e-7, db 2.4e-7 (1e-5)
  fold weight     out 3.9e-8, dW 4.2e-8, dw 1.3e-7 (yard 7.5e-7; 3e-6)
  segments        sum 5.8e-7, yard 5.8e-7 -> 2.3e-6 (D = 1); broadcast exact; gather msg 5.9e-8, da 2.2e-7, db 3.1e-7
Wall time of this file on an MI355X, one run each (pytest's figure): 5.8 s at the parent commit, 6.8 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py).
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ops as fo  # noqa: E402
from poison import poisoned_ops  # noqa: E402,F401  (every launch of this file runs on poisoned, guarded allocations)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_ops")]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class _Layout:
    """What the operators need of a row layout (segments, the C descriptor, the row length); RowLayout refuses rows with
    two 0e segments, the C ABI does not."""

    def __init__(self, irreps):
        import ctypes
        from equiformer_amd import lib
        seg = fo.Segs(irreps)
        self.segs, self.par, self.offsets, self.dim = seg.segs, seg.par, seg.offsets, seg.dim
        self.c = lib.make_irreps(self.segs, self.par)
        self.c_ref = ctypes.byref(self.c)


def _layout(seg):
    from equiformer_amd.layout import RowLayout
    irr = "+".join("%dx%d%s" % (mul, l, "e" if p == 1 else "o") for (mul, l), p in zip(seg.segs, seg.par))
    try:
        return RowLayout(irr)
    except NotImplementedError:
        return _Layout(irr)


def _randn(shape, seed, scale=1.0):
    return fo.f32r(torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale)


class _Checker:
    """collects every comparison of a test, prints its figures and fails at the end, so that one run shows them all"""

    def __init__(self, case):
        self.case, self.bad, self.worst = case, [], {}

    def cmp(self, name, got, ref, bound, y32=None, slices=None):
        assert got is not None and torch.isfinite(got).all(), (self.case, name, "not finite")
        err = fo.per_row_rel(got, ref, slices=slices)
        yard = fo.per_row_rel(y32, ref, slices=slices) if y32 is not None else None
        lim = bound if yard is None else max(bound, 4.0 * yard)
        w = self.worst.get(name)
        if w is None or err / lim > w[0] / w[2]:
            self.worst[name] = (err, yard, lim)
        if not err < lim:
            self.bad.append((name, err, yard, lim))

    def done(self):
        for name, (err, yard, lim) in self.worst.items():
            print("FIG %s %s err=%.2e yard=%s bound=%.2e" % (self.case, name, err,
                                                              "-" if yard is None else "%.2e" % yard, lim))
        assert not self.bad, (self.case, self.bad)


def _run(ck, names, hip_fn, ref_fn, inputs, gouts, bounds, use_yard=(), slices=None, wrt=None):
    """outputs and gradients of hip_fn (float32, GPU) against ref_fn (float64, CPU); names / bounds / slices are per
    compared tensor, outputs first, then the gradients wrt the floating inputs (or `wrt`); use_yard: the names whose
    bound takes the float32 yardstick"""
    ro, rg, yo, yg = fo.yardstick(ref_fn, inputs, gouts, wrt=wrt)
    ho, hg = fo.evaluate(hip_fn, inputs, gouts, torch.float32, device=_dev(), wrt=wrt)
    slices = slices or {}
    for name, h, r, y in zip(names, ho + hg, ro + rg, yo + yg):
        ck.cmp(name, h, r, bounds[name], y if name in use_yard else None, slices.get(name))
    return ho, hg, ro, rg


# ------------------------------------------------------------------------------------------------- attention
# Dispatch (csrc/edge.hip, attn_aggregate_{fwd,bwd}_impl): G <= 32 float4 groups per head -> attn_{fwd,bwd}_half_kernel,
# else attn_{fwd,bwd}_kernel with slot s = group lane + 64 s.  fo.ATTN_HEADS gives G = 30, 32 (half), 54 (full, slot 0),
# 65 (lane 0 of slot 1), 120 (slots 0-1), 256 (slots 0-3 full) and H = 16 (1024 threads).  fo.ATTN_DEGREES puts degrees
# 0..9 (the `e0 += 4` / half-wave tails), 62..69 (shuffle -> re-read hand-over at edge 64 of a row) and 127..130 in ONE
# launch, so the forward and the backward of both kernels run on rows longer than a wavefront.
ATTN_BOUNDS = {"out": 1e-5, "alpha": 1e-5, "d_logit": 3e-5, "d_value": 1e-5}


def _attn_setup(head_irr, H, seed):
    dev = _dev()
    graph = fo.ragged_graph(fo.ATTN_DEGREES, 9, seed, device=dev)
    seg = fo.all_heads_layout(head_irr, H)
    lay = _layout(seg)
    row_ptr = graph.row_ptr.cpu()
    assert (row_ptr[1:] - row_ptr[:-1]).tolist() == fo.ATTN_DEGREES
    return graph, seg, lay, row_ptr


@pytest.mark.parametrize("regime", ["randn", "+80", "-80", "peak"])
@pytest.mark.parametrize("head_irr,H", fo.ATTN_HEADS)
def test_attention_ragged(head_irr, H, regime):
    """out, the saved softmax (read through d_value with d_out = 1), d_logit and d_value on the ragged graph.
    d_logit = alpha (da - sum alpha da) cancels inside every row (the float32 restatement itself misses 3e-5 per row on
    plain "randn" logits: 4.7e-5 at G = 65), so its bound takes the float32 yardstick in every regime.  out, alpha and
    d_value use the plain bounds in "randn", "+80" and "-80" (the max subtraction makes the shifted ones as good as
    "randn"); "peak" (one logit 60 above the rest, a near one-hot softmax) takes the yardstick throughout.
    Yardstick values: see the head of this file."""
    from equiformer_amd import ops
    graph, seg, lay, row_ptr = _attn_setup(head_irr, H, 40)
    E = graph.E
    logit = fo.attn_logits(regime, E, H, row_ptr, 41)
    value = _randn((E, seg.dim), 42)
    go = _randn((graph.N, seg.dim), 43)
    ck = _Checker("attn[%s,H=%d,G=%d,%s]" % (head_irr, H, fo.head_groups(head_irr), regime))
    yard = ("out", "d_logit", "d_value") if regime == "peak" else ("d_logit",)

    def hip(lg, v):
        return ops.attn_aggregate(lg, v, graph, H, lay, 0.0, 0)

    def ref(lg, v):
        return fo.attn_aggregate(lg, v, row_ptr, H, seg)[0]

    _run(ck, ["out", "d_logit", "d_value"], hip, ref, [logit, value], [go], ATTN_BOUNDS, yard)
    # the softmax the forward saved: with d_out = 1, d_value[e, any column of head h] = alpha[e, h]
    ones = torch.ones(graph.N, seg.dim, dtype=torch.float64)
    _, hg = fo.evaluate(hip, [logit, value], [ones], torch.float32, device=_dev(), wrt=[1])
    alpha_ref = fo.segment_softmax(logit, row_ptr)
    hoc = fo.head_of_column(seg, H)
    ck.cmp("alpha", hg[0], alpha_ref[:, hoc], ATTN_BOUNDS["alpha"])
    ck.done()


@pytest.mark.parametrize("head_irr,H", [fo.ATTN_HEADS[0], fo.ATTN_HEADS[2], fo.ATTN_HEADS[4]])
def test_attention_dropout_ragged(head_irr, H):
    """p = 0.25 on the ragged graph.  d_value = alpha * keep * d_out is linear, so the keep mask is read back from it:
    every entry is 0 or 1 / (1 - p), the kept share is inside the binomial 4 sigma band, and `out` and `d_logit` match the
    fp64 reference evaluated with THAT mask -- which pins the (e H + h) mask index across the two half-wave edges of a
    step, the full kernel and rows longer than a wavefront (forward and backward must regenerate the same mask)."""
    from equiformer_amd import ops
    graph, seg, lay, row_ptr = _attn_setup(head_irr, H, 44)
    E, p = graph.E, 0.25
    logit = fo.attn_logits("randn", E, H, row_ptr, 45)
    value = _randn((E, seg.dim), 46)
    go = _randn((graph.N, seg.dim), 47)
    ck = _Checker("attn_drop[%s,H=%d]" % (head_irr, H))

    def hip(lg, v):
        return ops.attn_aggregate(lg, v, graph, H, lay, p, 1234)

    ones = torch.ones(graph.N, seg.dim, dtype=torch.float64)
    _, hg = fo.evaluate(hip, [logit, value], [ones], torch.float32, device=_dev(), wrt=[1])
    alpha_ref = fo.segment_softmax(logit, row_ptr)
    hoc = fo.head_of_column(seg, H)
    first_col = torch.tensor([int((hoc == h).nonzero()[0]) for h in range(H)])
    ak = hg[0].double().cpu()
    assert float((ak - ak[:, first_col][:, hoc]).abs().max()) == 0.0  # one factor per (edge, head)
    m = ak[:, first_col] / alpha_ref
    kept = (m - 1.0 / (1.0 - p)).abs() < 1e-4
    assert bool((kept | (m.abs() < 1e-4)).all()), "mask entries other than 0 and 1 / (1 - p)"
    share, n = float(kept.double().mean()), E * H
    assert abs(share - (1.0 - p)) < 4.0 * math.sqrt(p * (1.0 - p) / n), (share, n)
    keep = kept.double() / (1.0 - p)

    def ref(lg, v):
        return fo.attn_aggregate(lg, v, row_ptr, H, seg, keep)[0]

    _run(ck, ["out", "d_logit", "d_value"], hip, ref, [logit, value], [go], ATTN_BOUNDS, ("d_logit",))
    ck.done()


# ------------------------------------------------------------------------------------------------- alpha logits
# Dispatch (eqf_alpha_bwd): alpha_bwd4_kernel needs H Kh <= 256 and 256 % (H Kh / 4) == 0.  (3,32): 256 % 24, (5,16):
# 256 % 20, (6,32): 256 % 48 fail that, (16,32) and (8,64) have H Kh = 512 -> all five take alpha_bwd_kernel, the fallback
# (CH = 16 edges per workgroup: E = 15, 16, 17 and 130 straddle it); (2,8) and (4,32) take alpha_bwd4_kernel (64 edges per
# workgroup: E = 63, 64, 65).
@pytest.mark.parametrize("H,Kh", [(3, 32), (5, 16), (6, 32), (16, 32), (8, 64), (2, 8), (4, 32)])
def test_alpha_logits_edges(H, Kh):
    """logit, d_a and d_alpha_dot.  d_alpha_dot is an atomic sum of signed terms over the edges, compared per element: its
    bound takes the float32 yardstick.  alpha_bwd_kernel forms the 16 products of a thread in fp64: as a serial fp32 chain
    it gave 6.0e-5 at H = 3, Kh = 32 against a bound of 4.8e-5 (yard 1.2e-5); now 2.7e-5."""
    from equiformer_amd import ops, so3
    ck = _Checker("alpha[H=%d,Kh=%d]" % (H, Kh))
    bounds = {"logit": 5e-6, "d_a": 3e-5, "d_alpha_dot": 3e-5}
    for E in (1, 15, 16, 17, 63, 64, 65, 130):
        a = _randn((E, H * Kh), 50 + E, 2.0)
        a[:, ::7] = 0.0                     # exact zeros; randn gives both signs
        adot = _randn((H * Kh,), 51)
        go = _randn((E, H), 52 + E)
        _run(ck, ["logit", "d_a", "d_alpha_dot"],
             lambda x, d: ops.alpha_logits(x, d, H, Kh, so3.C_SMOOTH_LEAKY_RELU_02),
             lambda x, d: fo.alpha_logits(x, d, H, Kh), [a, adot], [go], bounds, ("d_alpha_dot",),
             slices={"d_alpha_dot": [slice(i, i + 1) for i in range(H * Kh)]})
    ck.done()


# ------------------------------------------------------------------------------------------------- layer norm
LN_ROWS = (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 130)  # around WAVES_PER_BLOCK = 4, LN_WGRAD_CHUNK = 16, LN_WGRAD_ROWS = 64
LN_BOUNDS = {"y": 5e-6, "xsum": 2e-7, "dx": 2e-5, "da": 2e-5, "db": 2e-5, "d_weight": 2e-5, "d_bias": 2e-5}
# families whose 0e segments cancel (mean >> spread; a constant segment is ZERO after the mean subtraction and then
# multiplied by 1 / sqrt(eps)): float32 yardstick
LN_YARD = {"randn+100": ("y", "dx", "da", "db", "d_weight", "d_bias"),
           "zero-and-constant": ("y", "dx", "da", "db", "d_weight", "d_bias")}


def _ln_params(seg):
    nw = sum(mul for mul, _ in seg.segs)
    nb = sum(mul for s, (mul, _) in enumerate(seg.segs) if seg.scalar(s))
    wsl, off = [], 0
    for mul, _ in seg.segs:
        wsl.append(slice(off, off + mul))
        off += mul
    return _randn((nw,), 60) * 0.5 + 1.0, _randn((nb,), 61), wsl


@pytest.mark.parametrize("family", fo.LN_FAMILIES)
@pytest.mark.parametrize("irr", fo.LN_IRREPS)
def test_layer_norm_edges(irr, family):
    """y, dx per (row, segment), d_weight per segment, d_bias -- also for 64x0e+32x1e+16x0e, whose second 0e segment used
    to get the FIRST segment's mean in the weight gradient (a wrong d_weight with status 0)."""
    from equiformer_amd import ops
    seg = fo.Segs(irr)
    lay = _layout(seg)
    w, b, wsl = _ln_params(seg)
    ck = _Checker("ln[%s,%s]" % (irr, family))
    sl = {"y": seg.slices(), "dx": seg.slices(), "d_weight": wsl, "d_bias": [slice(None)]}
    for rows in LN_ROWS:
        x = fo.ln_input(family, rows, seg, 62 + rows)
        go = _randn((rows, seg.dim), 63 + rows)
        _run(ck, ["y", "dx", "d_weight", "d_bias"],
             lambda t, ww, bb: ops.layer_norm(t, ww, bb, lay, 1e-5),
             lambda t, ww, bb: fo.layer_norm(t, ww, bb, seg, 1e-5), [x, w, b], [go], LN_BOUNDS,
             LN_YARD.get(family, ()), slices=sl)
    ck.done()


@pytest.mark.parametrize("family", fo.LN_FAMILIES)
@pytest.mark.parametrize("irr", fo.LN_IRREPS)
def test_add_layer_norm_edges(irr, family):
    """(xsum, y) = (a + b, LN(a + b)) with a gradient flowing into xsum as well (the `dres` path of the backward)."""
    from equiformer_amd import ops
    seg = fo.Segs(irr)
    lay = _layout(seg)
    w, b, wsl = _ln_params(seg)
    ck = _Checker("add_ln[%s,%s]" % (irr, family))
    sl = {"y": seg.slices(), "xsum": seg.slices(), "da": seg.slices(), "db": seg.slices(), "d_weight": wsl,
          "d_bias": [slice(None)]}
    for rows in LN_ROWS:
        x = fo.ln_input(family, rows, seg, 64 + rows)
        a1 = fo.f32r(0.25 * x)
        a2 = fo.f32r(x - a1)                 # zero rows stay zero, the constant 1.5 stays constant
        gy, gs = _randn((rows, seg.dim), 65 + rows), _randn((rows, seg.dim), 66 + rows)

        def hip(p, q, ww, bb):
            s, y = ops.add_layer_norm(p, q, ww, bb, lay, 1e-5)
            return y, s

        _run(ck, ["y", "xsum", "da", "db", "d_weight", "d_bias"], hip,
             lambda p, q, ww, bb: fo.add_layer_norm(p, q, ww, bb, seg, 1e-5), [a1, a2, w, b], [gy, gs], LN_BOUNDS,
             LN_YARD.get(family, ()), slices=sl)
    ck.done()


# ------------------------------------------------------------------------------------------------- gate, SiLU, LN + SiLU
@pytest.mark.parametrize("irr", ["128x0e+64x1e+32x2e", "384x0e+192x1e+192x2e+96x3e", "8x0e+4x1e+4x2e+4x3e"])
def test_gate_edges(irr):
    """rows around the 8-row blocks of the column kernels, Din and Dout above and below 256 columns, inputs scaled by 30 so
    that the sigmoids saturate on both sides"""
    from equiformer_amd import ops, so3
    full = fo.Segs(irr)
    S = full.segs[0][0]
    gseg = fo.Segs([(mul, l, p) for (mul, l), p in zip(full.segs[1:], full.par[1:])])
    G = sum(mul for mul, _ in gseg.segs)
    glay = _layout(gseg)
    ck = _Checker("gate[%s]" % irr)
    for rows in (1, 7, 8, 9, 203):
        x = _randn((rows, S + G + gseg.dim), 70 + rows, 30.0)
        go = _randn((rows, S + gseg.dim), 71 + rows)
        _run(ck, ["y", "dx"], lambda t: ops.gate(t, S, glay, so3.C_SILU, so3.C_SIGMOID),
             lambda t: fo.gate(t, S, gseg, so3.C_SILU, so3.C_SIGMOID), [x], [go], {"y": 3e-6, "dx": 5e-6})
    ck.done()


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, 1024, 1025])
def test_scaled_silu_edges(n):
    """the float4 body and the scalar tail (n % 4 != 0), as (n,) and (n, 1); per element, values in +-30"""
    from equiformer_amd import ops, so3
    ck = _Checker("silu[n=%d]" % n)
    g = torch.Generator().manual_seed(72 + n)
    for shape in ((n,), (n, 1)):
        x = fo.f32r((torch.rand(shape, generator=g, dtype=torch.float64) * 2.0 - 1.0) * 30.0)
        go = _randn(shape, 73 + n)
        _run(ck, ["y", "dx"], lambda t: ops.scaled_silu(t, so3.C_SILU), lambda t: fo.scaled_silu(t, so3.C_SILU), [x], [go],
             {"y": 2e-6, "dx": 5e-6})
    ck.done()


# Dispatch (eqf_lnsilu_group_bwd): C % 4 == 0 -> lnsilu_bwd4_kernel, else lnsilu_bwd_kernel (C = 1, 3, 30, 50).
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("C", [1, 3, 30, 50, 4, 32, 64])
def test_ln_silu_edges(C, groups):
    """y, dx, d_gamma, d_beta.  A row of few channels whose values lie close together is the layer norm's ill-conditioned
    input (the float32 restatement itself reaches 3.3e-5 on dx at C = 3): y and dx take the float32 yardstick."""
    from equiformer_amd import ops
    ck = _Checker("lnsilu[C=%d,groups=%d]" % (C, groups))
    gam, bet = _randn((C * groups,), 74) * 0.5 + 1.0, _randn((C * groups,), 75)
    bounds = {"y": 5e-6, "dx": 2e-5, "d_gamma": 2e-5, "d_beta": 2e-5}
    for rows in (1, 3, 31, 32, 33, 65, 257):
        x = _randn((rows, C * groups), 76 + rows, 1.3)
        go = _randn((rows, C * groups), 77 + rows)
        _run(ck, ["y", "dx", "d_gamma", "d_beta"], lambda t, ga, be: ops.ln_silu(t, ga, be, 1e-5, groups),
             lambda t, ga, be: fo.ln_silu(t, ga, be, 1e-5, groups), [x, gam, bet], [go], bounds, ("y", "dx"),
             slices={"d_gamma": [slice(None)], "d_beta": [slice(None)]})
    ck.done()


# ------------------------------------------------------------------------------------------------- embedding
# embed_bwd_kernel: 64-row chunks (blockIdx.y), an LDS table of EMB_SLOTS = 16 types per chunk that is flushed when a
# chunk shows a 17th type, 256 columns per workgroup (blockIdx.x > 0 from C = 512 on).
@pytest.mark.parametrize("irr", ["128x0e+64x1e+32x2e", "512x0e"])
def test_embedding_edges(irr):
    from equiformer_amd import ops
    seg = fo.Segs(irr)
    C, D, T = seg.segs[0][0], seg.dim, 40
    W, b = _randn((T, C), 80), _randn((C,), 81)
    present = torch.arange(0, T, 1)[torch.arange(T) % 4 != 3]  # 30 of the 40 types occur
    ck = _Checker("embed[%s]" % irr)
    for rows in (200, 1, 63, 64, 65):
        g = torch.Generator().manual_seed(82 + rows)
        z = present[torch.randint(0, present.numel(), (rows,), generator=g)]
        for c0 in range(0, rows - 63, 64):
            assert z[c0:c0 + 64].unique().numel() > 16  # every full chunk overflows the slot table
        go = _randn((rows, D), 83 + rows)
        zi = z.to(torch.int32)
        _, hg, _, rg = _run(ck, ["y", "dW", "db"], lambda t, ww, bb: ops.embed(t, ww, bb, D),
                            lambda t, ww, bb: fo.embedding(t, ww, bb, D), [zi, W, b], [go],
                            {"y": 1e-6, "dW": 1e-5, "db": 1e-5}, slices={"db": [slice(None)]})
        absent = torch.ones(T, dtype=torch.bool)
        absent[z] = False
        assert absent.any() and float(hg[0].cpu()[absent].abs().max()) == 0.0  # types that never occur: exactly zero
    ck.done()


# ------------------------------------------------------------------------------------------------- fold weight
def test_fold_weight_edges():
    """row lengths around the 64-lane stride; one shared weight per row (w_of_row a permutation: the kernel's contract).
    dw is a dot product of signed terms, compared per element: float32 yardstick."""
    from equiformer_amd import ops
    dev = _dev()
    lens = [1, 2, 63, 64, 65, 200, 1]
    row_start = torch.tensor([0] + lens).cumsum(0).to(torch.int32)
    w_of_row = torch.randperm(len(lens), generator=torch.Generator().manual_seed(84)).to(torch.int32)
    n = int(row_start[-1])
    W, w, go = _randn((n,), 85), _randn((len(lens),), 86), _randn((n,), 87)
    rs_d, wr_d = row_start.to(dev), w_of_row.to(dev)
    ck = _Checker("fold")
    rows = [slice(int(row_start[r]), int(row_start[r + 1])) for r in range(len(lens))]
    _run(ck, ["out", "dW", "dw"], lambda a, c: ops.fold_weight(a, c, rs_d, wr_d).reshape(1, -1),
         lambda a, c: fo.fold_weight(a, c, row_start, w_of_row).reshape(1, -1), [W, w], [go.reshape(1, -1)],
         {"out": 2e-6, "dW": 3e-6, "dw": 3e-6}, ("dw",),
         slices={"out": rows, "dW": rows, "dw": [slice(i, i + 1) for i in range(len(lens))]})
    ck.done()


# ------------------------------------------------------------------------------------------------- segments
# segment_sum_kernel: D % 4 == 0 -> float4 columns, four rows per step (tails at lengths 1, 3, 5, 9), else one column per
# thread (D = 1, 6).  Sums of signed terms: float32 yardstick.
SEG_BOUNDS = {"out": 2e-6, "dx": 3e-6, "d_go": 3e-6, "msg": 2e-6, "da": 3e-6, "db": 3e-6}


@pytest.mark.parametrize("D", [1, 6, 480])
def test_segment_sum_and_broadcast_edges(D):
    """segment_sum with a scale over segment lengths 0, 1, 3, 4, 5, 8, 9, 0, 130, 0; its gradient (the broadcast kernel);
    and the broadcast as an operator of its own (the create_graph backward) with ITS gradient"""
    from equiformer_amd import ops
    dev = _dev()
    ptr = torch.tensor([0] + fo.SEG_LENGTHS).cumsum(0).to(torch.int32)
    seg_of = fo.seg_of_ptr(ptr).to(torch.int32)
    n, nseg = int(ptr[-1]), len(fo.SEG_LENGTHS)
    ptr_d, seg_d = ptr.to(dev), seg_of.to(dev)
    x, go, c = _randn((n, D), 90), _randn((nseg, D), 91), _randn((n, D), 92)
    ck = _Checker("segsum[D=%d]" % D)
    _run(ck, ["out", "dx"], lambda t: ops.segment_sum(t, ptr_d, seg_d, nseg, 0.25),
         lambda t: fo.segment_sum(t, ptr, 0.25), [x], [go], SEG_BOUNDS, ("out",))

    def hip_bcast(t, g):
        (dx,) = torch.autograd.grad(ops.segment_sum(t, ptr_d, seg_d, nseg, 0.25), [t], g, create_graph=True)
        return dx

    def ref_bcast(t, g):
        return fo.segment_bcast(g, seg_of, 0.25) + 0.0 * t

    _run(ck, ["dx", "d_go"], hip_bcast, ref_bcast, [x, go], [c], SEG_BOUNDS, ("d_go",), wrt=[1])
    ck.done()


@pytest.mark.parametrize("D", [8, 480])
def test_gather_add_and_segment_scale_edges(D):
    """gather_add with and without b on a ragged graph with repeated sources and nodes that are nobody's source: its
    backward is segment_sum through the by-source permutation (da) and over the rows (db); segment_scale with its gradient"""
    from equiformer_amd import ops
    dev = _dev()
    graph = fo.ragged_graph(fo.SEG_LENGTHS, 7, 93, device=dev)
    src, dst = graph.src.cpu(), graph.dst.cpu()
    a, b, go = _randn((graph.N, D), 94), _randn((graph.N, D), 95), _randn((graph.E, D), 96)
    ck = _Checker("gather[D=%d]" % D)
    _run(ck, ["msg", "da", "db"], lambda p, q: ops.gather_add(p, q, graph), lambda p, q: fo.gather_add(p, q, src, dst),
         [a, b], [go], SEG_BOUNDS, ("da", "db"))
    _run(ck, ["msg", "da"], lambda p: ops.gather_add(p, None, graph), lambda p: fo.gather_add(p, None, src, dst),
         [a], [go], SEG_BOUNDS, ("da",))
    s = _randn((graph.N,), 97)
    s[3] = 0.0
    s_d = s.float().to(dev)
    _run(ck, ["out", "dx"], lambda t: ops.segment_scale(t, s_d, graph.dst), lambda t: fo.segment_scale(t, s, dst),
         [go], [_randn((graph.E, D), 98)], SEG_BOUNDS)
    ck.done()


@pytest.mark.parametrize("D", [1, 6])
def test_float4_only_operators_refuse_other_widths(D):
    """gather_add and segment_scale move float4 columns: a width that is no multiple of 4 is refused by status, before
    any launch"""
    from equiformer_amd import lib, ops
    dev = _dev()
    graph = fo.ragged_graph(fo.SEG_LENGTHS, 7, 93, device=dev)
    a = torch.zeros(graph.N, D, device=dev)
    with pytest.raises(lib.HipLibraryError, match="code -2"):
        ops.gather_add(a, None, graph)
    with pytest.raises(lib.HipLibraryError, match="code -2"):
        ops.segment_scale(torch.zeros(graph.E, D, device=dev), torch.ones(graph.N, device=dev), graph.dst)
