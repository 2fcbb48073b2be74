"""The edge-row and node-row kernels whose loads were taken out of their dependent chains (csrc/edge.hip: attn_bwd_half_kernel,
gather_add_rows_kernel, alpha_fwd_kernel; csrc/rowops.hip: layernorm_{fwd,bwd}_reg_kernel, lnsilu_fwd_kernel) against the float64 restatements of
tests/fp64_ops.py, on poisoned, guarded allocations (tests/poison.py), at the smallest shapes at which the new loops can go
wrong.  Bounds, checker and runner are those of tests/test_gpu_op_edges.py, imported, not copied.

Constants the shapes are derived from:
  attention backward   one destination row per wave, 4 edges per step (two per half-wave), the next step's value rows requested
                       one step ahead, alpha and d(alpha) of the row's first 64 edges in lane registers, memory stash from the
                       65th edge on; half-wave kernels up to G = 32 float4 groups per head, full-wave kernels above
  gather_add           GATHER_ROWS = 4 edges per wave, GATHER_WAVES = 4 waves per workgroup (16 edges), rows of at least
                       GATHER_ROW_MIN_D4 = 32 float4 columns; narrower rows keep the float4-per-thread kernel
  layer norm           WAVES_PER_BLOCK = 4 rows per workgroup; register kernels for rows of at most LN_REG_SEGS = 4 segments of at
                       most 64 * LN_REG_K = 256 entries, the segment-by-segment kernels otherwise
  LN + SiLU forward    LNSILU_ROWS = 4 rows per wave, 4 waves per workgroup (16 rows)
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ops as fo  # noqa: E402
import test_gpu_op_edges as oe  # noqa: E402  (bounds, _Checker, _run, _layout, _randn: stated once, there)
from poison import guard_input, poisoned_ops  # noqa: E402,F401

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_ops")]

# 0, 1..5 (the 4-edge step and its tail), 7, 8, 9 (two steps: the prefetch distance), 63, 64, 65 (the 64-lane register
# hand-over), 130 (two wavefronts of stash); an empty row first, last and between two long rows
ROW_DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 130, 0, 65, 0]
# (per-head irreps, heads): the QM9 value layout with 8 heads (G = 15), G = 32 (the half-wave limit), G = 33 (full-wave kernels)
ROW_HEADS = [("16x0e+8x1e+4x2e", 8), ("128x0e", 2), ("132x0e", 1)]


def _graph(seed):
    graph = fo.ragged_graph(ROW_DEGREES, 5, seed, device=oe._dev())
    row_ptr = graph.row_ptr.cpu()
    assert (row_ptr[1:] - row_ptr[:-1]).tolist() == ROW_DEGREES
    return graph, row_ptr


@pytest.mark.parametrize("head_irr,H", ROW_HEADS)
def test_attention_rows(head_irr, H):
    """out, alpha (read through d_value with d_out = 1), d_logit, d_value without dropout; bounds of test_attention_ragged"""
    from equiformer_amd import ops
    graph, row_ptr = _graph(140)
    seg = fo.all_heads_layout(head_irr, H)
    lay = oe._layout(seg)
    E = graph.E
    logit = fo.attn_logits("randn", E, H, row_ptr, 141)
    value = oe._randn((E, seg.dim), 142)
    go = oe._randn((graph.N, seg.dim), 143)
    ck = oe._Checker("rows_attn[%s,H=%d,G=%d]" % (head_irr, H, fo.head_groups(head_irr)))

    def hip(lg, v):
        return ops.attn_aggregate(lg, v, graph, H, lay, 0.0, 0)

    oe._run(ck, ["out", "d_logit", "d_value"], hip, lambda lg, v: fo.attn_aggregate(lg, v, row_ptr, H, seg)[0],
            [logit, value], [go], oe.ATTN_BOUNDS, ("d_logit",))
    ones = torch.ones(graph.N, seg.dim, dtype=torch.float64)
    _, hg = fo.evaluate(hip, [logit, value], [ones], torch.float32, device=oe._dev(), wrt=[1])
    ck.cmp("alpha", hg[0], fo.segment_softmax(logit, row_ptr)[:, fo.head_of_column(seg, H)], oe.ATTN_BOUNDS["alpha"])
    ck.done()


@pytest.mark.parametrize("head_irr,H", ROW_HEADS)
def test_attention_rows_dropout_device_seed(head_irr, H):
    """drop_p = 0.2 through the _dseed entry points with a non-zero device word: the mask is read back from d_value (d_out = 1:
    every entry 0 or 1 / (1 - p) times alpha), then out, d_logit and d_value must match the restatement WITH THAT MASK -- forward
    and backward regenerate the same (e H + h) mask across both half-wave edges of a step and beyond the 64th edge"""
    from equiformer_amd import ops
    graph, row_ptr = _graph(144)
    seg = fo.all_heads_layout(head_irr, H)
    lay = oe._layout(seg)
    E, p = graph.E, 0.2
    logit = fo.attn_logits("randn", E, H, row_ptr, 145)
    value = oe._randn((E, seg.dim), 146)
    go = oe._randn((graph.N, seg.dim), 147)
    word = torch.tensor([0x1234567], dtype=torch.int64, device=oe._dev())
    ck = oe._Checker("rows_attn_drop[%s,H=%d]" % (head_irr, H))

    def hip(lg, v):
        with ops.dropout_seed_offset(word):
            out = ops.attn_aggregate(lg, v, graph, H, lay, p, 4321)
        return out

    def hip_bwd_too(lg, v):  # (the backward runs inside evaluate: the device word must be in force there as well)
        return hip(lg, v)

    ones = torch.ones(graph.N, seg.dim, dtype=torch.float64)
    with ops.dropout_seed_offset(word):
        _, hg = fo.evaluate(hip_bwd_too, [logit, value], [ones], torch.float32, device=oe._dev(), wrt=[1])
    alpha_ref = fo.segment_softmax(logit, row_ptr)
    hoc = fo.head_of_column(seg, H)
    first_col = torch.tensor([int((hoc == h).nonzero()[0]) for h in range(H)])
    ak = hg[0].double().cpu()
    assert float((ak - ak[:, first_col][:, hoc]).abs().max()) == 0.0  # one factor per (edge, head)
    m = ak[:, first_col] / alpha_ref
    kept = (m - 1.0 / (1.0 - p)).abs() < 1e-4
    assert bool((kept | (m.abs() < 1e-4)).all()), "mask entries other than 0 and 1 / (1 - p)"
    assert 0 < int(kept.sum()) < kept.numel()
    keep = kept.double() / (1.0 - p)
    with ops.dropout_seed_offset(word):
        oe._run(ck, ["out", "d_logit", "d_value"], hip_bwd_too, lambda lg, v: fo.attn_aggregate(lg, v, row_ptr, H, seg, keep)[0],
                [logit, value], [go], oe.ATTN_BOUNDS, ("d_logit",))
    ck.done()


# ------------------------------------------------------------------------------------------------- alpha logits
# alpha_fwd_kernel: ALPHA_U = 4 elements per thread, 1 024 per workgroup = 4 edges at H Kh = 256, 16 at H Kh = 64.  alpha_bwd4_kernel
# (unchanged, the backward of the same operator): 64 edges per workgroup, passes of 4 rows (H Kh = 256) or 16 rows (H Kh = 64).  (The float4
# kernel reads the rows of `a` with 16-byte loads: the ABI admits no row that is not 16-byte aligned.)
@pytest.mark.parametrize("H,Kh", [(8, 32), (8, 8)])
def test_alpha_logits_rows(H, Kh):
    """logit, d_a, d_alpha_dot; bounds and yardstick use of test_alpha_logits_edges"""
    from equiformer_amd import ops, so3
    ck = oe._Checker("rows_alpha[H=%d,Kh=%d]" % (H, Kh))
    bounds = {"logit": 5e-6, "d_a": 3e-5, "d_alpha_dot": 3e-5}
    for E in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257):
        a = oe._randn((E, H * Kh), 180 + E, 2.0)
        a[:, ::7] = 0.0
        adot = oe._randn((H * Kh,), 181)
        go = oe._randn((E, H), 182 + E)
        oe._run(ck, ["logit", "d_a", "d_alpha_dot"],
                lambda x, d: ops.alpha_logits(x, d, H, Kh, so3.C_SMOOTH_LEAKY_RELU_02),
                lambda x, d: fo.alpha_logits(x, d, H, Kh), [a, adot], [go], bounds, ("d_alpha_dot",),
                slices={"d_alpha_dot": [slice(i, i + 1) for i in range(H * Kh)]})
    ck.done()


# ------------------------------------------------------------------------------------------------- gather_add
@pytest.mark.parametrize("D", [480, 20, 128, 124])  # 120 and 5 float4 columns; 32 and 31: both sides of GATHER_ROW_MIN_D4
@pytest.mark.parametrize("with_b", [False, True])
def test_gather_add_rows(D, with_b):
    """msg = a[src] (+ b[dst]) through the C ABI with repeated and out-of-order src / dst (the operator of ops.py only ever passes a
    destination-sorted graph); E around the 4 edges of a wave and the 16 of a workgroup.  A copy and one add: exact in float32,
    so the comparison with the float64 restatement is for equality (bound of test_gather_add_and_segment_scale_edges kept)."""
    from equiformer_amd import lib
    dev = oe._dev()
    N = 9
    ck = oe._Checker("rows_gather[D=%d,b=%d]" % (D, with_b))
    for E in (1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 257):
        g = torch.Generator().manual_seed(150 + E)
        src = torch.randint(0, 4, (E,), generator=g).to(torch.int32)   # repeats, nodes that are nobody's source
        dst = torch.randint(0, N, (E,), generator=g).to(torch.int32)   # not sorted
        a, b = oe._randn((N, D), 151), oe._randn((N, D), 152)
        a_d, b_d = guard_input(a.float().to(dev)), guard_input(b.float().to(dev))
        src_d, dst_d = guard_input(src.to(dev)), guard_input(dst.to(dev))
        msg = guard_input(torch.full((E, D), float("nan"), device=dev))
        lib.call("eqf_gather_add_fwd", a_d.data_ptr(), b_d.data_ptr() if with_b else None, src_d.data_ptr(),
                 dst_d.data_ptr() if with_b else None, msg.data_ptr(), E, D, None)
        ref = fo.gather_add(a, b if with_b else None, src, dst)
        ck.cmp("msg", msg, ref, oe.SEG_BOUNDS["msg"])
        assert torch.equal(msg.cpu(), ref.float())
    ck.done()


# ------------------------------------------------------------------------------------------------- layer norm
LN_ROWS = (1, 3, 4, 5, 255, 256, 257)  # around WAVES_PER_BLOCK = 4; 64 workgroups and one row more
# QM9; segment lengths 5 and 9 (no multiple of 4 or 64, fewer entries than lanes); an E(3) row with a 0o segment (normalised like
# l > 0: no mean, no bias); a segment of exactly 256 entries (the register kernels' limit) and one of 260 (segment-by-segment kernels)
LN_IRREPS = ["128x0e+64x1e+32x2e", "5x0e+3x1e", "32x0e+16x0o+16x1o+8x1e", "256x0e+64x1e", "260x0e+64x1e"]


@pytest.mark.parametrize("irr", LN_IRREPS)
def test_layer_norm_rows(irr):
    from equiformer_amd import ops
    seg = fo.Segs(irr)
    lay = oe._layout(seg)
    w, b, wsl = oe._ln_params(seg)
    ck = oe._Checker("rows_ln[%s]" % irr)
    sl = {"y": seg.slices(), "dx": seg.slices(), "d_weight": wsl, "d_bias": [slice(None)]}
    for rows in LN_ROWS:
        x = fo.ln_input("randn", rows, seg, 160 + rows)
        go = oe._randn((rows, seg.dim), 161 + rows)
        oe._run(ck, ["y", "dx", "d_weight", "d_bias"], lambda t, ww, bb: ops.layer_norm(t, ww, bb, lay, 1e-5),
                lambda t, ww, bb: fo.layer_norm(t, ww, bb, seg, 1e-5), [x, w, b], [go], oe.LN_BOUNDS, slices=sl)
    ck.done()


@pytest.mark.parametrize("irr", LN_IRREPS)
def test_add_layer_norm_rows(irr):
    """the residual input in front of the norm and `dres` behind it"""
    from equiformer_amd import ops
    seg = fo.Segs(irr)
    lay = oe._layout(seg)
    w, b, wsl = oe._ln_params(seg)
    ck = oe._Checker("rows_add_ln[%s]" % irr)
    sl = {"y": seg.slices(), "xsum": seg.slices(), "da": seg.slices(), "db": seg.slices(), "d_weight": wsl, "d_bias": [slice(None)]}
    for rows in LN_ROWS:
        x = fo.ln_input("randn", rows, seg, 162 + rows)
        a1 = fo.f32r(0.25 * x)
        a2 = fo.f32r(x - a1)
        gy, gs = oe._randn((rows, seg.dim), 163 + rows), oe._randn((rows, seg.dim), 164 + rows)

        def hip(p, q, ww, bb):
            s, y = ops.add_layer_norm(p, q, ww, bb, lay, 1e-5)
            return y, s

        oe._run(ck, ["y", "xsum", "da", "db", "d_weight", "d_bias"], hip,
                lambda p, q, ww, bb: fo.add_layer_norm(p, q, ww, bb, seg, 1e-5), [a1, a2, w, b], [gy, gs], oe.LN_BOUNDS, slices=sl)
    ck.done()


# rstd and mean0 have no bound in tests/test_gpu_op_edges.py.  Both are one fp32 sum of at most 260 terms per segment -- at most 5
# serial additions per lane, 6 butterfly steps -- followed by a division; rstd adds the squares, eps and v_rsq_f32 (1 ulp): at most 16
# roundings of 2^-24 = 6e-8 each, 1e-6, on "randn" rows whose sums do not cancel (the squares) or are compared against the
# largest entry of the segment (the mean).  Bound: twice that.
STAT_BOUND = 2e-6


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("irr", LN_IRREPS)
def test_layer_norm_saved_statistics(irr, with_res):
    """rstd [rows][nseg] and mean0 [rows][n0] as the forward saves them for the backward and the weight gradient, through the C ABI"""
    from equiformer_amd import lib
    dev = oe._dev()
    seg = fo.Segs(irr)
    lay = oe._layout(seg)
    w, b, _ = oe._ln_params(seg)
    scal = [s for s in range(len(seg.segs)) if seg.scalar(s)]
    n0 = max(1, len(scal))
    ck = oe._Checker("rows_ln_stats[%s,res=%d]" % (irr, with_res))
    for rows in LN_ROWS:
        x = fo.ln_input("randn", rows, seg, 165 + rows)
        x1 = fo.f32r(0.25 * x) if with_res else x
        x2 = fo.f32r(x - x1) if with_res else None
        xs = fo.f32r(x1 + x2) if with_res else x
        put = lambda t: guard_input(t.float().to(dev))  # noqa: E731
        nanbuf = lambda *shape: guard_input(torch.full(shape, float("nan"), device=dev))  # noqa: E731
        x1_d, w_d, b_d = put(x1), put(w), put(b)
        x2_d = put(x2) if with_res else None
        xsum, y, rstd, mean0 = nanbuf(rows, seg.dim), nanbuf(rows, seg.dim), nanbuf(rows, len(seg.segs)), nanbuf(rows, n0)
        lib.call("eqf_add_layernorm_fwd", x1_d.data_ptr(), x2_d.data_ptr() if with_res else None,
                 xsum.data_ptr() if with_res else None, w_d.data_ptr(), b_d.data_ptr(), y.data_ptr(), rstd.data_ptr(), mean0.data_ptr(),
                 rows, lay.c_ref, 1e-5, None)
        ref_rstd, ref_mean, ref_max = [], [], []
        for s, sl in enumerate(seg.slices()):
            f = xs[:, sl]
            if seg.scalar(s):
                m = f.mean(dim=1, keepdim=True)
                ref_mean.append(m)
                ref_max.append(f.abs().amax(dim=1, keepdim=True))
                f = f - m
            ref_rstd.append((f.pow(2).mean(dim=1, keepdim=True) + 1e-5).pow(-0.5))
        ck.cmp("rstd", rstd, torch.cat(ref_rstd, dim=1), STAT_BOUND, slices=[slice(s, s + 1) for s in range(len(seg.segs))])
        if scal:
            got, ref, mx = mean0.double().cpu(), torch.cat(ref_mean, dim=1), torch.cat(ref_max, dim=1)
            assert torch.isfinite(got).all()
            err = float(((got - ref).abs() / mx).max())
            print("FIG %s mean0 rows=%d err=%.2e bound=%.2e" % (ck.case, rows, err, STAT_BOUND))
            assert err < STAT_BOUND, (irr, rows, err)
        ck.cmp("y", y, fo.layer_norm(xs, w, b, seg, 1e-5), oe.LN_BOUNDS["y"], slices=seg.slices())
        if with_res:
            ck.cmp("xsum", xsum, xs, oe.LN_BOUNDS["xsum"], slices=seg.slices())
    ck.done()


# ------------------------------------------------------------------------------------------------- LN + SiLU
@pytest.mark.parametrize("groups", [1, 7])
def test_ln_silu_rows(groups):
    """C = 64 (the radial MLP's width), rows around the 4 of a wave and the 16 of a workgroup, 1 025 = 64 workgroups and a row;
    bounds and yardstick use of test_ln_silu_edges"""
    from equiformer_amd import ops
    C = 64
    ck = oe._Checker("rows_lnsilu[groups=%d]" % groups)
    gam, bet = oe._randn((C * groups,), 170) * 0.5 + 1.0, oe._randn((C * groups,), 171)
    bounds = {"y": 5e-6, "dx": 2e-5, "d_gamma": 2e-5, "d_beta": 2e-5}
    for rows in (1, 3, 4, 5, 15, 16, 17, 1025):
        x = oe._randn((rows, C * groups), 172 + rows, 1.3)
        go = oe._randn((rows, C * groups), 173 + rows)
        oe._run(ck, ["y", "dx", "d_gamma", "d_beta"], lambda t, ga, be: ops.ln_silu(t, ga, be, 1e-5, groups),
                lambda t, ga, be: fo.ln_silu(t, ga, be, 1e-5, groups), [x, gam, bet], [go], bounds, ("y", "dx"),
                slices={"d_gamma": [slice(None)], "d_beta": [slice(None)]})
    ck.done()
