"""Shared by tests/test_gpu_dtp_edges.py (GPU) and tests/test_fp64_ops.py (CPU): the path tables, edge counts, inputs and
float64 references at which the un-fused depth-wise tensor product (eqf_dtp_coupling_*, eqf_dtp_fwd / _bwd in csrc/edge.hip) and
the DTP-generating GEMMs (eqf_dtp_linear_fwd / _wgrad in csrc/gemm.hip) are pinned to tests/fp64_tp.py (TEST INFRASTRUCTURE,
importable without a GPU; nothing here launches a kernel).

Tile arithmetic of the DTP-generating GEMMs, restated from csrc/gemm.hip (`tile_of`, `tn_tile_of`, checked against the names the
library's profiler reports):
  rows kernel   bn = 128 / 64 / 32 for N > 64 / > 32 / <= 32; bm = 64 when bn >= 64 (few tiles at these E), else 128; a 128-row
                tile that holds more than 8 ROWS_PAIRS = 64 edges, or more coupling than MAX_MTILE floats, becomes 64 x 64
                (N <= 32 scalars: 128 edges per tile).  ept = bm / d3: 64, 21, 12, 9 at bm = 64 and 42, 25, 18 at bm = 128.
  tn kernel     BM = 32 iff K % 64 != 0 and K < 256, BN likewise from N; ept = 32 / d3 edges per step, at least 8 steps per split:
                the second split starts at E = 8 (32 / d3) + 1 = 257, 81, 49, 33.
"""
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ops as fo  # noqa: E402
import fp64_tp as tp  # noqa: E402

SH = {1: "1x0e+1x1e", 2: "1x0e+1x1e+1x2e", 3: "1x0e+1x1e+1x2e+1x3e"}
# name: irreps in, irreps sh, node output (the degrees the product keeps)
TABLES = {
    "narrow": ("8x0e+4x1e+4x2e", SH[2], "8x0e+4x1e+4x2e"),                    # 72 weights: one partial block
    "two_blocks": ("32x0e+32x1e+32x2e", SH[2], "32x0e+32x1e+32x2e"),          # 480 weights: blockIdx.y = 0, 1 of the forward
    "l3": ("128x0e+64x1e+64x2e+32x3e", SH[3], "128x0e+64x1e+64x2e+32x3e"),    # 288 input channels: the backward's stride loop
    "parity": ("64x0e+32x0o+32x1e+64x1o", "1x0e+1x1o", "64x0e+32x0o+32x1e+64x1o"),
    "uncovered": ("8x0e+8x3e", SH[1], "8x0e"),                               # no path reads 8x3e: dx there is the zero prefill
}
EDGES = [1, 2, 255, 257]
# the un-fused product: tests/test_gpu_ops.py::test_dtp_unfused; M has no bound there: it is an output like `out`
BOUNDS = {"M": 5e-6, "out": 5e-6, "dx": 1e-5, "d_sh": 2e-5, "dM": 1e-5, "dw": 1e-5}
# dtp_linear: tests/test_gpu_gemm_edges.py, exact-fp32 back end (BASE: forward 2e-6, gradients 5e-6)
LIN_BOUNDS = {"out": 2e-6, "dx": 5e-6, "dM": 5e-6, "dw": 5e-6, "dweight": 5e-6}
YARD_FACTOR = 4.0

# DTP-generating GEMMs: K per output degree 96 / 192 / 192; 128 / 256 / 288; degree 3 with 32 channels per input degree
LIN_TABLES = {
    "k96": ("32x0e+32x1e+32x2e", SH[2], "32x0e+32x1e+32x2e"),
    "k288": ("32x0e+32x1e+64x2e", SH[2], "32x0e+32x1e+64x2e"),
    "deg3": ("32x0e+32x1e+32x2e+32x3e", SH[3], "32x0e+32x1e+32x2e+32x3e"),
}
LIN_N = [32, 64, 96, 160]
ROWS_PAIRS, MAX_MTILE = 8, 6656  # csrc/gemm.hip (tests/test_fp64_ops.py reads them back from the source)


def lin_edges(lmax):
    """E on either side of one row tile (ept, ept + 1) and of one weight-gradient split (8 (32 / d3), + 1), per degree"""
    out = set()
    for l in range(lmax + 1):
        d = 2 * l + 1
        for ept in (64 // d, 64 if d == 1 else 128 // d, 8 * (32 // d)):
            out |= {ept, ept + 1}
    return sorted(out)


def table(name):
    from equiformer_amd.layout import DtpTable
    return DtpTable(*{**TABLES, **LIN_TABLES}[name])


def consumer(name, N):
    """the consumer layout: N channels of every segment the table produces"""
    from equiformer_amd.layout import RowLayout
    t = table(name)
    return RowLayout("+".join("%dx%d%s" % (N, l, "e" if p == 1 else "o") for (_, l), p in zip(t.layout_out.segs, t.layout_out.par)))


def m_len(t, l3, par):
    return sum((2 * p["l1"] + 1) * (2 * l3 + 1) for p in t.paths if (p["l3"], p["p3"]) == (l3, par))


def tile_of(t, l3, par, N, E):
    """(bm, bn, ept) of launch_rows<A_DTP> for the segment (l3, par) with N consumer channels at E edges"""
    d = 2 * l3 + 1
    bn = 128 if N > 64 else (64 if N > 32 else 32)
    tiles128 = -(-E * d // ((128 // d) * d)) * -(-N // bn)
    bm = 64 if (bn >= 64 and tiles128 < 4096) else 128
    if 128 // d > 8 * ROWS_PAIRS or (128 // d) * m_len(t, l3, par) > MAX_MTILE:
        bm, bn = 64, max(bn, 64)
    ept = bm // d
    assert ept <= 8 * ROWS_PAIRS and ept * m_len(t, l3, par) <= MAX_MTILE
    return bm, bn, ept


def tn_tile_of(K, N):
    return (32 if (K % 64 != 0 and K < 256) else 64), (32 if (N % 64 != 0 and N < 256) else 64)


def _randn(shape, seed, scale=1.0):
    return fo.f32r(torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale)


def inputs(name, E):
    """float32-rounded float64 tensors of the coupling and product launches"""
    t = table(name)
    s = 7000 + 100 * sorted({**TABLES, **LIN_TABLES}).index(name) + E
    return dict(x=_randn((E, t.layout_in.dim), s), M=_randn((E, t.m_numel), s + 1), w=_randn((E, t.weight_numel), s + 2),
                sh=_randn((E, (t.lmax_sh + 1) ** 2), s + 3), go=_randn((E, t.layout_out.dim), s + 4),
                cM=_randn((E, t.m_numel), s + 5))


def sfc_like(t, lay):
    """what fp64_tp.reference / blocks read of a spec (degs, pars, w_offs, n2, table), from the table and the consumer layout,
    with the flat weight in the order of ops.DtpLinearSpec"""
    degs, pars, w_offs, off = [], [], [], 0
    for (K, l3), par in zip(t.layout_out.segs, t.layout_out.par):
        j = lay.seg_index(l3, par)
        if j is None:
            continue
        N = lay.segs[j][0]
        degs.append((l3, K, N, N)), pars.append(par), w_offs.append(off)
        off += K * N
    return types.SimpleNamespace(table=t, degs=degs, pars=pars, w_offs=w_offs, n2=0, weight_numel=off)


def lin_inputs(name, N, E):
    t, lay = table(name), consumer(name, N)
    sp = sfc_like(t, lay)
    d = inputs(name, E)
    s = 9000 + 100 * sorted(LIN_TABLES).index(name) + N + E
    d.update(weight=_randn((sp.weight_numel,), s, 0.1), bias=_randn((lay.mul_of(0),), s + 1), go=_randn((E, lay.dim), s + 2))
    return d


def lin_reference(name, N, use_w=True):
    """(x, M, [w,] weight, bias) -> out of fp64_tp.reference: product, then the per-segment linear"""
    sp = sfc_like(table(name), consumer(name, N))
    if use_w:
        return lambda x, M, w, weight, bias: tp.reference(sp, x, M, w, tp.blocks(sp, weight), None, bias, None)[0]
    return lambda x, M, weight, bias: tp.reference(sp, x, M, None, tp.blocks(sp, weight), None, bias, None)[0]


# ------------------------------------------------------------------------------------------------- wrong restatements
def wrong_table(t, kind):
    """the path table a faulty kernel would follow: "out_ch" -- two paths of one output segment (equal mul) write each other's
    channels; "w" -- one path reads the weights of the neighbouring channel"""
    paths = [dict(p) for p in t.paths]
    if kind == "out_ch":
        a = paths[0]
        b = next(p for p in paths[1:] if (p["l3"], p["p3"], p["mul"]) == (a["l3"], a["p3"], a["mul"]))
        a["out_ch"], b["out_ch"] = b["out_ch"], a["out_ch"]
    else:
        assert kind == "w"
        paths[0]["w_off"] += 1
    return types.SimpleNamespace(paths=paths, layout_out=t.layout_out)
