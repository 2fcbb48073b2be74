"""Shared by tests/test_gpu_dp_edges.py (GPU) and tests/test_fp64_ops.py (CPU): the head layouts, graphs and inputs at which the
dot-product attention kernels (csrc/dpattn.hip) are pinned to the float64 restatements of tests/fp64_ops.py (TEST
INFRASTRUCTURE, importable without a GPU; nothing here launches a kernel).

Head layouts: (irreps of one head, H); the q / k / v row holds H heads per segment, G = dim(head) H / 4 float4 groups.
  forward     one wavefront per edge, lane + 64 t owns group t of DP_SLOTS = 4: G = 1, 64 | 65 (slot 1), 192 | 193 (slot 3), 256
              (every slot full, the limit); E % 4 != 0 leaves waves of the last workgroup without an edge
  backward    one workgroup of 64 ceil(G / 64) threads per destination row, one thread per group: G = 64 | 65 adds a wavefront
  make_dptab  mul % H == 0 and (mul / H) % 4 == 0, H <= 8; `locate` finds the head of a group as (j4 % mul) / (mul / H): H = 1,
              H = 3 and 5 (no power of two), mul / H == 4 (one group per head and m-row), degree 3, odd-parity segments
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ops as fo  # noqa: E402

BOUND = 1e-5  # tests/test_gpu_dp_attention.py::test_kv_split_and_dp_logits_against_torch, here per row
YARD_FACTOR = 4.0  # tests/test_gpu_op_edges.py: max(project bound, 4 x float32 restatement on the same inputs)
HEADS = [("4x0e", 1),                      # G = 1
         ("4x0e+4x1e+4x2e", 3),            # G = 27, H = 3, mul / H == 4
         ("4x0e+4x1e", 8),                 # G = 32, H = 8 (the head limit), mul / H == 4
         ("16x0e+16x1e", 4),               # G = 64: slot 0 full, one wavefront in the backward
         ("20x0e+80x1e", 1),               # G = 65: lane 0 of slot 1, a second wavefront in the backward
         ("24x0e+24x1e", 8),               # G = 192: slots 0-2 full
         ("4x0e+256x1e", 1),               # G = 193: lane 0 of slot 3
         ("32x0e+32x1e", 8),               # G = 256: the forward's limit
         ("4x0e+4x3e", 5),                 # G = 40: degree 3, H = 5
         ("8x0e+4x0o+4x1e+4x1o", 2)]       # G = 18: odd-parity segments
SECOND_ORDER = [HEADS[4], HEADS[1]]        # G = 65 and H = 3
REFUSED_FWD = ("260x0e+256x1e", 1)         # G = 257: above the forward's 64 DP_SLOTS, inside the backward's 1024
REFUSED_BWD = ("1028x0e+1024x1e", 1)       # G = 1025
REFUSED_TAB = [("8x0e", 4), ("36x0e", 9), ("12x0e+8x1e", 3)]  # irreps of the whole row, H: mul / H = 2; H = 9; 8 % 3 != 0
GRAPHS = ["ragged", "chain1", "chain3", "chain4", "chain5"]


def groups(head_irr, H):
    return fo.Segs(head_irr).dim * H // 4


def irreps_str(seg):
    return "+".join("%dx%d%s" % (mul, l, "e" if p == 1 else "o") for (mul, l), p in zip(seg.segs, seg.par))


def graph(kind, device="cpu"):
    """"ragged": fo.ATTN_DEGREES (in-degrees 0-9, 31-33, 62-69, 127-130, empty rows first, in the middle and last);
    "chainE": E edges, one per destination, behind an empty first row"""
    if kind == "ragged":
        return fo.ragged_graph(fo.ATTN_DEGREES, 9, 140, device=device)
    E = int(kind[5:])
    return fo.ragged_graph([0] + [1] * E, 1, 141 + E, device=device)


def _randn(shape, seed):
    return fo.f32r(torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64))


def inputs(head_irr, H, N, E):
    """float32-rounded float64 tensors: q [N, D], kv [E, 2 D] and the cotangents of logit, k, v, dq and dkv"""
    D = fo.Segs(head_irr).dim * H
    s = 1000 * HEADS.index((head_irr, H)) if (head_irr, H) in HEADS else 99000
    return dict(q=_randn((N, D), s + 1), kv=_randn((E, 2 * D), s + 2), cl=_randn((E, H), s + 3), ck=_randn((E, D), s + 4),
                cv=_randn((E, D), s + 5), a=_randn((N, D), s + 6), b=_randn((E, 2 * D), s + 7))


def bound(yard=None):
    return BOUND if yard is None else max(BOUND, YARD_FACTOR * yard)


# ------------------------------------------------------------------------------------------------- wrong restatements
# What a kernel with a wrong `locate` or `kv_col` would compute, as the restatement on permuted inputs (the CPU controls).
def swap_heads(t, seg, H, s, h0, h1):
    """t [rows, D] with the channels of heads h0 and h1 exchanged in segment s"""
    (mul, l), off = seg.segs[s], seg.offsets[s]
    d, mh = 2 * l + 1, seg.segs[s][0] // H
    f = t[:, off:off + mul * d].reshape(-1, d, H, mh).clone()
    f[:, :, [h0, h1]] = f[:, :, [h1, h0]]
    out = t.clone()
    out[:, off:off + mul * d] = f.reshape(-1, mul * d)
    return out


def rescale_segment(t, seg, H, s, s_from):
    """t with segment s multiplied by scale[s_from] / scale[s]: the logits then carry the scale of s_from on segment s"""
    sc = fo.dp_scales(seg, H)
    (mul, l), off = seg.segs[s], seg.offsets[s]
    out = t.clone()
    out[:, off:off + mul * (2 * l + 1)] *= sc[s_from] / sc[s]
    return out


def swap_kv(kv, seg, s):
    """kv [E, 2 D] with keys and values exchanged in segment s"""
    (mul, l), off = seg.segs[s], 2 * seg.offsets[s]
    d = 2 * l + 1
    f = kv[:, off:off + 2 * mul * d].reshape(-1, d, 2, mul).clone()
    out = kv.clone()
    out[:, off:off + 2 * mul * d] = f.flip(2).reshape(-1, 2 * mul * d)
    return out
