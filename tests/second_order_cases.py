"""Inputs of tests/test_gpu_second_order_ops.py (TEST INFRASTRUCTURE, not product code): float32-rounded float64 CPU tensors,
built once per case at the largest row count and sliced per E.  tests/test_tp_restatements.py builds the same inputs for its
negative controls, so what it shows about the size of every substitution term holds for the seeds and scales the GPU tests
compare at.  Nothing here needs a GPU."""
import torch

import fp64_ops as fo
import fp64_tp as tp
from equiformer_amd import ops
from equiformer_amd.layout import DtpTable, RowLayout

# tests/test_gpu_sfcx.py::CASES: (input irreps, sh, consumer irreps, n2, per-edge w)
FUSED = {
    "qm9_sep_act": ("128x0e+64x1e+32x2e", "1x0e+1x1e+1x2e", "224x0e+64x1e+32x2e", 128, True),
    "qm9_sep_value": ("128x0e+64x1e+32x2e", "1x0e+1x1e+1x2e", "128x0e+64x1e+32x2e", 0, False),
    "md17_l3": ("128x0e+64x1e+64x2e+32x3e", "1x0e+1x1e+1x2e+1x3e", "128x0e+64x1e+64x2e+32x3e", 0, True),
    "wide_l2": ("256x0e+128x1e+64x2e", "1x0e+1x1e+1x2e", "256x0e+128x1e+64x2e", 0, True),
}
FUSED_E = [1, 37, 130]
# per-mode bars of tests/test_gpu_sfcx.py::TOL (exact-fp32 kernels: the fp32-class bar of split6)
FUSED_TOL = {"split": 1e-4, "bf16": 3e-2, "split6": 5e-6, "fp32": 5e-6}
# the gate of tests/test_gpu_sfcx.py::test_gate_folded_into_the_operator and tests/test_gpu_sfc_e3.py::GATES["four_segments"]:
# (irreps, sh, gated irreps, S)
GATED = {
    "so3": ("128x0e+64x1e+32x2e", "1x0e+1x1e+1x2e", "64x1e+32x2e", 128),
    "e3_four_segments": ("64x0e+32x0o+32x1e+64x1o", "1x0e+1x1o", "32x0o+32x1e+64x1o", 64),
}
DTP = {
    "so3": ("8x0e+4x1e+4x2e", "1x0e+1x1e+1x2e"),
    "e3": ("32x0e+32x0o+32x1e+32x1o", "1x0e+1x1o"),
}
DTP_E = [1, 37, 257]


class _Layout:
    """What the row operators need of a layout (segments, the C descriptor, the row length); RowLayout refuses rows with two
    0e segments, the C ABI does not (as in tests/test_gpu_op_edges.py)."""

    def __init__(self, seg):
        import ctypes
        from equiformer_amd import lib
        self.segs, self.par, self.offsets, self.dim = seg.segs, seg.par, seg.offsets, seg.dim
        self.c = lib.make_irreps(self.segs, self.par)
        self.c_ref = ctypes.byref(self.c)


def op_layout(irr):
    try:
        return RowLayout(irr)
    except NotImplementedError:
        return _Layout(fo.Segs(irr))


def _randn(g, *shape, scale=1.0):
    return fo.f32r(torch.randn(*shape, generator=g, dtype=torch.float64) * scale)


class Fused:
    """One fused SeparableFCTP problem.  `inputs(E)` = ([x, M, (w), weight, (weight2), bias, (bias2)], names), all requiring
    grad: the biases too, whose second-order gradients must come out absent or zero."""

    def __init__(self, case, seed=0):
        irr, sh, out_irr, n2, use_w = FUSED[case]
        self.table, self.lay = DtpTable(irr, sh, irr), RowLayout(out_irr)
        self.spec = ops.SfcSpec(self.table, self.lay, n2=n2)
        self.n2, self.use_w = n2, use_w
        g = torch.Generator().manual_seed(seed)
        E, t, s = max(FUSED_E), self.table, self.spec
        self.t = dict(x=_randn(g, E, t.layout_in.dim), M=_randn(g, E, t.m_numel))
        if use_w:
            self.t["w"] = _randn(g, E, t.weight_numel)
        self.t["weight"] = _randn(g, s.weight_numel, scale=0.1)
        if n2:
            self.t["weight2"] = _randn(g, s.weight2_numel, scale=0.1)
        self.t["bias"] = _randn(g, self.lay.mul_of(0))
        if n2:
            self.t["bias2"] = _randn(g, n2)
        self.names = list(self.t)

    def inputs(self, E):
        return [(v[:E] if k in ("x", "M", "w") else v).clone().requires_grad_(True) for k, v in self.t.items()]

    def split(self, ins):
        d = dict(zip(self.names, ins))
        return d["x"], d["M"], d.get("w"), d["weight"], d.get("weight2"), d["bias"], d.get("bias2")

    def ref(self, *ins):
        x, M, w, weight, weight2, bias, bias2 = self.split(ins)
        o1, o2 = tp.reference(self.spec, x, M, w, tp.blocks(self.spec, weight), weight2, bias, bias2)
        return o1 if o2 is None else (o1, o2)

    def diff_sets(self):
        """name -> indices of the inputs the first derivative is taken with respect to"""
        data = [i for i, n in enumerate(self.names) if n in ("x", "M", "w")]
        return {"xMw": data, "M": [self.names.index("M")], "x": [self.names.index("x")]}


class Gated:
    """gate -> fused SeparableFCTP (no second consumer): inputs [x_raw, M, w, weight, bias]"""

    def __init__(self, case, seed=0):
        from equiformer_amd import so3
        irr, sh, gated_irr, S = GATED[case]
        self.table, self.lay = DtpTable(irr, sh, irr), RowLayout(irr)
        self.spec = ops.SfcSpec(self.table, self.lay, n2=0)
        self.gated = RowLayout(gated_irr)
        G = sum(m for m, _ in self.gated.segs)
        self.gate = (S, self.gated, so3.C_SILU, so3.C_SIGMOID)
        g = torch.Generator().manual_seed(seed)
        E, t = max(FUSED_E), self.table
        self.t = dict(x_raw=_randn(g, E, S + G + self.gated.dim), M=_randn(g, E, t.m_numel), w=_randn(g, E, t.weight_numel),
                      weight=_randn(g, self.spec.weight_numel, scale=0.1), bias=_randn(g, self.lay.mul_of(0)))
        self.names = list(self.t)

    def inputs(self, E):
        return [(v[:E] if k in ("x_raw", "M", "w") else v).clone().requires_grad_(True) for k, v in self.t.items()]

    def ref(self, x_raw, M, w, weight, bias):
        xg = fo.gate(x_raw, *self.gate)
        return tp.reference(self.spec, xg, M, w, tp.blocks(self.spec, weight), None, bias, None)[0]

    def diff_sets(self):
        return {"xMw": [0, 1, 2], "M": [1]}


class Dtp:
    """un-fused depth-wise tensor product: inputs [x, M, (w)]"""

    def __init__(self, case, use_w, seed=3):
        irr, sh = DTP[case]
        self.table = DtpTable(irr, sh, irr)
        g = torch.Generator().manual_seed(seed)
        E, t = max(DTP_E), self.table
        self.t = dict(x=_randn(g, E, t.layout_in.dim), M=_randn(g, E, t.m_numel))
        if use_w:
            self.t["w"] = _randn(g, E, t.weight_numel)
        self.sh = _randn(g, E, (t.lmax_sh + 1) ** 2)
        self.names = list(self.t)

    def inputs(self, E):
        return [v[:E].clone().requires_grad_(True) for v in self.t.values()]

    def ref(self, x, M, w=None):
        return tp.product(self.table, x, M, w)

    def diff_sets(self):
        d = {"xMw": list(range(len(self.names))), "M": [1]}
        if "w" in self.t:
            d["w"] = [2]
        return d


# ------------------------------------------------------------------------------------------------- the smaller operators
FOLD_LENS = [1, 2, 63, 64, 65, 200, 1]  # tests/test_gpu_op_edges.py::test_fold_weight_edges


def fold_problem():
    """(W, w, row_start, w_of_row): rows around the 64-lane stride, one shared weight per row"""
    row_start = torch.tensor([0] + FOLD_LENS).cumsum(0).to(torch.int32)
    w_of_row = torch.randperm(len(FOLD_LENS), generator=torch.Generator().manual_seed(84)).to(torch.int32)
    g = torch.Generator().manual_seed(85)
    n = int(row_start[-1])
    return (_randn(g, n).requires_grad_(True), _randn(g, len(FOLD_LENS)).requires_grad_(True), row_start, w_of_row)


ALN_IRREPS = [fo.LN_IRREPS[0], "8x0e+4x1e", "64x0e+32x1e+16x0e"]


def aln_problem(irr, rows=5, seed=41):
    """(a, b, weight, bias, segments) of add_layer_norm"""
    lay = fo.Segs(irr)
    g = torch.Generator().manual_seed(seed)
    nw = sum(m for m, _ in lay.segs)
    nb = sum(m for s, (m, _) in enumerate(lay.segs) if lay.scalar(s))
    a, b = _randn(g, rows, lay.dim), _randn(g, rows, lay.dim)
    w = fo.f32r(torch.rand(nw, generator=g, dtype=torch.float64) + 0.5)
    bias = _randn(g, nb)
    return [t.requires_grad_(True) for t in (a, b, w, bias)], lay
