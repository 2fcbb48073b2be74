"""Fused SeparableFCTP kernels (eqf_sfc_* / eqf_sfcx_*) on E(3) irreps, operator level, against an fp64 restatement of the
operator from the path table (autograd for every gradient):

    mid[e, seg(l3,p3), k, out_ch + u] = w[e, w_off + u] * sum_i M[e, m_off + i d3 + k] * x[e, in_off + i mul + u]
    out1[e, seg(l,p)] = mid[e, seg(l,p)] . W_(l,p)  (+ bias on 0e)        out2[e] = mid[e, seg(0e)] . W2 + bias2

Tolerances: those of tests/test_gpu_sfcx.py for the same quantity in the same mode (relative to the result scale): split 1e-4,
bf16 3e-2, split6 (sfcx mode 2, 3 + 3 planes) 5e-6, and the same fp32-class bar for the exact-fp32 kernels of matrix mode "fp32".  Edge counts: 1, 31, 33, 130 (tile edges), either side of the
dispatch thresholds of csrc/sfcx.hip -- Y_MIN_EDGES 1 500 (multi-wave forward), W_MIN_EDGES 9 000 / W_MIN_EDGES_PLAIN 20 000
(multi-wave weight gradient with / without per-edge weights), 22 000 (its rounds) -- and 700 / 2 800, which lie on either side
of the item-count limits of the wave-split forward and the two-waves-per-item data gradient for these layouts (those limits
count work items, 2 048 and 1 536 slots, not edges).
Wall time of this file on an MI355X, one run each (pytest's figure): 7.4 s at the parent commit, 9.3 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fp64_ops  # noqa: E402
from fp64_tp import blocks as _blocks, reference  # noqa: E402  (the restatement of the operator from its path table)
from equiformer_amd import ops, so3  # noqa: E402
from equiformer_amd.layout import DtpTable, RowLayout  # noqa: E402
from poison import guard_input, poisoned_ops  # noqa: E402,F401  (every launch on poisoned allocations, inputs between NaN bands)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_ops")]

SH = "1x0e+1x1o"
TOL = {0: 1e-4, 1: 3e-2, 2: 5e-6, None: 5e-6}  # tests/test_gpu_sfcx.py: split, bf16, split6; fp32-class for the exact kernels
MODE_OF = {"split": 0, "bf16": 1, "split6": 2, "fp32": None}
GATE_TOL = {"split": 1e-5, "bf16": 5e-3}  # tests/test_gpu_sfcx.py::test_gate_folded_into_the_operator: same-mode comparison
LAYOUTS = {
    "all_four_32": ("32x0e+32x0o+32x1e+32x1o", "32x0e+32x0o+32x1e+32x1o"),
    "unequal": ("64x0e+32x0o+32x1e+64x1o", "64x0e+32x0o+32x1e+64x1o"),
    "odd_only_degree": ("32x0e+32x1o", "32x0e+32x1o"),
    "oc20": ("256x0e+64x0o+64x1e+64x1o", "448x0e+64x0o+64x1e+64x1o"),
}
E_COMMON = [1, 31, 33, 130, 700, 1499, 1500, 2800]
E_WITH_W = [8999, 9000]
E_PLAIN = [19999, 20000, 21999, 22000]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


class Case:
    """inputs at the largest edge count (fp32 on the device, each between NaN guard bands), sliced per E into guarded copies; the
    fp64 reference is computed per slice"""

    def __init__(self, layout, n2, use_w):
        irr, out = LAYOUTS[layout]
        dev = _dev()
        self.table, self.lay = DtpTable(irr, SH, irr), RowLayout(out)
        self.spec = ops.SfcSpec(self.table, self.lay, n2=n2)
        assert self.spec.supported and self.table.has_odd
        self.Es = E_COMMON + (E_WITH_W if use_w else E_PLAIN)
        Emax = max(self.Es)
        g = torch.Generator().manual_seed(7)
        r = lambda *s, scale=1.0: guard_input(torch.randn(*s, generator=g).to(dev) * scale)  # noqa: E731
        t, s = self.table, self.spec
        self.x, self.M = r(Emax, t.layout_in.dim), r(Emax, t.m_numel)
        self.w = r(Emax, t.weight_numel) if use_w else None
        self.weight = r(s.weight_numel, scale=0.1)
        self.weight2 = r(s.weight2_numel, scale=0.1) if n2 else None
        self.bias, self.bias2 = r(self.lay.mul_of(0)), (r(n2) if n2 else None)
        self.d1, self.d2 = r(Emax, self.lay.dim), (r(Emax, n2) if n2 else None)

    def ref(self, E, swap=None):
        s = self.spec
        f = lambda t, n=None: None if t is None else (t if n is None else t[:n]).double().clone().requires_grad_(True)  # noqa: E731
        x, M, w = f(self.x, E), f(self.M, E), f(self.w, E)
        weight, weight2, bias, bias2 = f(self.weight), f(self.weight2), f(self.bias), f(self.bias2)
        blocks = _blocks(s, weight)
        if swap is not None:
            a, b = swap
            blocks[a], blocks[b] = blocks[b], blocks[a]
        o1, o2 = reference(s, x, M, w, blocks, weight2, bias, bias2)
        loss = (o1 * self.d1[:E].double()).sum()
        if o2 is not None:
            loss = loss + (o2 * self.d2[:E].double()).sum()
        wrt = dict(dx=x, dM=M, dw=w, gW=weight, gW2=weight2, gb=bias, gb2=bias2)
        names = [k for k, v in wrt.items() if v is not None]
        grads = torch.autograd.grad(loss, [wrt[k] for k in names])
        out = dict(zip(names, grads))
        out["o1"], out["o2"] = o1.detach(), (o2.detach() if o2 is not None else None)
        return out

    def run(self, E, mode):
        s = self.spec
        c = lambda t: None if t is None else guard_input(t[:E])  # noqa: E731  (NaN right behind row E - 1)
        x, M, w, d1, d2 = c(self.x), c(self.M), c(self.w), c(self.d1), c(self.d2)
        o1, o2 = ops._sfc_fwd(x, M, w, self.weight, self.bias, self.weight2, self.bias2, s, mode)
        dx, dM, dw = ops._sfc_bwd_data(x, M, w, self.weight, self.weight2, d1, d2, s, True, mode)
        gW = torch.zeros_like(self.weight)
        gW2 = torch.zeros_like(self.weight2) if self.weight2 is not None else None
        gb, gb2 = torch.zeros_like(self.bias), (torch.zeros_like(self.bias2) if self.bias2 is not None else None)
        if not ops._sfc_bwd_weight(x, M, w, d1, d2, s, gW, gW2, mode, gb, gb2):
            gb, gb2 = None, None  # (this launch does not take the bias gradients along: the column sums are another kernel's)
        torch.cuda.synchronize()
        return dict(o1=o1, o2=o2, dx=dx, dM=dM, dw=dw, gW=gW, gW2=gW2, gb=gb, gb2=gb2)


_cases = {}


def _case(layout, n2, use_w):
    key = (layout, n2, use_w)
    if key not in _cases:
        _cases.clear()  # one case resident at a time
        _cases[key] = Case(*key)
    return _cases[key]


def _errors(got, ref):
    errs = {}
    for k, g in got.items():
        if g is None:
            continue
        assert torch.isfinite(g).all(), k
        errs[k] = _rel(g, ref[k])
    return errs


@pytest.mark.parametrize("mode", ["split", "bf16", "split6", "fp32"])
@pytest.mark.parametrize("use_w", [True, False], ids=["w", "now"])
@pytest.mark.parametrize("n2", [0, 32])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_fused_operator_against_fp64(layout, n2, use_w, mode):
    case = _case(layout, n2, use_w)
    m = MODE_OF[mode]
    if m is not None:
        assert case.spec.x_mask(m) & 1  # the split-precision forward serves it (a cleared bit: the exact-fp32 launch)
    bad = {}
    for E in case.Es:
        errs = _errors(case.run(E, m), case.ref(E))
        print("%s n2=%d %s %s E=%d: %s" % (layout, n2, "w" if use_w else "-", mode, E, {k: "%.1e" % v for k, v in errs.items()}))
        assert {"o1", "dx", "dM", "gW"} <= set(errs) and (n2 == 0 or {"o2", "gW2"} <= set(errs)) and (not use_w or "dw" in errs)
        for k, v in errs.items():
            if v > TOL[m]:
                bad[(E, k)] = v
    assert not bad, bad


@pytest.mark.parametrize("mode", ["split", "fp32"])
def test_swapped_0e_0o_blocks_are_seen(mode):
    """the degree-keyed bug: 0e and 0o share l = 0.  all_four_32 has equal-shaped 0e / 0o matrices ([64, 32]); an expected value
    built with the two blocks exchanged must FAIL the comparison this file makes (and pass with them in place)."""
    case = _case("all_four_32", 0, True)
    assert case.spec.degs[0][:3] == case.spec.degs[1][:3] == (0, 64, 32) and case.spec.pars[:2] == [1, -1]
    m = MODE_OF[mode]
    got = case.run(130, m)
    right = _errors(got, case.ref(130))
    wrong = _errors(got, case.ref(130, swap=(0, 1)))
    print("swap check %s: right %s wrong %s" % (mode, right, wrong))
    assert max(right.values()) <= TOL[m]
    assert wrong["o1"] > 100 * TOL[m] and wrong["dx"] > 100 * TOL[m]


GATES = {  # irreps (input = output of the operator), gated segments, S
    # the gate the issue names.  Its 1o consumer is fed by two input segments of degree 1 (1o x Y0, 1e x Y1), which the
    # multi-wave forward declines: every E runs the one-wave forward, the E either side of Y_MIN_EDGES_GATED included
    "four_segments": ("64x0e+32x0o+32x1e+64x1o", "32x0o+32x1e+64x1o", 64),
    # one input segment per degree and consumer: the multi-wave forward takes this one from Y_MIN_EDGES_GATED (4 000) edges on
    "no_1e": ("64x0e+32x0o+64x1o", "32x0o+64x1o", 64),
}


@pytest.mark.parametrize("E", [1, 33, 130, 3999, 4000, 19999, 20000])
@pytest.mark.parametrize("mode", ["split", "bf16"])
@pytest.mark.parametrize("gate_case", sorted(GATES))
def test_gate_with_a_gated_0o_segment_folded_into_the_operator(gate_case, mode, E):
    """eqf_sfcx_*_gated on E(3) gates: scalars = 0e only, 0o / 1e / 1o multiplied by sigmoid gates.  Fused-with-folded-gate
    against  (a) the separate gate kernels followed by the plain fused operator in the same matrix mode -- the comparison and
    the bars (1e-5 split, 5e-3 bf16) of tests/test_gpu_sfcx.py::test_gate_folded_into_the_operator --,  (b) the un-fused chain
    linear(dtp(gate(x_raw))): exact-fp32 tensor product, another quantity, held to the mode's bar against any reference (1e-4 /
    3e-2),  (c) fp64 (fp64_ops.gate + the restatement above), same bar.  E: tile edges, either side of Y_MIN_EDGES_GATED (4 000:
    multi-wave forward, see GATES) and of W_MIN_EDGES_PLAIN (20 000: multi-wave weight gradient with gated 0o slabs)."""
    dev = _dev()
    irr, gated_irr, S = GATES[gate_case]
    table, lay = DtpTable(irr, SH, irr), RowLayout(irr)
    spec = ops.SfcSpec(table, lay, n2=0)
    gated_layout = RowLayout(gated_irr)
    G = sum(m for m, _ in gated_layout.segs)
    g = torch.Generator().manual_seed(E)
    r = lambda *s, scale=1.0: guard_input(torch.randn(*s, generator=g).to(dev) * scale)  # noqa: E731
    x_raw = r(E, S + G + gated_layout.dim).requires_grad_(True)
    M = r(E, table.m_numel).requires_grad_(True)
    weight = r(spec.weight_numel, scale=0.1).requires_grad_(True)
    bias = r(lay.mul_of(0)).requires_grad_(True)
    c = r(E, lay.dim)
    gate = (S, gated_layout, so3.C_SILU, so3.C_SIGMOID)
    lin = ops.LinearSpec(table.layout_out, lay)
    res = {}
    with ops.matrix_mode(mode):
        assert ops.sep_fctp_gated_ok(spec, x_raw.shape[1], S, gated_layout, E=E)
        for how in ("folded", "separate", "unfused"):
            if how == "folded":
                y = ops.sep_fctp_gated(x_raw, M, None, weight, bias, spec, gate)
            elif how == "separate":
                y = ops.sep_fctp(ops.gate(x_raw, *gate), M, None, weight, bias, spec)
            else:
                y = ops.irreps_linear(ops.dtp(ops.gate(x_raw, *gate), M, None, table), weight, bias, lin)
            grads = torch.autograd.grad((y * c).sum(), [x_raw, M, weight, bias])
            res[how] = [y.detach()] + [t.detach() for t in grads]
    f = lambda t: t.detach().double().clone().requires_grad_(True)  # noqa: E731
    xr, Mr, Wr, br = f(x_raw), f(M), f(weight), f(bias)
    yr, _ = reference(spec, fp64_ops.gate(xr, *gate), Mr, None, _blocks(spec, Wr), None, br, None)
    ref = [yr.detach()] + list(torch.autograd.grad((yr * c.double()).sum(), [xr, Mr, Wr, br]))
    names = ["out", "d x_raw", "d coupling", "d weight", "d bias"]
    tol = TOL[MODE_OF[mode]]
    e_sep = {n: _rel(a, b) for n, a, b in zip(names, res["folded"], res["separate"])}
    e_unf = {n: _rel(a, b) for n, a, b in zip(names, res["folded"], res["unfused"])}
    e_ref = {n: _rel(a, b) for n, a, b in zip(names, res["folded"], ref)}
    print("E(3) gate folded, %s %s E=%d: vs separate gate %s vs un-fused %s vs fp64 %s" % (gate_case, mode, E, e_sep, e_unf, e_ref))
    assert all(v < GATE_TOL[mode] for v in e_sep.values()), e_sep
    assert all(v < tol for v in e_unf.values()), e_unf
    assert all(v < tol for v in e_ref.values()), e_ref
