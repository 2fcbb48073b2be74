"""The graph-norm / instance-norm HIP kernels (csrc/graphnorm.hip; ops.graph_norm, ops.add_graph_norm) against the float64
restatements of tests/fp64_norms.py (which tests/test_norm_restatements.py pins to the reference's own classes).

Shapes: irreps with 8 / 224 / 5 / 0 scalar channels, a pseudo-scalar segment, channel chunks beyond one wavefront;
graphs of 1, 2, 63, 64, 65 and 130 nodes (around and beyond the 4 waves of a reduction workgroup), one-node graphs, empty
graphs in the middle and at the end, 70 graphs of 1-3 nodes.  Inputs: randn, randn + 100 (the mean dwarfs the spread; a
smaller offset on the sets with tiny graphs, see OFFSETS), and graphs whose nodes are all identical (zero variance: eps
governs).  mean_shift = ones, uniform in [0.5, 1.5], and the
instance norm; weights 1 + 0.5 randn.

Metric `fp64_ops.per_row_rel`: y / dx / da / db / xsum per (row, segment), d_weight per segment, d_bias and d_mean_shift
as a whole.  Bounds are the layer norm's (tests/test_gpu_op_edges.py LN_BOUNDS: y 5e-6, xsum 2e-7, gradients 2e-5;
d_mean_shift 2e-5 as well), each taken as max(bound, 4 x the error of the SAME restatement evaluated in float32 on the
CPU on the same inputs) on every quantity but xsum: float32 arithmetic itself misses the plain bounds where the centred
value cancels (one-node graphs with mean_shift near 1, randn + 100).  No bound in use may exceed BOUND_CAP = 1e-2, so the
yardstick cannot excuse a wrong formula; the checker asserts it.  Every test prints "FIG <case> <quantity> err=...
yard=... bound=..." lines (pytest -rA or -s shows them).

Measured on an MI355X: the worst case of each quantity (largest err / bound) from the FIG lines of one run; err = the
kernel, yard = the float32 restatement on the same inputs:
  graph_norm      y 1.3e-6, yard 1.2e-6 (5e-6; 5x0e, seventy); dx 3.6e-5, yard 2.2e-5 -> 8.8e-5 (8x0e+2x0o+4x1e+4x1o, one-node
                  and two-node graphs); d_mean_shift 1.5e-5, yard 1.5e-5 -> 5.8e-5 (224 channels, seventy); d_weight 9.9e-6,
                  yard 9.9e-6 -> 4.0e-5; d_bias 5.4e-8 (2e-5)
  add_graph_norm  xsum 4.5e-8 (2e-7); y 1.6e-6, yard 1.6e-6 -> 6.4e-6; da = db 5.9e-6, yard 5.3e-6 -> 2.1e-5; d_mean_shift
                  7.1e-6, yard 7.0e-6 -> 2.8e-5 ([130], offset 100); d_weight 1.3e-5, yard 1.3e-5 -> 5.1e-5; d_bias 5.4e-8
  the largest bound any case used: 5.5e-3 (dx of 5x0e on the one- to three-node graphs, where every entry of the
  reference is a residue of order eps); the kernel stays at or under the float32 restatement's own error there.
Wall time of this file on an MI355X, one run each (pytest's figure): 6.4 s at the parent commit, 6.8 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py).
"""
import ctypes
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_norms as fn  # noqa: E402
import fp64_ops as fo  # noqa: E402
from poison import poisoned_ops  # noqa: E402,F401  (every launch of this file runs on poisoned, guarded allocations)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_ops")]

BOUNDS = {"y": 5e-6, "xsum": 2e-7, "dx": 2e-5, "da": 2e-5, "db": 2e-5, "d_weight": 2e-5, "d_bias": 2e-5,
          "d_mean_shift": 2e-5}
YARD = ("y", "dx", "da", "db", "d_weight", "d_bias", "d_mean_shift")  # everything but xsum
BOUND_CAP = 1e-2
EPS = 1e-5

IRREPS = ["8x0e+4x1e+2x2e", "128x0e+64x1e+32x2e", "8x0e+2x0o+4x1e+4x1o", "5x0e", "3x1e+2x2e"]
_g70 = torch.Generator().manual_seed(7)
SIZES = {"ragged": [1, 2, 63, 64, 65, 3],
         "one130": [130],
         "ones-and-empty": [1, 1, 1, 1, 1, 0, 2, 2, 2, 0],
         "seventy": torch.randint(1, 4, (70,), generator=_g70).tolist()}
FAMILIES = ["randn", "randn+offset", "identical"]
# "randn+offset" is randn + 100 where float32 can be judged on it.  In a graph of one to three nodes the centred value of
# a 0e channel is a difference of two or three nearly equal numbers, and its input gradient is a residue of order eps:
# the float32 restatement itself is off by 0.2 (per_row_rel of dx) at an offset of 100 on the sets made of such graphs,
# which would lift the bound above BOUND_CAP.  The offset of a set is therefore the largest of 100, 30, 10, 3, 1 at which
# 4 x the float32 restatement's error (CPU, from the reference alone; all irreps, mean shifts and quantities) stays under
# half the cap: 9.0e-5 at 100 for [130]; 3.2e-3 at 30 for the ragged set (1.5e-1 at 100); 3.4e-3 and 4.5e-3 at 1 for the
# two sets of one- to three-node graphs (1.3e-2 and 1.7e-2 at 3).
OFFSETS = {"ragged": 30.0, "one130": 100.0, "ones-and-empty": 1.0, "seventy": 1.0}
SHIFTS = ["ones", "uniform", "instance"]


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


class _Layout:
    """What the operators need of a row layout (segments, the C descriptor, the row length)."""

    def __init__(self, irreps):
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
        assert lim <= BOUND_CAP, (self.case, name, "the float32 yardstick lifts the bound to %.2e, above the cap" % lim)
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


def _run(ck, names, hip_fn, ref_fn, inputs, gouts, slices):
    """outputs and gradients of hip_fn (float32, GPU) against ref_fn (float64, CPU; float32: the yardstick); names are per
    compared tensor, outputs first, then the gradients wrt the floating inputs"""
    ro, rg, yo, yg = fo.yardstick(ref_fn, inputs, gouts)
    # (a row without 0e segments has empty bias / mean_shift tensors, which the restatement never touches)
    rg = [torch.zeros_like(t) if g is None else g for g, t in zip(rg, inputs)]
    yg = [torch.zeros_like(t) if g is None else g for g, t in zip(yg, inputs)]
    ho, hg = fo.evaluate(hip_fn, inputs, gouts, torch.float32, device=_dev())
    for name, h, r, y in zip(names, ho + hg, ro + rg, yo + yg):
        ck.cmp(name, h, r, BOUNDS[name], y if name in YARD else None, slices.get(name))
    return ho, hg


def _graph(sizes, extra_rows=0):
    """(what ops.graph_norm reads of an EdgeGraph, ptr list): mol_ptr / batch int32 on the GPU; extra_rows > 0 appends a
    trailing phantom graph that owns that many further rows (0: none)"""
    sizes = list(sizes) + ([extra_rows] if extra_rows else [])
    ptr = [0]
    for s in sizes:
        ptr.append(ptr[-1] + s)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    dev = _dev()
    g = SimpleNamespace(mol_ptr=torch.tensor(ptr, dtype=torch.int32, device=dev),
                        batch=batch.to(torch.int32).to(dev), num_graphs=len(sizes))
    return g, ptr


def _params(seg, shift):
    nw = sum(mul for mul, _ in seg.segs)
    nb = sum(mul for s, (mul, _) in enumerate(seg.segs) if seg.scalar(s))
    wsl, off = [], 0
    for mul, _ in seg.segs:
        wsl.append(slice(off, off + mul))
        off += mul
    w, b = _randn((nw,), 60) * 0.5 + 1.0, _randn((nb,), 61)
    if shift == "ones":
        ms = torch.ones(nb, dtype=torch.float64)
    elif shift == "uniform":
        ms = fo.f32r(torch.rand(nb, generator=torch.Generator().manual_seed(62), dtype=torch.float64) + 0.5)
    else:
        ms = None
    return ms, w, b, wsl


def _input(family, ptr, seg, seed, offset=100.0):
    n = ptr[-1]
    x = _randn((n, seg.dim), seed)
    if family == "randn+offset":
        x = fo.f32r(x + offset)
    elif family == "identical":
        # every second graph (the odd ones: 2, 64 and 3 nodes in the ragged set): all nodes equal to its first node.  The
        # other graphs keep the parameter gradients away from an all-zero reference, which no relative metric can judge.
        for g in range(1, len(ptr) - 1, 2):
            if ptr[g + 1] > ptr[g]:
                x[ptr[g]:ptr[g + 1]] = x[ptr[g]]
    return x


def _slices(seg, wsl):
    rs = seg.slices()
    return {"y": rs, "xsum": rs, "dx": rs, "da": rs, "db": rs, "d_weight": wsl, "d_bias": [slice(None)],
            "d_mean_shift": [slice(None)]}


@pytest.mark.parametrize("sizes", list(SIZES))
@pytest.mark.parametrize("irr", IRREPS)
def test_graph_norm(irr, sizes):
    """y, dx, d_mean_shift, d_weight, d_bias of ops.graph_norm for every input family and mean-shift setting"""
    from equiformer_amd import ops
    seg = fo.Segs(irr)
    lay = _layout(seg)
    graph, ptr = _graph(SIZES[sizes])
    ck = _Checker("gn[%s,%s]" % (irr, sizes))
    for shift in SHIFTS:
        ms, w, b, wsl = _params(seg, shift)
        sl = _slices(seg, wsl)
        for fi, family in enumerate(FAMILIES):
            x = _input(family, ptr, seg, 70 + fi, OFFSETS[sizes])
            go = _randn((ptr[-1], seg.dim), 80 + fi)
            if ms is None:
                _run(ck, ["y", "dx", "d_weight", "d_bias"],
                     lambda t, ww, bb: ops.graph_norm(t, None, ww, bb, lay, graph, EPS),
                     lambda t, ww, bb: fn.instance_norm(t, ww, bb, seg, ptr, EPS), [x, w, b], [go], sl)
            else:
                _run(ck, ["y", "dx", "d_mean_shift", "d_weight", "d_bias"],
                     lambda t, mm, ww, bb: ops.graph_norm(t, mm, ww, bb, lay, graph, EPS),
                     lambda t, mm, ww, bb: fn.graph_norm(t, mm, ww, bb, seg, ptr, EPS), [x, ms, w, b], [go], sl)
    ck.done()


@pytest.mark.parametrize("sizes", list(SIZES))
@pytest.mark.parametrize("irr", IRREPS)
def test_add_graph_norm(irr, sizes):
    """(xsum, y) = (a + b, norm(a + b)) with a cotangent flowing into xsum as well (the `dres` path of the backward)"""
    from equiformer_amd import ops
    seg = fo.Segs(irr)
    lay = _layout(seg)
    graph, ptr = _graph(SIZES[sizes])
    ck = _Checker("add_gn[%s,%s]" % (irr, sizes))
    for shift in SHIFTS:
        ms, w, b, wsl = _params(seg, shift)
        sl = _slices(seg, wsl)
        for fi, family in enumerate(FAMILIES):
            x = _input(family, ptr, seg, 90 + fi, OFFSETS[sizes])
            a1 = fo.f32r(0.25 * x)
            a2 = fo.f32r(x - a1)  # 0.25 x and 0.75 x are exact for identical rows: they stay identical
            gy, gs = _randn((ptr[-1], seg.dim), 100 + fi), _randn((ptr[-1], seg.dim), 110 + fi)

            def hip(p, q, *rest):
                mm = rest[0] if ms is not None else None
                s, y = ops.add_graph_norm(p, q, mm, rest[-2], rest[-1], lay, graph, EPS)
                return y, s

            if ms is None:
                _run(ck, ["y", "xsum", "da", "db", "d_weight", "d_bias"], hip,
                     lambda p, q, ww, bb: fn.add_instance_norm(p, q, ww, bb, seg, ptr, EPS), [a1, a2, w, b], [gy, gs], sl)
            else:
                _run(ck, ["y", "xsum", "da", "db", "d_mean_shift", "d_weight", "d_bias"], hip,
                     lambda p, q, mm, ww, bb: fn.add_graph_norm(p, q, mm, ww, bb, seg, ptr, EPS), [a1, a2, ms, w, b],
                     [gy, gs], sl)
    ck.done()


def _all_outputs(irr, sizes, extra_rows, shift, seed):
    """y, xsum and every gradient of ops.add_graph_norm on `sizes` (+ a trailing phantom graph of extra_rows rows whose
    inputs are random and whose cotangents are zero), float32 on the GPU; rows of the real graphs only"""
    from equiformer_amd import ops
    seg = fo.Segs(irr)
    lay = _layout(seg)
    n = sum(sizes)
    graph, ptr = _graph(sizes, extra_rows)
    ms, w, b, _ = _params(seg, shift)
    dev = _dev()

    def padded(t, fill):
        return torch.cat([t, fill((extra_rows, seg.dim))]) if extra_rows else t

    x = padded(_randn((n, seg.dim), seed), lambda s: _randn(s, seed + 1, 3.0))
    gy = padded(_randn((n, seg.dim), seed + 2), lambda s: torch.zeros(s, dtype=torch.float64))
    gs = padded(_randn((n, seg.dim), seed + 3), lambda s: torch.zeros(s, dtype=torch.float64))
    leaves = [t.float().to(dev).requires_grad_(True) if t is not None else None for t in (0.25 * x, 0.75 * x, ms, w, b)]
    s, y = ops.add_graph_norm(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], lay, graph, EPS)
    grads = torch.autograd.grad([y, s], [t for t in leaves if t is not None], [gy.float().to(dev), gs.float().to(dev)])
    rows = [y.detach()[:n], s.detach()[:n], grads[0][:n], grads[1][:n]]
    return rows, list(grads[2:])


@pytest.mark.parametrize("extra_rows", [0, 5, 70])
@pytest.mark.parametrize("irr", ["8x0e+4x1e+2x2e", "128x0e+64x1e+32x2e"])
def test_trailing_phantom_graph_leaves_the_real_rows_alone(irr, extra_rows):
    """what a padded (bucketed) batch does: a trailing phantom graph of extra rows with zero cotangents -- or an EMPTY
    phantom graph (extra_rows = 0: one more graph without rows) -- leaves y and dx of the real rows bit-identical and the
    parameter gradients equal to 1e-6 relative"""
    sizes = SIZES["ragged"]
    for shift in ("uniform", "instance"):
        rows0, par0 = _all_outputs(irr, sizes, 0, shift, 120)
        if extra_rows:
            rows1, par1 = _all_outputs(irr, sizes, extra_rows, shift, 120)
        else:
            rows1, par1 = _all_outputs(irr, sizes + [0], 0, shift, 120)
        for a, b in zip(rows0, rows1):
            assert torch.equal(a, b)
        for a, b in zip(par0, par1):
            assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max())


def test_two_identical_calls_are_bit_identical():
    """no atomics: outputs and every gradient repeat bit for bit"""
    for shift in ("uniform", "instance"):
        r0, p0 = _all_outputs("128x0e+64x1e+32x2e", SIZES["seventy"], 0, shift, 130)
        r1, p1 = _all_outputs("128x0e+64x1e+32x2e", SIZES["seventy"], 0, shift, 130)
        for a, b in zip(r0 + p0, r1 + p1):
            assert torch.equal(a, b)


def test_bad_arguments_return_an_error_code():
    """num_graphs <= 0 and null pointers are argument errors (-1), detected before anything is launched or read"""
    from equiformer_amd import lib
    h = lib.load()
    lay = _Layout("8x0e+4x1e")
    P = ctypes.c_void_p(64)  # never dereferenced: the checks come first
    fwd = lambda *a: h.eqf_graphnorm_fwd(*a, lay.c_ref, 1e-5, None)  # noqa: E731
    bwd = lambda *a: h.eqf_graphnorm_bwd(*a, lay.c_ref, None)  # noqa: E731
    for B in (0, -3):
        assert fwd(P, None, None, P, P, P, P, P, P, P, P, 4, B) == -1
        assert bwd(P, P, P, P, None, P, P, P, P, P, P, P, P, P, 4, B) == -1
    assert fwd(None, None, None, P, P, P, P, P, P, P, P, 4, 2) == -1          # x
    assert fwd(P, None, None, P, P, P, P, P, P, None, P, 4, 2) == -1          # mol_ptr
    assert fwd(P, None, None, P, P, P, P, P, P, P, None, 4, 2) == -1          # batch
    assert fwd(P, P, None, P, P, P, P, P, P, P, P, 4, 2) == -1                # x2 without xsum
    assert h.eqf_graphnorm_fwd(P, None, None, P, P, P, P, P, P, P, P, 4, 2, None, 1e-5, None) == -1  # irreps
    assert bwd(P, P, P, None, None, P, P, P, P, P, P, P, P, P, 4, 2) == -1    # dy
    assert bwd(P, P, P, P, None, P, P, P, P, P, P, P, P, None, 4, 2) == -1    # workspace
    assert bwd(P, P, P, P, None, P, P, P, P, P, P, None, P, P, 4, 2) == -1    # d_weight without d_bias
    assert bwd(P, None, P, P, None, P, P, P, P, P, P, P, P, P, 4, 2) == -1    # d_mean_shift without mean_shift
    with pytest.raises(lib.HipLibraryError):
        lib.call("eqf_graphnorm_fwd", None, None, None, None, None, None, None, None, None, None, None, 4, 2, None, 1e-5,
                 None)
