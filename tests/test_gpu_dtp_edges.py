"""The un-fused depth-wise tensor product (csrc/edge.hip: eqf_dtp_coupling_fwd / _bwd, eqf_dtp_fwd / _bwd) and the DTP-generating
GEMM operand behind eqf_dtp_linear_fwd / _wgrad (csrc/gemm.hip, A_DTP) against the float64 restatements of tests/fp64_tp.py
(coupling, product, reference = product -> per-segment linear); tables, edge counts and inputs: tests/dtp_edge_cases.py.

Covered.  Coupling and product on five tables -- 72 weights (one partial block of the forward), 480 weights (two blocks), the
degree-3 table with 288 input channels (the `ch += blockDim.x` stride of the backward runs twice), an E(3) table with odd
segments, and a table whose 8x3e input segment no path reads (`not table.in_covered`: dx there is the caller's zero prefill,
so that table's backward goes through ops.dtp and dx of the segment is asserted exactly zero) -- at E = 1, 2, 255, 257, with per-edge
weights and without, dM and dw each requested and not.  Every tensor of a C-ABI launch sits in a guarded buffer
(tests/sfc_edge_cases.py): inputs between NaN guard rows, outputs prefilled with NaN, guard rows bit-identical afterwards,
every result element finite.  dx and dw are bit-identical whatever else a launch writes; dM comes from LDS float atomics and
is only held to its bound.
dtp_linear forward, data gradient and weight gradient on three tables (K = 96 / 192 / 192, 128 / 256 / 288, and degree 3) with
consumers of N = 32, 64, 96, 160 channels per segment, at E on either side of one row tile per degree (ept = 64, 21, 12, 9 with
64-row tiles; 42, 25, 18 with the 128 x 32 tile of N <= 32) and of one weight-gradient split (8 (32 / d3) edges: 256, 80, 48, 32),
which also gives last tiles and last steps with fewer edges than ept.  The tile every launch reached is asserted from the names
the library's profiler reports (gemm_rows_<bm>x<bn>_dtp_kn, gemm_tn_<BM>x<BN>_dtp) against the dispatch arithmetic restated in
tests/dtp_edge_cases.py: 64x64, 64x128, 128x32 rows tiles and all four widths of launch_tn.
The N <= 32 scalar consumer: launch_rows<A_DTP> used to pick the 128 x 32 tile for a degree-0 segment of N <= 32 (128 edges per
tile, above the 64 the loader generates) and return EQF_E_UNSUPPORTED although ops.DtpLinearSpec.make had accepted the
operator; it now takes the 64 x 64 tile with the columns past N masked.  Checked here at the operator (N = 32 items) and in a
SeparableFCTP with a 32x0e+32x1e consumer, use_fused="legacy" against use_fused=False.

Metric: `fp64_ops.per_row_rel`, every row of every tensor (weight gradients: every row AND every column of every [K, N] block).
Bound = max(plain bound, 4 x the error of the SAME restatement in float32 on the CPU on the same inputs); plain bounds: M and out
5e-6, dx 1e-5, d_sh 2e-5, dM and dw 1e-5 (tests/test_gpu_ops.py::test_dtp_unfused); dtp_linear out 2e-6, gradients 5e-6
(tests/test_gpu_gemm_edges.py, exact-fp32 back end).  tests/test_fp64_ops.py shows that a wrong out_ch of one path and the
weights of the neighbouring channel miss these bounds by >= 10 x.

Measured on an MI355X, the worst FIG line (largest err / bound) per quantity of one run; err = the kernel, yard = the float32
restatement on the same inputs:
  coupling      M 7.69e-08 = yard (5e-06); d_sh 4.54e-07, yard 2.23e-07 (2e-05)  (degree-3 table, E = 257)
  product       out 1.76e-07 = yard (5e-06); dx 4.75e-07, yard 1.94e-07 (1e-05); dw 2.69e-07 = yard (1e-05);
                dM 6.88e-06 = yard -> bound 2.75e-05 (the table with the unread segment, E = 257, no w: 8 signed terms per
                element, rows compared per row); the other tables stay under the plain 1e-05
  dtp_linear    out 1.14e-06, yard 5.74e-07 -> bound 2.29e-06 (degree 3, N = 64); dx 7.30e-07, dM 8.11e-07, dw 8.94e-07 at their
                yardsticks (5e-06); dweight 1.08e-06, yard 5.92e-07 (5e-06; per row and per column of every block)
  N <= 32       every N = 32 item reached gemm_rows_64x64_dtp_kn (degree 0) and gemm_rows_128x32_dtp_kn (degrees 1-3)
  SeparableFCTP out bit-equal between "legacy" and False; dx 5.86e-06 (5e-05); parameter, sh and edge-scalar gradients <= 7.5e-06
No guard row changed, every result was finite.
Wall time: 73 tests in 11.6 s; the slowest items test_dtp_linear_edges[deg3-160] 1.1 s (22 edge counts + 2 without w) and the
first coupling item 1.2 s (library load and context).
Wall time of this file on an MI355X, one run each (pytest's figure): 10.5 s at the parent commit, 11.4 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py).
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dtp_edge_cases as dtc  # noqa: E402
import fp64_ops as fo  # noqa: E402
import fp64_tp as tp  # noqa: E402
from sfc_edge_cases import check_guarded, guarded  # noqa: E402
from test_gpu_gemm_edges import _prof  # noqa: E402
from test_gpu_op_edges import _Checker, _dev  # noqa: E402
from poison import poisoned_ops  # noqa: E402,F401  (every launch of this file runs on poisoned, guarded allocations)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_ops")]


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _in(t, dev):
    return guarded(t.shape[0], t.shape[1], t.float().to(dev), dev)


def _ptr(g):
    return None if g is None else g.ptr


@pytest.mark.parametrize("E", dtc.EDGES)
@pytest.mark.parametrize("name", sorted(dtc.TABLES))
def test_coupling_guarded(name, E):
    from equiformer_amd import lib
    dev = _dev()
    t, d = dtc.table(name), dtc.inputs(name, E)
    ck = _Checker("coupling[%s,E=%d]" % (name, E))
    (M_r,), (dsh_r,), (M_y,), (dsh_y,) = fo.yardstick(lambda sh: tp.coupling(t, sh), [d["sh"]], [d["cM"]])
    sh, cM = _in(d["sh"], dev), _in(d["cM"], dev)
    M, dsh = guarded(E, t.m_numel, "nan", dev), guarded(E, sh.mid.shape[1], "nan", dev)
    cg = t.cg(dev)
    lib.call("eqf_dtp_coupling_fwd", sh.ptr, ctypes.c_void_p(cg.data_ptr()), t.c_ref, M.ptr, E, _st())
    lib.call("eqf_dtp_coupling_bwd", cM.ptr, ctypes.c_void_p(cg.data_ptr()), t.c_ref, dsh.ptr, E, _st())
    ck.cmp("M", check_guarded(M, "M"), M_r, dtc.BOUNDS["M"], M_y)
    ck.cmp("d_sh", check_guarded(dsh, "d_sh"), dsh_r, dtc.BOUNDS["d_sh"], dsh_y)
    check_guarded(sh, "sh"), check_guarded(cM, "dM")
    ck.done()


@pytest.mark.parametrize("use_w", [True, False])
@pytest.mark.parametrize("E", dtc.EDGES)
@pytest.mark.parametrize("name", sorted(dtc.TABLES))
def test_product_guarded(name, E, use_w):
    from equiformer_amd import lib, ops
    dev = _dev()
    t, d = dtc.table(name), dtc.inputs(name, E)
    ck = _Checker("dtp[%s,E=%d,%s]" % (name, E, "w" if use_w else "no w"))
    ins = [d["x"], d["M"]] + ([d["w"]] if use_w else [])
    names = ["out", "dx", "dM"] + (["dw"] if use_w else [])
    ro, rg, yo, yg = fo.yardstick(lambda x, M, w=None: tp.product(t, x, M, w), ins, [d["go"]])
    ref = dict(zip(names, zip(ro + rg, yo + yg)))
    x, M, go = _in(d["x"], dev), _in(d["M"], dev), _in(d["go"], dev)
    w = _in(d["w"], dev) if use_w else None
    out = guarded(E, t.layout_out.dim, "nan", dev)
    lib.call("eqf_dtp_fwd", x.ptr, M.ptr, _ptr(w), t.c_ref, out.ptr, E, _st())
    ck.cmp("out", check_guarded(out, "out"), ref["out"][0], dtc.BOUNDS["out"], ref["out"][1])
    if t.in_covered:
        first = None
        for want_M, want_w in ((True, True), (True, False), (False, True), (False, False)):
            if want_w and not use_w:
                continue
            dx = guarded(E, t.layout_in.dim, "nan", dev)
            dM = guarded(E, t.m_numel, "nan", dev) if want_M else None
            dw = guarded(E, t.weight_numel, "nan", dev) if want_w else None
            lib.call("eqf_dtp_bwd", x.ptr, M.ptr, _ptr(w), t.c_ref, go.ptr, dx.ptr, _ptr(dw), _ptr(dM), E, _st())
            got = dict(dx=check_guarded(dx, "dx"), dM=check_guarded(dM, "dM") if want_M else None,
                       dw=check_guarded(dw, "dw") if want_w else None)
            for n, g in got.items():
                if g is not None:
                    ck.cmp(n, g, ref[n][0], dtc.BOUNDS[n], ref[n][1])
            if first is None:
                first = got
            else:
                assert torch.equal(got["dx"], first["dx"])
                assert got["dw"] is None or torch.equal(got["dw"], first["dw"])
    else:  # dx of the unread segment is the zero prefill of ops._dtp_bwd: the operator, not the bare launch
        ho, hg = fo.evaluate(lambda a, b, c=None: ops.dtp(a, b, c, t), ins, [d["go"]], torch.float32, device=dev)
        for n, g in zip(names, ho + hg):
            ck.cmp(n, g, ref[n][0], dtc.BOUNDS[n], ref[n][1])
        read = {p["in_off"] for p in t.paths}
        for (mul, l), off in zip(t.layout_in.segs, t.layout_in.offsets):
            if off not in read:
                assert float(hg[0][:, off:off + mul * (2 * l + 1)].abs().max()) == 0.0
    for g, what in ((x, "x"), (M, "M"), (go, "d_out")) + (((w, "w"),) if use_w else ()):
        check_guarded(g, what)
    ck.done()


def _wgrad_views(flat, sp):
    """the [K, N] blocks of a flat weight gradient, and their transposes: compared per row and per column"""
    out = []
    for (_, K, N, _), off in zip(sp.degs, sp.w_offs):
        b = flat.reshape(-1)[off:off + K * N].reshape(K, N)
        out += [b, b.t()]
    return out


def _expected_kernels(t, lay, E):
    rows, tn = set(), set()
    for (K, l3), par in zip(t.layout_out.segs, t.layout_out.par):
        j = lay.seg_index(l3, par)
        bm, bn, _ = dtc.tile_of(t, l3, par, lay.segs[j][0], E)
        rows.add("gemm_rows_%dx%d_dtp_kn" % (bm, bn))
        tn.add("gemm_tn_%dx%d_dtp" % dtc.tn_tile_of(K, lay.segs[j][0]))
    return rows, tn


@pytest.mark.parametrize("N", dtc.LIN_N)
@pytest.mark.parametrize("name", sorted(dtc.LIN_TABLES))
def test_dtp_linear_edges(name, N):
    """forward and weight gradient through the C ABI on guarded buffers (the flat weight gradient is accumulated: random prefill
    and sentinels, as [n / 32, 32] rows), all five results through ops.dtp_linear, at every E of dtc.lin_edges; without per-edge
    weights at the first and the last E"""
    from equiformer_amd import lib, ops
    dev = _dev()
    t, lay = dtc.table(name), dtc.consumer(name, N)
    spec = ops.DtpLinearSpec.make(t, lay)
    sp = dtc.sfc_like(t, lay)
    assert spec is not None and spec.weight_numel == sp.weight_numel
    assert [b[3] for b in spec.blocks] == sp.w_offs and [b[:3] for b in spec.blocks] == [g[:3] for g in sp.degs]
    ck = _Checker("dtp_linear[%s,N=%d]" % (name, N))
    names = ["out", "dx", "dM", "dw", "dweight"]
    seen_rows, seen_tn = set(), set()
    edges = dtc.lin_edges(t.lmax_sh)
    for E, use_w in [(e, True) for e in edges] + [(edges[0], False), (edges[-1], False)]:
        d = dtc.lin_inputs(name, N, E)
        ins = [d["x"], d["M"]] + ([d["w"]] if use_w else []) + [d["weight"], d["bias"]]
        nm = [n for n in names if use_w or n != "dw"]
        wrt = list(range(len(ins) - 1))
        ro, rg, yo, yg = fo.yardstick(dtc.lin_reference(name, N, use_w), ins, [d["go"]], wrt=wrt)

        def cmp(n, got, r, y):
            if n == "dweight":
                for gv, rv, yv in zip(_wgrad_views(got, sp), _wgrad_views(r, sp), _wgrad_views(y, sp)):
                    ck.cmp(n, gv, rv, dtc.LIN_BOUNDS[n], yv)
            else:
                ck.cmp(n, got, r, dtc.LIN_BOUNDS[n], y)

        # the operator
        if use_w:
            hip = lambda x, M, w, weight, bias: ops.dtp_linear(x, M, w, weight, bias, spec)  # noqa: E731
        else:
            hip = lambda x, M, weight, bias: ops.dtp_linear(x, M, None, weight, bias, spec)  # noqa: E731
        ho, hg = fo.evaluate(hip, ins, [d["go"]], torch.float32, device=dev, wrt=wrt)
        for n, g, r, y in zip(nm, ho + hg, ro + rg, yo + yg):
            cmp(n, g, r, y)
        # the two DTP-generating launches on guarded buffers
        x, M, go = _in(d["x"], dev), _in(d["M"], dev), _in(d["go"], dev)
        w = _in(d["w"], dev) if use_w else None
        weight, bias = d["weight"].float().to(dev), d["bias"].float().to(dev)
        out = guarded(E, lay.dim, "nan", dev)
        dwt = guarded(sp.weight_numel // 32, 32, "acc", dev, seed=E)
        Wl = ops._ptr_array((slot, weight.data_ptr() + 4 * off) for (_, _, _, off, _, _, slot) in spec.blocks)
        dWl = ops._ptr_array((slot, dwt.mid.data_ptr() + 4 * off) for (_, _, _, off, _, _, slot) in spec.blocks)
        prof = _prof(lambda: (lib.call("eqf_dtp_linear_fwd", x.ptr, M.ptr, _ptr(w), t.c_ref, Wl, ctypes.c_void_p(bias.data_ptr()),
                                       out.ptr, lay.c_ref, E, _st()),
                              lib.call("eqf_dtp_linear_wgrad", x.ptr, M.ptr, _ptr(w), t.c_ref, go.ptr, lay.c_ref, dWl, E, _st())),
                     "gemm_")
        rows, tn = _expected_kernels(t, lay, E)
        assert {k for k in prof if k.startswith("gemm_rows")} == rows, (E, sorted(prof), rows)
        assert {k for k in prof if k.startswith("gemm_tn")} == tn, (E, sorted(prof), tn)
        seen_rows |= rows
        seen_tn |= tn
        cmp("out", check_guarded(out, "out"), ro[0], yo[0])
        cmp("dweight", check_guarded(dwt, "dweight").float(), rg[-1], yg[-1])
        for g, what in ((x, "x"), (M, "M"), (go, "d_out")) + (((w, "w"),) if use_w else ()):
            check_guarded(g, what)
    # the tiles this item was meant to reach
    want_rows = {32: {"gemm_rows_64x64_dtp_kn", "gemm_rows_128x32_dtp_kn"}, 64: {"gemm_rows_64x64_dtp_kn"},
                 96: {"gemm_rows_64x128_dtp_kn"}, 160: {"gemm_rows_64x128_dtp_kn"}}[N]
    assert seen_rows == want_rows, seen_rows
    assert seen_tn == {"gemm_tn_%dx%d_dtp" % dtc.tn_tile_of(K, N) for K, _ in t.layout_out.segs}, seen_tn
    ck.done()


def test_separable_fctp_with_32_scalar_consumer_legacy_matches_unfused():
    """a SeparableFCTP whose consumer has 32 scalar channels: use_fused="legacy" (ops.dtp_linear, which the spec accepts) gives
    what use_fused=False (ops.dtp, then the linear) gives -- it used to raise HipLibraryError from forward.  Both are fp32
    evaluations of one function: the bounds are those tests/test_gpu_ops.py::test_separable_fctp_fused_and_unfused holds each to
    against the oracle (1e-5 forward, 5e-5 gradients), out and dx per row."""
    from equiformer_amd import ops
    from equiformer_amd.nets.layers import EdgeContext, SeparableFCTP
    dev = _dev()
    torch.manual_seed(12)
    irr, out_irr, E = "32x0e+32x1e+32x2e", "32x0e+32x1e", 301
    mod = SeparableFCTP(irr, dtc.SH[2], out_irr, [16, 64, 64], use_activation=False).to(dev)
    assert mod.fused_spec is not None and mod.lin.layout_out.segs == [(32, 0), (32, 1)]
    g = torch.Generator().manual_seed(13)
    x0 = torch.randn(E, mod.dtp.table.layout_in.dim, generator=g)
    sh0, es0, go = torch.randn(E, 9, generator=g), torch.rand(E, 16, generator=g), torch.randn(E, mod.lin.layout_out.dim, generator=g)
    res = {}
    for fused in ("legacy", False):
        xg, shg, esg = (v.to(dev).requires_grad_(True) for v in (x0, sh0, es0))
        with ops.matrix_mode("fp32"):  # the linear of the un-fused path in exact fp32 too, as the DTP-generating GEMM is
            y = mod(xg, EdgeContext(None, shg, esg), use_fused=fused)
        res[fused] = [y.detach()] + list(torch.autograd.grad(y, [xg, shg, esg] + list(mod.parameters()), go.to(dev)))
    ck = _Checker("sep_fctp[32x0e+32x1e,legacy vs unfused]")
    for i, (a, b) in enumerate(zip(res["legacy"], res[False])):
        if i < 2:
            ck.cmp("out" if i == 0 else "dx", a, b, 1e-5 if i == 0 else 5e-5)
        else:
            ck.cmp("grad%d" % i, a.reshape(1, -1), b.reshape(1, -1), 5e-5)
    ck.done()
    assert ops.DtpLinearSpec.make(mod.dtp.table, mod.lin.layout_out) is not None
