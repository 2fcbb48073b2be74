"""The dot-product attention kernels (csrc/dpattn.hip: eqf_kv_split, eqf_kv_merge, eqf_dp_logits_fwd / _bwd) against the float64
restatements of tests/fp64_ops.py at the edges of their launch shapes; layouts and graphs: tests/dp_edge_cases.py.

Covered.  Ten head layouts (G = 1, 27, 32, 64 | 65, 192 | 193, 256; H = 1, 2, 3, 4, 5, 8; mul / H == 4; degree 3; odd parity) on
the ragged graph of fo.ATTN_DEGREES (E = 1180; rows of 0-9, 31-33, 62-69 and 127-130 edges, empty rows first, in the middle and
last) and on chains of E = 1, 3, 4, 5 edges (the forward serves four edges per workgroup).  Through the C ABI, every tensor in
a guarded buffer (tests/sfc_edge_cases.py: inputs between NaN guard rows, outputs prefilled with NaN, guard rows bit-identical
afterwards, every result element finite): k, v and the three forms of kv_merge ((k, v), (k, null), (null, v)) bit-exact;
logit; dq and dk together and each alone, dq of rows without edges exactly zero; a second identical launch bit-identical
(no atomics).  Through ops.kv_split / ops.dp_logits: the first-order autograd path on every layout, and on G = 65 and H = 3 the
second-order gradients through ops._DpLogitsBwd against the fp64 double backward of the restatement.  Refusals by status,
outputs still all NaN: G = 257 forward (the backward takes it), G = 1025 backward, (mul / H) % 4 != 0, H = 9, mul % H != 0, null
arguments.

Metric: `fp64_ops.per_row_rel`, every row of every tensor.  Bound 1e-5 (tests/test_gpu_dp_attention.py), now per row; for the
sums of many signed terms (logit, dq, and the second-order g_q and g_dlogit) max(1e-5, 4 x the error of the SAME restatement
in float32 on the CPU on the same inputs).  dk and g_k are single products: plain bound.  tests/test_fp64_ops.py shows that
exchanged heads, a segment's scale on another segment and exchanged keys and values miss these bounds by >= 10 x.

Measured on an MI355X, the worst FIG line (largest err / bound) per quantity of one run; err = the kernel, yard = the float32
restatement on the same inputs ("-": plain bound):
  C ABI, guarded   logit 2.19e-05, yard 1.08e-05 -> bound 4.33e-05 (G = 65, chain of 3 edges: one row's 260 signed products);
                   dq 5.29e-07, yard 4.35e-07 (1e-05; G = 256, ragged); dk 1.26e-07 (1e-05; G = 32, ragged); k, v and the
                   three merges bit-exact; no guard row changed
  ops, first order logit 2.56e-06, yard 1.51e-06 (1e-05; odd-parity layout); dq 5.29e-07, yard 5.01e-07; dkv 1.17e-07
  second order     g_dlogit 1.98e-05, yard 2.95e-05 -> bound 1.18e-04 (G = 65); g_q 3.61e-07, yard 3.04e-07; g_kv 1.19e-07;
                   dq 4.13e-07; dkv 5.27e-08 (H = 3)
  G = 257          backward dq and dk inside 1e-05 on the chain of 5 edges; the forward returns EQF_E_UNSUPPORTED
Wall time: 63 tests in 4.8 s; the slowest item 1.2 s (the first of the file: library load and context), every other <= 0.14 s.
Wall time of this file on an MI355X, one run each (pytest's figure): 4.5 s at the parent commit, 4.4 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py).
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dp_edge_cases as dpc  # noqa: E402
import fp64_ops as fo  # noqa: E402
from sfc_edge_cases import check_guarded, guarded  # noqa: E402
from test_gpu_op_edges import _Checker, _dev  # noqa: E402
from poison import poisoned_ops  # noqa: E402,F401  (every launch of this file runs on poisoned, guarded allocations)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_ops")]


def _setup(head_irr, H, kind):
    from equiformer_amd.layout import RowLayout
    dev = _dev()
    seg = fo.all_heads_layout(head_irr, H)
    lay = RowLayout(dpc.irreps_str(seg))
    assert lay.segs == seg.segs and lay.par == seg.par and lay.dim == seg.dim == 4 * dpc.groups(head_irr, H)
    graph = dpc.graph(kind, dev)
    return dev, seg, lay, graph, dpc.inputs(head_irr, H, graph.N, graph.E)


def _status(name, *args):
    from equiformer_amd import lib
    return getattr(lib.load(), name)(*args)


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ip(t):
    return ctypes.c_void_p(t.data_ptr())


def _f32(t, dev):
    return t.float().to(dev)


@pytest.mark.parametrize("kind", dpc.GRAPHS)
@pytest.mark.parametrize("head_irr,H", dpc.HEADS)
def test_dp_kernels_guarded(head_irr, H, kind):
    from equiformer_amd import lib
    dev, seg, lay, graph, d = _setup(head_irr, H, kind)
    N, E, D = graph.N, graph.E, seg.dim
    dst, row_ptr = graph.dst.long().cpu(), graph.row_ptr.long().cpu()
    ck = _Checker("dp[%s,H=%d,G=%d,%s]" % (head_irr, H, dpc.groups(head_irr, H), kind))
    # ---- split and merge: pure copies
    kv = guarded(E, 2 * D, _f32(d["kv"], dev), dev)
    k, v = guarded(E, D, "nan", dev), guarded(E, D, "nan", dev)
    lib.call("eqf_kv_split", kv.ptr, k.ptr, v.ptr, E, H, lay.c_ref, _st())
    k_r, v_r = fo.kv_split(d["kv"], seg, H)
    check_guarded(kv, "kv")
    assert torch.equal(check_guarded(k, "k").double(), k_r) and torch.equal(check_guarded(v, "v").double(), v_r)
    for use_k, use_v in ((True, True), (True, False), (False, True)):
        out = guarded(E, 2 * D, "nan", dev)
        lib.call("eqf_kv_merge", k.ptr if use_k else None, v.ptr if use_v else None, out.ptr, E, H, lay.c_ref, _st())
        want = fo.kv_merge(k_r if use_k else None, v_r if use_v else None, seg, H)
        assert torch.equal(check_guarded(out, "kv_merge %s %s" % (use_k, use_v)).double(), want)
    check_guarded(k, "k"), check_guarded(v, "v")
    # ---- logits
    q = guarded(N, D, _f32(d["q"], dev), dev)
    ref = {t: fo.evaluate(lambda a, b: fo.dp_logits(a, b, dst, seg, H), [d["q"], k_r], [d["cl"]], t)
           for t in (torch.float64, torch.float32)}
    (lg_r,), (dq_r, dk_r) = ref[torch.float64]
    (lg_y,), (dq_y, _) = ref[torch.float32]
    logit = [guarded(E, H, "nan", dev) for _ in range(2)]
    for lg in logit:
        lib.call("eqf_dp_logits_fwd", q.ptr, k.ptr, _ip(graph.dst), lg.ptr, E, H, lay.c_ref, _st())
    got = [check_guarded(lg, "logit") for lg in logit]
    assert torch.equal(got[0], got[1])
    ck.cmp("logit", got[0], lg_r, dpc.BOUND, lg_y)
    # ---- dq and dk: together, each alone
    dl = guarded(E, H, _f32(d["cl"], dev), dev)
    empty = (row_ptr[1:] == row_ptr[:-1])
    assert bool(empty.any())
    both = None
    for want_q, want_k, rep in ((True, True, 0), (True, True, 1), (True, False, 0), (False, True, 0)):
        dq = guarded(N, D, "nan", dev) if want_q else None
        dk = guarded(E, D, "nan", dev) if want_k else None
        lib.call("eqf_dp_logits_bwd", q.ptr if want_k else None, k.ptr if want_q else None, dl.ptr, _ip(graph.row_ptr),
                 dq.ptr if want_q else None, dk.ptr if want_k else None, N, H, lay.c_ref, _st())
        gq = check_guarded(dq, "dq") if want_q else None
        gk = check_guarded(dk, "dk") if want_k else None
        if both is None:
            both = (gq, gk)
            ck.cmp("dq", gq, dq_r, dpc.BOUND, dq_y)
            ck.cmp("dk", gk, dk_r, dpc.BOUND)
            assert float(gq[empty].abs().max()) == 0.0
        else:  # the same arithmetic whatever else the launch writes
            assert gq is None or torch.equal(gq, both[0])
            assert gk is None or torch.equal(gk, both[1])
    for g, what in ((q, "q"), (k, "k"), (dl, "d_logit")):
        check_guarded(g, what)
    ck.done()


@pytest.mark.parametrize("head_irr,H", dpc.HEADS)
def test_dp_autograd_first_order(head_irr, H):
    """ops.kv_split and ops.dp_logits on the ragged graph: (k, v, logit) and the gradients wrt (q, kv)"""
    from equiformer_amd import ops
    dev, seg, lay, graph, d = _setup(head_irr, H, "ragged")
    dst = graph.dst.long().cpu()
    ck = _Checker("dp_ops[%s,H=%d]" % (head_irr, H))

    def hip(q, kv):
        k, v = ops.kv_split(kv, H, lay)
        return k, v, ops.dp_logits(q, k, graph, H, lay)

    def ref(q, kv):
        k, v = fo.kv_split(kv, seg, H)
        return k, v, fo.dp_logits(q, k, dst, seg, H)

    gouts = [d["ck"], d["cv"], d["cl"]]
    ro, rg, yo, yg = fo.yardstick(ref, [d["q"], d["kv"]], gouts)
    ho, hg = fo.evaluate(hip, [d["q"], d["kv"]], gouts, torch.float32, device=dev)
    assert torch.equal(ho[0].double().cpu(), ro[0]) and torch.equal(ho[1].double().cpu(), ro[1])
    ck.cmp("logit", ho[2], ro[2], dpc.BOUND, yo[2])
    ck.cmp("dq", hg[0], rg[0], dpc.BOUND, yg[0])
    ck.cmp("dkv", hg[1], rg[1], dpc.BOUND)
    ck.done()


@pytest.mark.parametrize("head_irr,H", dpc.SECOND_ORDER)
def test_dp_second_order(head_irr, H):
    """(dq, dkv) with create_graph, then the gradients of <a, dq> + <b, dkv> wrt (q, kv, d_logit): ops._DpLogitsBwd.backward and
    the split / merge pair against the fp64 double backward of the restatement"""
    from equiformer_amd import ops
    dev, seg, lay, graph, d = _setup(head_irr, H, "ragged")
    dst = graph.dst.long().cpu()
    ck = _Checker("dp_2nd[%s,H=%d]" % (head_irr, H))

    def first(split, logits):
        def fn(q, kv, cl, cv):
            k, v = split(kv)
            return torch.autograd.grad([logits(q, k), v], [q, kv], [cl, cv], create_graph=True)
        return fn

    hip = first(lambda kv: ops.kv_split(kv, H, lay), lambda q, k: ops.dp_logits(q, k, graph, H, lay))
    ref = first(lambda kv: fo.kv_split(kv, seg, H), lambda q, k: fo.dp_logits(q, k, dst, seg, H))
    ins, gouts = [d["q"], d["kv"], d["cl"], d["cv"]], [d["a"], d["b"]]
    ro, rg, yo, yg = fo.yardstick(ref, ins, gouts, wrt=[0, 1, 2])
    ho, hg = fo.evaluate(hip, ins, gouts, torch.float32, device=dev, wrt=[0, 1, 2])
    ck.cmp("dq", ho[0], ro[0], dpc.BOUND, yo[0])
    ck.cmp("dkv", ho[1], ro[1], dpc.BOUND)
    ck.cmp("g_q", hg[0], rg[0], dpc.BOUND, yg[0])
    ck.cmp("g_kv", hg[1], rg[1], dpc.BOUND)
    ck.cmp("g_dlogit", hg[2], rg[2], dpc.BOUND, yg[2])
    ck.done()


def _all_nan(g):
    return bool(torch.isnan(g.buf).all())


def test_dp_refusals():
    """a refused call returns its status before any launch: the outputs keep their NaN prefill"""
    from equiformer_amd import lib
    from equiformer_amd.layout import RowLayout
    dev = _dev()
    graph = dpc.graph("chain5", dev)
    N, E = graph.N, graph.E

    def bufs(head_irr, H, row=False):  # row: the irreps are those of the whole q / k / v row
        seg = fo.Segs(head_irr) if row else fo.all_heads_layout(head_irr, H)
        lay = lib.make_irreps(seg.segs, seg.par)
        D = seg.dim
        z = lambda r, c: guarded(r, c, torch.zeros(r, c), dev)  # noqa: E731
        n = lambda r, c: guarded(r, c, "nan", dev)  # noqa: E731
        return dict(lay=ctypes.byref(lay), keep=lay, D=D, q=z(N, D), k=z(E, D), kv=z(E, 2 * D), dl=z(E, H), o_k=n(E, D), o_v=n(E, D),
                    o_kv=n(E, 2 * D), o_lg=n(E, H), o_dq=n(N, D), o_dk=n(E, D))

    def fwd(b, H, q=True, k=True, dst=True, out=True, lay=True):
        return _status("eqf_dp_logits_fwd", b["q"].ptr if q else None, b["k"].ptr if k else None,
                       _ip(graph.dst) if dst else None, b["o_lg"].ptr if out else None, E, H, b["lay"] if lay else None, _st())

    def bwd(b, H, q=True, k=True, dl=True, rp=True, lay=True):
        return _status("eqf_dp_logits_bwd", b["q"].ptr if q else None, b["k"].ptr if k else None, b["dl"].ptr if dl else None,
                       _ip(graph.row_ptr) if rp else None, b["o_dq"].ptr, b["o_dk"].ptr, N, H, b["lay"] if lay else None, _st())

    outs = ("o_k", "o_v", "o_kv", "o_lg", "o_dq", "o_dk")
    # G = 257: the forward refuses, the backward serves (and is right)
    head_irr, H = dpc.REFUSED_FWD
    assert dpc.groups(head_irr, H) == 257
    b = bufs(head_irr, H)
    assert fwd(b, H) == -2 and all(_all_nan(b[o]) for o in outs)
    seg = fo.all_heads_layout(head_irr, H)
    d = dpc.inputs(head_irr, H, N, E)
    qg, kg, dlg = (guarded(*t.shape, _f32(t, dev), dev) for t in (d["q"], d["ck"], d["cl"]))
    assert _status("eqf_dp_logits_bwd", qg.ptr, kg.ptr, dlg.ptr, _ip(graph.row_ptr), b["o_dq"].ptr, b["o_dk"].ptr, N, H, b["lay"],
                   _st()) == 0
    _, (dq_r, dk_r) = fo.evaluate(lambda x, y: fo.dp_logits(x, y, graph.dst.long().cpu(), seg, H), [d["q"], d["ck"]], [d["cl"]],
                                  torch.float64)
    ck = _Checker("dp[G=257,bwd]")
    ck.cmp("dq", check_guarded(b["o_dq"], "dq"), dq_r, dpc.BOUND)  # one edge per row: single products
    ck.cmp("dk", check_guarded(b["o_dk"], "dk"), dk_r, dpc.BOUND)
    ck.done()
    # G = 1025: the backward refuses
    head_irr, H = dpc.REFUSED_BWD
    assert dpc.groups(head_irr, H) == 1025
    b = bufs(head_irr, H)
    assert bwd(b, H) == -2 and fwd(b, H) == -2 and all(_all_nan(b[o]) for o in outs)
    # tables make_dptab refuses, in every entry point
    for head_irr, H in dpc.REFUSED_TAB:
        b = bufs(head_irr, H, row=True)
        assert fwd(b, H) == -2 and bwd(b, H) == -2
        assert _status("eqf_kv_split", b["kv"].ptr, b["o_k"].ptr, b["o_v"].ptr, E, H, b["lay"], _st()) == -2
        assert _status("eqf_kv_merge", b["k"].ptr, b["k"].ptr, b["o_kv"].ptr, E, H, b["lay"], _st()) == -2
        assert all(_all_nan(b[o]) for o in outs), (head_irr, H)
    # null arguments
    head_irr, H = dpc.HEADS[1]
    b = bufs(head_irr, H)
    for kw in (dict(q=False), dict(k=False), dict(dst=False), dict(out=False), dict(lay=False)):
        assert fwd(b, H, **kw) == -1, kw
    for kw in (dict(q=False), dict(k=False), dict(dl=False), dict(rp=False), dict(lay=False)):
        assert bwd(b, H, **kw) == -1, kw  # dq needs k, dk needs q
    assert _status("eqf_kv_split", None, b["o_k"].ptr, b["o_v"].ptr, E, H, b["lay"], _st()) == -1
    assert _status("eqf_kv_split", b["kv"].ptr, None, b["o_v"].ptr, E, H, b["lay"], _st()) == -1
    assert _status("eqf_kv_split", b["kv"].ptr, b["o_k"].ptr, None, E, H, b["lay"], _st()) == -1
    assert _status("eqf_kv_merge", b["k"].ptr, b["k"].ptr, None, E, H, b["lay"], _st()) == -1
    assert _status("eqf_kv_merge", b["k"].ptr, b["k"].ptr, b["o_kv"].ptr, E, H, None, _st()) == -1
    assert all(_all_nan(b[o]) for o in outs)
    # through ops: the error, not a fallback
    from equiformer_amd import ops
    head_irr, H = dpc.REFUSED_FWD
    lay = RowLayout(dpc.irreps_str(fo.all_heads_layout(head_irr, H)))
    with pytest.raises(lib.HipLibraryError, match="code -2"):
        ops.dp_logits(torch.zeros(N, lay.dim, device=dev), torch.zeros(E, lay.dim, device=dev), graph, H, lay)
