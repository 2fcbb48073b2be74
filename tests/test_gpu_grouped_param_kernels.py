"""The grouped parameter-side launches through the C ABI: eqf_layernorm_wgrad_group (the affine gradients of many layer norms in
one flat grid, csrc/rowops.hip) and eqf_segment_sum_pair (both adjoints of gather_add in one launch, csrc/edge.hip).

Norm group: every problem is compared with what eqf_layernorm_bwd accumulates for it alone and with the float64 restatement
tests/fp64_ops.py::layer_norm (the layer norm's restatement lives there; tests/fp64_norms.py holds the graph and instance
norms).  The bound is the one tests/test_gpu_ops.py::test_layer_norm states for d_weight and d_bias, 2e-5 of the largest entry:
the grouped kernel forms the same per-thread partial sums, only the order of its atomics differs.  Row counts 1, 63, 64, 65, 129
sit at the edges of the 64 rows a thread walks and of its chunks of 16.  Pair: bit-equal to two eqf_segment_sum launches."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ops as fo  # noqa: E402

pytestmark = pytest.mark.gpu

BOUND = 2e-5  # tests/test_gpu_ops.py::test_layer_norm, d_weight and d_bias
ROWS = (1, 63, 64, 65, 129)
IRREPS = ("128x0e+64x1e+32x2e", "512x0e", "24x0e+16x0o+8x1e+40x0e")  # the last: two 0e segments and a 0o segment
EXTRA = ("16x0e+8x1e", "8x0e+8x2e")  # with these a group has five layouts; one launch keeps the tables of four
CAP = 32  # problems per launch (LNG_MAXP in csrc/rowops.hip)


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


class _Problem:
    """one norm: inputs on the GPU, what the forward saved, the ungrouped kernel's gradients and the float64 ones"""

    def __init__(self, irr, rows, seed):
        from equiformer_amd import lib
        from equiformer_amd.ops import _p
        dev = _dev()
        seg = fo.Segs(irr)
        self.irr, self.rows, self.seg = irr, rows, seg
        self.c = lib.make_irreps(seg.segs, seg.par)
        nw = sum(mul for mul, _ in seg.segs)
        nb = sum(mul for s, (mul, _) in enumerate(seg.segs) if seg.scalar(s))
        n0 = max(1, sum(1 for s in range(len(seg.segs)) if seg.scalar(s)))
        g = torch.Generator().manual_seed(seed)
        x = fo.f32r(torch.randn(rows, seg.dim, generator=g, dtype=torch.float64) * 2 + 0.3)
        dy = fo.f32r(torch.randn(rows, seg.dim, generator=g, dtype=torch.float64))
        w = fo.f32r(torch.randn(nw, generator=g, dtype=torch.float64) * 0.5 + 1.0)
        b = fo.f32r(torch.randn(nb, generator=g, dtype=torch.float64))
        wr, br = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        self.dw64, self.db64 = torch.autograd.grad(fo.layer_norm(x, wr, br, seg, 1e-5), [wr, br], dy)
        self.x, self.dy = x.float().to(dev), dy.float().to(dev)
        wg, bg = w.float().to(dev), b.float().to(dev)
        y, dx = torch.empty_like(self.x), torch.empty_like(self.x)
        self.rstd = torch.empty(rows, len(seg.segs), device=dev)
        self.mean0 = torch.empty(rows, n0, device=dev)
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        lib.call("eqf_layernorm_fwd", _p(self.x), _p(wg), _p(bg), _p(y), _p(self.rstd), _p(self.mean0), rows,
                 ctypes.byref(self.c), 1e-5, st)
        self.dw1, self.db1 = torch.zeros(nw, device=dev), torch.zeros(nb, device=dev)
        lib.call("eqf_layernorm_bwd", _p(self.x), _p(wg), _p(self.dy), _p(self.rstd), _p(self.mean0), _p(dx), _p(self.dw1),
                 _p(self.db1), rows, ctypes.byref(self.c), st)
        torch.cuda.synchronize()

    def desc(self, d, dw, db):
        from equiformer_amd.ops import _p
        d.x, d.dy, d.rstd, d.mean0, d.d_weight, d.d_bias = (_p(self.x), _p(self.dy), _p(self.rstd), _p(self.mean0), _p(dw),
                                                           _p(db))
        d.rows, d.irreps = self.rows, ctypes.pointer(self.c)


_cache = {}


def _problem(irr, rows):
    """computed once, shared by the tests, never written to"""
    key = (irr, rows)
    if key not in _cache:
        _cache[key] = _Problem(irr, rows, 1000 + 7 * len(_cache))
    return _cache[key]


def _run_group(problems, targets=None):
    """one eqf_layernorm_wgrad_group call; problems: _Problem or None (a zero-row problem without any buffer);
    targets[i]: index of the problem whose accumulators problem i writes into (default: its own) -> [(dw, db) or None]"""
    from equiformer_amd import lib
    dev = _dev()
    outs = []
    for i, p in enumerate(problems):
        if p is None:
            outs.append(None)
        elif targets is not None and targets[i] != i:
            outs.append(outs[targets[i]])
        else:
            outs.append((torch.zeros_like(p.dw1), torch.zeros_like(p.db1)))
    arr = (lib.EqfLnWgradDesc * len(problems))()
    for d, p, o in zip(arr, problems, outs):
        if p is None:
            d.rows = 0
        else:
            p.desc(d, *o)
    lib.call("eqf_layernorm_wgrad_group", arr, len(problems), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return outs


def _check(p, dw, db, tag):
    figs = (_rel(dw, p.dw1), _rel(db, p.db1), _rel(dw, p.dw64), _rel(db, p.db64))
    print("FIG %s %s rows=%d: d_weight vs ungrouped %.2e, d_bias %.2e; vs fp64 %.2e, %.2e" % ((tag, p.irr, p.rows) + figs))
    assert all(f < BOUND for f in figs), (tag, p.irr, p.rows, figs)


@pytest.mark.parametrize("irr", IRREPS)
def test_one_problem_at_every_row_edge(irr):
    for rows in ROWS:
        p = _problem(irr, rows)
        _check(p, *_run_group([p])[0], "n=1")


@pytest.mark.parametrize("n", [2, 13, CAP + 8])
def test_mixed_group_with_a_zero_row_problem_in_the_middle(n):
    """layouts and row counts cycle at different periods, so every launch of the group mixes them.  n = 40: the first launch
    ends at the cap of 32 problems; the last five problems bring a fourth and a fifth layout, and the fifth starts a third launch"""
    irr = lambda i: IRREPS[i % len(IRREPS)] if i < CAP + 3 else EXTRA[i % len(EXTRA)]  # noqa: E731
    problems = [_problem(irr(i), ROWS[(i * 2 + i // len(IRREPS)) % len(ROWS)]) for i in range(n)]
    problems.insert(n // 2, None)
    outs = _run_group(problems)
    assert outs[n // 2] is None
    for p, o in zip(problems, outs):
        if p is not None:
            _check(p, *o, "n=%d" % n)


def test_two_norms_that_share_their_parameters_accumulate():
    a, b, c = _problem(IRREPS[0], 129), _problem(IRREPS[0], 65), _problem(IRREPS[1], 64)
    outs = _run_group([a, c, b], targets=[0, 1, 0])
    dw, db = outs[0]
    for got, r1, r64 in ((dw, a.dw1 + b.dw1, a.dw64 + b.dw64), (db, a.db1 + b.db1, a.db64 + b.db64)):
        assert _rel(got, r1) < BOUND and _rel(got, r64) < BOUND, (_rel(got, r1), _rel(got, r64))
    _check(c, *outs[1], "between the sharing pair")


def test_group_argument_errors():
    from equiformer_amd import lib
    st = ctypes.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    assert lib.load().eqf_layernorm_wgrad_group(None, 0, st) == 0
    assert lib.load().eqf_layernorm_wgrad_group(None, 2, st) == -1
    arr = (lib.EqfLnWgradDesc * 1)()
    arr[0].rows = 5  # rows without buffers
    assert lib.load().eqf_layernorm_wgrad_group(arr, 1, st) == -1


# ------------------------------------------------------------------------------------------------- eqf_segment_sum_pair
def _degrees(E, N=40):
    """in-degrees of N nodes that sum to E, several of them zero"""
    g = torch.Generator().manual_seed(E)
    deg = [0] * N
    live = torch.randperm(N, generator=g)[:max(1, min(E, N - 9))].tolist()
    for e in range(E):
        deg[live[int(torch.randint(0, len(live), (1,), generator=g))]] += 1
    return deg


@pytest.mark.parametrize("D", [3, 480])
@pytest.mark.parametrize("E", [1, 333])
def test_segment_sum_pair_is_bit_equal_to_two_launches(E, D):
    from equiformer_amd import lib
    from equiformer_amd.ops import _p
    dev = _dev()
    N = 40
    deg = _degrees(E, N)
    graph = fo.ragged_graph(deg, 29, 5 + E, device=dev)  # sources among the first 29 nodes: 11 nodes send nothing
    assert graph.E == E and sum(1 for d in deg if d == 0) >= 9
    x = torch.randn(E, D, generator=torch.Generator().manual_seed(D), dtype=torch.float32).to(dev)
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ra, rb, pa, pb = (torch.full((N, D), float("nan"), device=dev) for _ in range(4))
    lib.call("eqf_segment_sum", _p(x), _p(graph.src_ptr), _p(graph.src_perm), _p(ra), N, D, 1.0, 0, st)
    lib.call("eqf_segment_sum", _p(x), _p(graph.row_ptr), None, _p(rb), N, D, 1.0, 0, st)
    lib.call("eqf_segment_sum_pair", _p(x), _p(graph.src_ptr), _p(graph.src_perm), _p(pa), _p(graph.row_ptr), None, _p(pb),
             N, D, st)
    torch.cuda.synchronize()
    assert torch.isfinite(ra).all() and torch.isfinite(rb).all()
    assert torch.equal(pa, ra) and torch.equal(pb, rb)
    assert float(ra.abs().sum()) > 0 and not torch.equal(ra, rb)


def test_gather_add_backward_takes_the_pair_launch():
    """ops.gather_add's backward with both gradients wanted (the paired launch) against the float64 adjoints.  Bound: a node
    sums at most ~30 fp32 terms of unit scale, 30 x 2^-24 = 1.8e-6 of the largest entry at worst."""
    from equiformer_amd import ops
    dev = _dev()
    N, D = 40, 480
    graph = fo.ragged_graph(_degrees(333, N), 29, 338, device=dev)
    g = torch.Generator().manual_seed(11)
    a, b = (fo.f32r(torch.randn(N, D, generator=g, dtype=torch.float64)) for _ in range(2))
    go = fo.f32r(torch.randn(333, D, generator=g, dtype=torch.float64))
    ar, br = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ref = torch.autograd.grad(fo.gather_add(ar, br, graph.src.cpu().long(), graph.dst.cpu().long()), [ar, br], go)
    ag, bg = a.float().to(dev).requires_grad_(True), b.float().to(dev).requires_grad_(True)
    got = torch.autograd.grad(ops.gather_add(ag, bg, graph), [ag, bg], go.float().to(dev))
    for h, r in zip(got, ref):
        assert _rel(h, r) < 2e-6, _rel(h, r)
