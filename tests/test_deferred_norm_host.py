"""Host logic of the deferred (grouped) affine gradients of the layer norms (equiformer_amd/ops.py) on CPU: the library call and
the grouped launch are replaced by recorders, everything else is the product's own code (ops.layer_norm / ops.add_layer_norm,
their autograd Functions, the per-graph-task queue).  Queued under .backward(); computed at once under torch.autograd.grad,
create_graph and for a hooked parameter; a shared weight receives both contributions; an early flush launches only entries whose
.grad exists; a pass that dies takes its entries with it; the linear entries keep the format test_deferred_wgrad_host.py reads."""
import gc

import pytest
import torch

from equiformer_amd import ops
from equiformer_amd.layout import RowLayout


class _Rec:
    def __init__(self):
        self.calls = []     # (name, args) of every library call
        self.groups = []    # one list of (x, dy, rstd, mean0, layout, dw, db) per grouped norm launch
        self.lin = []       # grouped launches of the linears

    def bwd_calls(self):
        return [(n, a) for n, a in self.calls if n in ("eqf_layernorm_bwd", "eqf_add_layernorm_bwd")]


@pytest.fixture()
def rec(monkeypatch):
    r = _Rec()

    def call(name, *args):
        r.calls.append((name, args))

    monkeypatch.setattr(ops, "call", call)
    monkeypatch.setattr(ops, "_chk", lambda *ts: None)
    monkeypatch.setattr(ops, "_capturing", lambda: False)  # (the zero arena asks the GPU runtime)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_ln_wgrad_group", lambda descs, st: r.groups.append(list(descs)))
    monkeypatch.setattr(ops, "_lin_wgrad_descs", lambda x, dy, spec, tw, tb: [(tw.data_ptr(), tw.numel(), spec)])
    monkeypatch.setattr(ops, "_gemm_group", lambda descs, st: r.lin.append(list(descs)))
    prev = ops.set_deferred_weight_gradients(True)
    ops.deferred_weight_gradient_stats(reset=True)
    yield r
    ops.set_deferred_weight_gradients(prev)
    ops.deferred_weight_gradient_stats(reset=True)


LAY = RowLayout("8x0e+4x1e")


def _params():
    return torch.ones(12, requires_grad=True), torch.zeros(8, requires_grad=True)


def _x(seed=0):
    return torch.randn(5, LAY.dim, generator=torch.Generator().manual_seed(seed)).requires_grad_(True)


def _queued():
    gc.collect()
    return sum(len(q.norms) + len(q.entries) for q in ops._task_queues.values())


def _wgrad_ptrs(args, add):
    """(d_weight, d_bias) arguments of a recorded eqf_layernorm_bwd / eqf_add_layernorm_bwd call"""
    return (args[7], args[8]) if add else (args[6], args[7])


def test_queued_under_backward_and_aimed_at_the_tensor_that_is_grad(rec):
    w, b = _params()
    w2, b2 = _params()
    x = _x()
    s, y = ops.add_layer_norm(x, x * 0.5, w2, b2, LAY)
    (ops.layer_norm(y + s, w, b, LAY)).sum().backward()
    # both kernels ran without their second launch (null accumulators) ...
    bw = rec.bwd_calls()
    assert [n for n, _ in bw] == ["eqf_layernorm_bwd", "eqf_add_layernorm_bwd"]
    assert _wgrad_ptrs(bw[0][1], False) == (None, None) and _wgrad_ptrs(bw[1][1], True) == (None, None)
    # ... and ONE grouped launch took both norms, in backward order, into the memory of .grad itself
    assert len(rec.groups) == 1 and _queued() == 0 and len(ops._task_queues) == 0
    (g0, g1) = rec.groups[0]
    assert g0[4] is LAY and g0[5].data_ptr() == w.grad.data_ptr() and g0[6].data_ptr() == b.grad.data_ptr()
    assert g1[5].data_ptr() == w2.grad.data_ptr() and g1[6].data_ptr() == b2.grad.data_ptr()
    assert g0[5].numel() == 12 and g0[6].numel() == 8 and g0[0].shape == (5, LAY.dim) and g0[2].shape == (5, 2)
    st = ops.deferred_weight_gradient_stats()
    assert st["norms_queued"] == 2 and st["norm_flushes"] == 1 and st["queued"] == 0 and st["flushes"] == 0
    # a second pass: .grad exists now -> computed at once by the kernel's own second launch
    del rec.calls[:], rec.groups[:]
    ops.layer_norm(_x(1), w, b, LAY).sum().backward()
    (n, a), = rec.bwd_calls()
    assert _wgrad_ptrs(a, False)[0] is not None and _wgrad_ptrs(a, False)[1] is not None and not rec.groups


def test_not_queued_under_autograd_grad_create_graph_or_for_a_hooked_parameter(rec):
    w, b = _params()
    # torch.autograd.grad: the engine captures the gradient, AccumulateGrad does not run
    torch.autograd.grad(ops.layer_norm(_x(), w, b, LAY).sum(), [w, b])
    (n, a), = rec.bwd_calls()
    assert None not in _wgrad_ptrs(a, False) and not rec.groups and _queued() == 0
    # create_graph: the differentiable backward operator computes everything at once
    del rec.calls[:]
    s, y = ops.add_layer_norm(_x(), _x(1), w, b, LAY)
    (y.sum() + s.sum()).backward(create_graph=True)
    (n, a), = rec.bwd_calls()
    assert n == "eqf_layernorm_bwd" and None not in _wgrad_ptrs(a, False) and not rec.groups and _queued() == 0
    # a tensor hook on the weight: somebody reads the gradient during backward
    del rec.calls[:]
    w, b = _params()
    seen = []
    h = w.register_hook(lambda g: seen.append(g.data_ptr()))
    ops.layer_norm(_x(), w, b, LAY).sum().backward()
    h.remove()
    (n, a), = rec.bwd_calls()
    assert None not in _wgrad_ptrs(a, False) and seen and not rec.groups and _queued() == 0
    # the switch
    del rec.calls[:]
    w, b = _params()
    prev = ops.set_deferred_weight_gradients(False)
    ops.layer_norm(_x(), w, b, LAY).sum().backward()
    ops.set_deferred_weight_gradients(prev)
    (n, a), = rec.bwd_calls()
    assert None not in _wgrad_ptrs(a, False) and not rec.groups
    assert "norms_queued" not in ops.deferred_weight_gradient_stats()


def test_a_shared_weight_ends_with_both_contributions(rec, monkeypatch):
    """two norms with ONE weight and bias: the engine sums their two zero tensors out of place, .grad is a third tensor, and both
    queued launches accumulate into it (the recorder adds 1 and 2: nothing is overwritten, nothing lands in a dead tensor)"""
    def launch(descs, st):
        rec.groups.append(list(descs))
        for k, d in enumerate(descs):
            d[5].add_(k + 1.0)
            d[6].add_(10.0 * (k + 1))
    monkeypatch.setattr(ops, "_ln_wgrad_group", launch)
    w, b = _params()
    y = ops.layer_norm(ops.layer_norm(_x(), w, b, LAY), w, b, LAY)
    y.sum().backward()
    (group,) = rec.groups
    assert len(group) == 2
    assert all(d[5].data_ptr() == w.grad.data_ptr() and d[6].data_ptr() == b.grad.data_ptr() for d in group)
    assert torch.equal(w.grad, torch.full((12,), 3.0)) and torch.equal(b.grad, torch.full((8,), 30.0))


class _Lin(torch.autograd.Function):
    """CPU stand-in for ops._Linear, as in test_deferred_wgrad_host.py"""

    @staticmethod
    def forward(ctx, x, w, tag):
        ctx.save_for_backward(x, w)
        ctx.tag, ctx.w = tag, w
        return x @ w

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        assert ops._can_defer(ctx.w)
        dw = torch.zeros(w.numel())
        ops._defer_lin_wgrad(ctx.w, None, x, dy, ctx.tag, False, dw, None)
        return dy @ w.t(), dw.view_as(w), None


def test_early_flush_launches_only_entries_whose_grad_exists(rec):
    """the norm in the middle is flushed from a post-accumulate hook of a linear in front of it (in backward order), while the
    shared norm weight of the outer two still waits for its second contribution; the linear entries are the 8-tuples of before"""
    w, b = _params()        # shared by the first and the last norm
    wm, bm = _params()      # the middle norm
    v = torch.randn(LAY.dim, LAY.dim, requires_grad=True)
    for p in (w, b, wm, bm, v):
        p._eqf_flushes = True
    seen = []

    def hook(p):
        q = list(ops._task_queues.values())[0]
        seen.append(("before", len(q.entries), len(q.norms), [len(e) for e in q.entries]))
        ops.flush_deferred_weight_gradients()
        seen.append(("after", len(q.entries), len(q.norms)))

    h = v.register_post_accumulate_grad_hook(hook)
    y = ops.layer_norm(_x(), w, b, LAY)
    y = _Lin.apply(y, v, "v")
    y = ops.layer_norm(y, wm, bm, LAY)
    y = ops.layer_norm(y, w, b, LAY)
    y.sum().backward()
    h.remove()
    # when v's hook fires: the last and the middle norm are queued (2), the linear is queued (one 8-tuple).  wm / bm have been
    # accumulated, w / b have not: the early flush launches the linear and the middle norm, the shared one stays
    assert seen == [("before", 1, 2, [8]), ("after", 0, 1)]
    assert [len(g) for g in rec.groups] == [1, 2]
    assert rec.groups[0][0][5].data_ptr() == wm.grad.data_ptr()
    assert all(d[5].data_ptr() == w.grad.data_ptr() and d[6].data_ptr() == b.grad.data_ptr() for d in rec.groups[1])
    assert [[d[2] for d in g] for g in rec.lin] == [["v"]] and rec.lin[0][0][0] == v.grad.data_ptr()
    st = ops.deferred_weight_gradient_stats()
    assert (st["queued"], st["flushes"], st["norms_queued"], st["norm_flushes"]) == (1, 1, 3, 2)
    assert _queued() == 0


def test_a_pass_that_dies_takes_its_entries_with_it(rec):
    """the norm is queued, then a later node of the pass raises: nothing is launched then or later"""

    class Die(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.clone()

        @staticmethod
        def backward(ctx, dy):
            raise RuntimeError("backward dies here")

    w, b = _params()
    with pytest.raises(RuntimeError):
        ops.layer_norm(Die.apply(_x()), w, b, LAY).sum().backward()
    assert not rec.groups and _queued() == 0 and len(ops._task_queues) == 0
    w2, b2 = _params()
    ops.layer_norm(_x(), w2, b2, LAY).sum().backward()
    (group,) = rec.groups
    assert len(group) == 1 and group[0][5].data_ptr() == w2.grad.data_ptr()
