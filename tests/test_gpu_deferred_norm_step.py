"""One QM9 train step (4 molecules x 18 atoms, the flagship model) with the grouped parameter-side launches against the same step
with every weight gradient computed at once (ops.set_deferred_weight_gradients(False)): the forward is the same launches, so loss
and energies are bit-equal; gradients differ only in the order of fp32 atomics and stay within the bound
tests/test_gpu_capture.py uses for eager against replay (2e-5 of the tensor's largest entry).  The captured-and-replayed step is
compared with eager steps by tests/test_gpu_capture.py itself, which runs the same queue."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def test_train_step_with_grouped_norm_gradients_equals_the_ungrouped_step():
    from equiformer_amd import ops
    from equiformer_amd.nets import graph_attention_transformer as gat
    from equiformer_amd.synthetic import qm9_like_batch
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    # the registered QM9 model with its attention dropout off: both steps must compute the same forward
    m = gat.GraphAttentionTransformer(**gat._l2_kwargs("5x0e", 5.0, 128, None, None, None, alpha_drop=0.0)).to(dev).train()
    with torch.no_grad():
        g = torch.Generator().manual_seed(5)
        for n, p in m.named_parameters():  # affine parameters away from (1, 0), so that their gradients are not special
            if n.endswith("affine_weight") or n.endswith("affine_bias"):
                p.add_(0.3 * torch.randn(p.shape, generator=g).to(dev))
    d = {k: v.to(dev) for k, v in qm9_like_batch(4, 18, side=6.5, seed=3).items()}
    params = [p for p in m.parameters() if p.requires_grad]
    names = [n for n, p in m.named_parameters() if p.requires_grad]

    def step(defer):
        prev = ops.set_deferred_weight_gradients(defer)
        ops.deferred_weight_gradient_stats(reset=True)
        try:
            for p in params:
                p.grad = None
            y = m(None, d["pos"], d["batch"], d["z"])
            loss = (y.squeeze() - d["y"]).abs().mean()
            loss.backward()
            torch.cuda.synchronize()
            stats = ops.deferred_weight_gradient_stats()
        finally:
            ops.set_deferred_weight_gradients(prev)
        return loss.detach().clone(), y.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in params], stats

    l0, y0, g0, s0 = step(False)
    l1, y1, g1, s1 = step(True)
    assert s0["queued"] == 0 and "norms_queued" not in s0
    assert s1["norms_queued"] >= 13 and s1["norm_flushes"] == 1 and s1["queued"] > 0, s1
    assert torch.equal(l0, l1) and torch.equal(y0, y1)
    worst, n_norm = 0.0, 0
    for n, a, b in zip(names, g1, g0):
        assert (a is None) == (b is None), n
        if b is not None and float(b.abs().max()) > 0:
            r = _rel(a, b)
            worst = max(worst, r)
            assert r < 2e-5, (n, r)
            n_norm += n.endswith("affine_weight") or n.endswith("affine_bias")
    print("FIG grouped against ungrouped step: worst gradient difference %.2e over %d tensors" % (worst, len(names)))
    assert n_norm >= 26
