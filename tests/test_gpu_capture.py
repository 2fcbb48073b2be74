"""HIP-graph capture of a forward + backward that runs entirely through the C ABI of include/equiformer_hip.h.

The header promises that every entry point only ENQUEUES work on the caller's stream (no allocation, no synchronisation, no
host read-back), i.e. that the launches are legal inside a stream capture ("HIP-graph captured where possible";
VERDICT r4: the promise had no test).  Here a reduced QM9 model -- radius graph built beforehand: its edge count is the one
data-dependent size of the step -- is captured once (forward, L1 loss, backward into the parameters' .grad, grouped deferred
weight gradients included) and replayed: the replays must reproduce the eager gradients, also after the target buffer changed."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def test_forward_backward_captured_in_a_hip_graph_and_replayed():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd import ops
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    from equiformer_amd.synthetic import qm9_like_batch
    dev = torch.device("cuda:0")
    m = GraphAttentionTransformer(irreps_in="5x0e", max_radius=5.0, number_of_basis=32, **dict(mg.SMALL_L2, alpha_drop=0.0))
    m = fill_deterministic(m, 21).to(dev).train()
    d = {k: v.to(dev) for k, v in qm9_like_batch(6, 12, side=5.5, seed=9).items()}
    g = EdgeGraph.from_radius(d["pos"], d["batch"], 5.0)  # (host read-back of the edge count: outside the capture)
    target = d["y"].clone()
    params = [p for p in m.parameters() if p.requires_grad]

    def step():
        y = m(None, d["pos"], d["batch"], d["z"], graph=g)
        loss = (y.squeeze() - target).abs().mean()
        loss.backward()
        return loss

    def eager(t):
        target.copy_(t)
        for p in params:
            p.grad = None
        loss = step()
        torch.cuda.synchronize()
        return loss.detach().clone(), [None if p.grad is None else p.grad.detach().clone() for p in params]

    y1, y2 = d["y"].clone(), d["y"].flip(0).clone() * 1.5
    l1, g1 = eager(y1)
    l2, g2 = eager(y2)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture stream (allocator pools, lazily built tables, packed planes)
        for _ in range(2):
            for p in params:
                p.grad = None
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for p in params:
        p.grad = None
    target.copy_(y1)
    graph = torch.cuda.CUDAGraph()
    ops.deferred_weight_gradient_stats(reset=True)
    with torch.cuda.graph(graph):
        static_loss = step()
    assert ops.deferred_weight_gradient_stats()["queued"] > 0  # the grouped weight gradients were captured too
    static_grads = [p.grad for p in params]

    def replay(t):
        target.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        return static_loss.detach().clone(), [None if x is None else x.detach().clone() for x in static_grads]

    for t, (le, ge) in ((y1, (l1, g1)), (y2, (l2, g2)), (y1, (l1, g1))):
        lr, gr = replay(t)
        assert _rel(lr, le) < 1e-6
        n = 0
        for a, b in zip(gr, ge):
            assert (a is None) == (b is None)
            if b is not None and float(b.abs().max()) > 0:
                # atomically accumulated weight gradients differ in summation order from launch to launch
                assert _rel(a, b) < 2e-5
                n += 1
        assert n > 50


def _train_setup(alpha_drop, seed=21):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    from equiformer_amd.optim import FlatAdamW
    from equiformer_amd.synthetic import qm9_like_batch
    dev = torch.device("cuda:0")
    m = GraphAttentionTransformer(irreps_in="5x0e", max_radius=5.0, number_of_basis=32, **dict(mg.SMALL_L2, alpha_drop=alpha_drop))
    m = fill_deterministic(m, seed).to(dev).train()
    d = {k: v.to(dev) for k, v in qm9_like_batch(6, 12, side=5.5, seed=9).items()}
    opt = FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)
    return m, opt, d


def test_captured_train_step_with_optimizer_equals_eager_over_two_batches_of_one_shape():
    """equiformer_amd/capture.py: forward + L1 + backward + fused AdamW as one HIP graph per (nodes, edges) shape, the radius graph
    rebuilt outside it every step INTO the captured tensors.  Two batches of the same shape (the molecules of one in another
    order: other positions per node, another edge list, the same counts) alternate; parameters after 8 steps -- 3 eager ones,
    the capture, 4 replays -- equal those of 8 eager steps (dropout off; AdamW's step count and learning rate, changed between
    steps, reach the captured launch through the device words)."""
    from equiformer_amd.capture import CapturedTrainStep
    from equiformer_amd.graph import EdgeGraph
    results = []
    for use_graph in (False, True):
        m, opt, d = _train_setup(0.0)
        pos_a, z_a, y_a = d["pos"].clone(), d["z"].clone(), d["y"].clone()
        perm = torch.tensor([3, 0, 5, 1, 4, 2], device=pos_a.device)
        idx = (perm[:, None] * 12 + torch.arange(12, device=pos_a.device)[None]).reshape(-1)
        pos_b, z_b, y_b = pos_a[idx].clone(), z_a[idx].clone(), y_a[perm].clone()
        pos, z, y = pos_a.clone(), z_a.clone(), y_a.clone()  # the static input tensors

        def forward_loss(g):
            return (m(None, pos, d["batch"], z, graph=g).squeeze() - y).abs().mean()

        def build(into):
            return EdgeGraph.from_radius(pos, d["batch"], 5.0, num_graphs=6, into=into)
        cs = CapturedTrainStep(opt, forward_loss, min_eager=3)
        losses = []
        for it in range(8):
            src = (pos_a, z_a, y_a) if it % 2 == 0 else (pos_b, z_b, y_b)
            pos.copy_(src[0]), z.copy_(src[1]), y.copy_(src[2])
            for gr in opt.param_groups:
                gr["lr"] = 1e-3 * (1.0 + 0.1 * it)  # a schedule: the captured launch must see it
            if use_graph:
                loss = cs.step(build)
            else:
                opt.zero_grad(set_to_none=True)
                loss = forward_loss(build(None))
                loss.backward()
                opt.step()
            losses.append(float(loss))
        torch.cuda.synchronize()
        if use_graph:
            assert cs.replays == 5 and cs.eager_steps == 3, (cs.replays, cs.eager_steps)
        results.append((losses, opt.flat_p.detach().clone(), opt.flat_m.detach().clone(), opt._step))
    (le, pe, me, se), (lg, pg, mg_, sg) = results
    assert se == sg == 8
    for a, b in zip(le, lg):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(a)), (le, lg)
    # Atomically accumulated weight gradients differ in summation order from launch to launch: the moments agree to
    # that noise; the PARAMETERS agree where the gradient is above it -- Adam's m / (sqrt(v) + eps) turns a noise-level gradient
    # into a full +-lr step of either sign, in two eager runs as well (measured: 7e-4 after the second eager step).
    assert _rel(mg_, me) < 5e-4, _rel(mg_, me)
    big = me.abs() > 1e-3 * me.abs().max()
    assert int(big.sum()) > 1000
    assert _rel(pg[big], pe[big]) < 1e-4, _rel(pg[big], pe[big])
    assert _rel(pg, pe) < 8 * 2e-3  # (nowhere more than the eight steps' learning rates apart)


def test_captured_step_draws_a_fresh_dropout_mask_at_every_replay():
    """alpha_drop > 0, learning rate 0 (the weights do not move): replays of the same batch must give DIFFERENT losses -- the
    mask seed of a captured launch is host seed + a device word the step rewrites before every replay."""
    from equiformer_amd.capture import CapturedTrainStep
    from equiformer_amd.graph import EdgeGraph
    m, opt, d = _train_setup(0.3)
    for gr in opt.param_groups:
        gr["lr"], gr["weight_decay"] = 0.0, 0.0

    def forward_loss(g):
        return (m(None, d["pos"], d["batch"], d["z"], graph=g).squeeze() - d["y"]).abs().mean()

    def build(into):
        return EdgeGraph.from_radius(d["pos"], d["batch"], 5.0, num_graphs=6, into=into)
    cs = CapturedTrainStep(opt, forward_loss, min_eager=2)
    losses = [float(cs.step(build)) for _ in range(8)]
    assert cs.replays == 6
    assert len({round(v, 7) for v in losses[2:]}) >= 5, losses


def test_captured_md17_force_loss_step_equals_eager():
    """BASELINE configs #3 / #4 are force-loss steps: forward, forces by a create_graph backward, loss, SECOND-order backward,
    AdamW.  The whole of it replays as one HIP graph (bench.py --workload md17_l2 / md17_l3); here two aspirin frames of the
    L_max = 2 model: loss trajectory and moments of 3 eager + 4 replayed steps against 7 eager ones."""
    from equiformer_amd import nets
    from equiformer_amd.capture import CapturedTrainStep
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW
    from equiformer_amd.synthetic import md17_aspirin_batch
    dev = torch.device("cuda:0")
    results = []
    for use_graph in (False, True):
        torch.manual_seed(0)
        m = nets.model_entrypoint("graph_attention_transformer_nonlinear_exp_l2_md17")(irreps_in="64x0e", radius=5.0, num_basis=32)
        m = m.to(dev).train()
        d = {k: v.to(dev) for k, v in md17_aspirin_batch(2, seed=3).items()}
        gen = torch.Generator().manual_seed(7)
        ty, tf = torch.randn(2, 1, generator=gen).to(dev), torch.randn(42, 3, generator=gen).to(dev)
        opt = FlatAdamW(m.parameters(), lr=5e-4, weight_decay=1e-6)

        def forward_loss(g):
            E, F = m(node_atom=d["z"], pos=d["pos"], batch=d["batch"], graph=g)
            return (E - ty).abs().mean() + 80.0 * (F - tf).norm(dim=1).mean()

        def build(into):
            return EdgeGraph.from_radius(d["pos"], d["batch"], 5.0, num_graphs=2, into=into)
        cs = CapturedTrainStep(opt, forward_loss, min_eager=3)
        losses = []
        for it in range(7):
            if use_graph:
                loss = cs.step(build)
            else:
                opt.zero_grad(set_to_none=True)
                loss = forward_loss(build(None))
                loss.backward()
                opt.step()
                loss = loss.detach()
            losses.append(float(loss))
        torch.cuda.synchronize()
        if use_graph:
            assert cs.replays == 4 and cs.eager_steps == 3
        results.append((losses, opt.flat_m.detach().clone()))
    (le, me), (lg, mg_) = results
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(a)), (le, lg)
    assert _rel(mg_, me) < 2e-3, _rel(mg_, me)
