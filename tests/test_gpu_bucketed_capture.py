"""Shape-bucketed captured train step (equiformer_amd/capture.py BucketedTrainStep) on the GPU: a batch padded to its bucket's
capacity with one phantom molecule (csrc/graph.hip eqf_graph_pad_tail, EdgeGraph.from_radius(capacity=)) gives the real rows
the unpadded step gives, and one HIP graph per bucket trains as the eager, unpadded loop does -- for batches whose node and edge
counts change every step.  Tolerances of the trajectory comparisons are those of tests/test_gpu_capture.py."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 5.0
NODE_STEP, EDGE_STEP = 16, 128  # small-test buckets (the molecules here have 60-90 nodes and 450-950 edges per batch)


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _dev(d):
    dev = torch.device("cuda:0")
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def _model(cfg="SMALL_L2", alpha_drop=0.0, seed=21):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    m = GraphAttentionTransformer(irreps_in="5x0e", max_radius=R, number_of_basis=32, **dict(getattr(mg, cfg), alpha_drop=alpha_drop))
    return fill_deterministic(m, seed).to(torch.device("cuda:0")).train()


def _varying(n=20):
    """20 different batches of 6 molecules of 9-15 atoms: three buckets at steps of 16 nodes / 128 edges."""
    from equiformer_amd.synthetic import qm9_like_varying_batches
    return [_dev(d) for d in qm9_like_varying_batches(n, 6, (9, 15), side=5.5, seed=0)]


def _unpadded_loss(m, d):
    from equiformer_amd.graph import EdgeGraph
    g = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=d["num_graphs"])
    return (m(None, d["pos"], d["batch"], d["z"], graph=g).squeeze(-1) - d["y"]).abs().mean()


def _padded_loss(m):
    def forward_loss(g, v):
        return (m(None, v.pos, v.batch, v.z, graph=g).squeeze(-1)[:v.B] - v.y[:v.B]).abs().mean()
    return forward_loss


def _key(d):
    from equiformer_amd.capture import bucket_of
    from equiformer_amd.graph import EdgeGraph
    g = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=d["num_graphs"])
    return bucket_of(d["num_graphs"], g.N, g.E, NODE_STEP, EDGE_STEP)


# ------------------------------------------------------------------------------------------------------------------ the padded graph
def _check_padded(g, g0, pos_real, N, E, n_cap, e_cap, B):
    """every bullet of the kernel's contract, on the host with plain torch"""
    assert (g.N, g.E, g.num_graphs, g.n_real, g.e_real, g.num_real_graphs) == (n_cap, e_cap, B + 1, N, E, B)
    row_ptr, src, dst = g.row_ptr.cpu().long(), g.src.cpu().long(), g.dst.cpu().long()
    assert row_ptr.shape == (n_cap + 1,) and src.shape == dst.shape == (e_cap,)
    # the real part is the unpadded graph
    assert torch.equal(g.row_ptr[:N + 1], g0.row_ptr) and torch.equal(g.src[:E], g0.src) and torch.equal(g.dst[:E], g0.dst)
    assert torch.equal(g.batch[:N], g0.batch) and torch.equal(g.mol_ptr[:B + 1], g0.mol_ptr)
    P, Q = n_cap - N, e_cap - E
    ts, td = src[E:], dst[E:]
    assert int(row_ptr[n_cap]) == e_cap and bool((row_ptr[1:] >= row_ptr[:-1]).all())
    if Q:
        assert int(ts.min()) >= N and int(ts.max()) < n_cap and int(td.min()) >= N and int(td.max()) < n_cap  # range
        assert bool((td[1:] >= td[:-1]).all())  # sorted by destination
        assert bool((ts != td).all())  # no self-loop
        assert torch.unique(ts * n_cap + td).numel() == Q  # no repeated pair
    deg = torch.bincount(td - N, minlength=P) if P else torch.zeros(0, dtype=torch.long)
    assert torch.equal(row_ptr[N:], E + torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)]))  # CSR offsets = the degrees' scan
    if P:
        assert int(deg.max()) - int(deg.min()) <= 1  # no straggler row
    # sources ascend inside a row, as the radius graph's do
    same_row = td[1:] == td[:-1]
    assert bool((ts[1:][same_row] > ts[:-1][same_row]).all())
    assert bool((g.batch[N:] == B).all()) and int(g.mol_ptr[B + 1]) == n_cap
    pos = g.pos.cpu()
    assert torch.equal(pos[:N], pos_real.cpu())
    assert bool(torch.isfinite(pos).all())
    if P > 1:
        assert float(torch.cdist(pos[N:].double(), pos[N:].double()).add(torch.eye(P, dtype=torch.float64) * 10).min()) > 0.5  # distinct
    if Q:
        assert float((pos[ts] - pos[td]).norm(dim=1).min()) > 0.5  # every phantom edge vector is non-zero
    if g.z is not None:
        assert bool((g.z[N:] == 1).all())
    assert torch.equal(g.node_mask.cpu(), (torch.arange(n_cap) < N).float())
    assert torch.equal(g.graph_mask.cpu(), (torch.arange(B + 1) < B).float())
    # by-source view over all B + 1 molecules
    perm, sptr = g.src_perm.cpu().long(), g.src_ptr.cpu().long()
    assert torch.equal(torch.sort(perm).values, torch.arange(e_cap))
    s_sorted = src[perm]
    assert bool((s_sorted[1:] >= s_sorted[:-1]).all())
    same_src = s_sorted[1:] == s_sorted[:-1]
    assert bool((perm[1:][same_src] > perm[:-1][same_src]).all())  # stable
    assert torch.equal(sptr, torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(src, minlength=n_cap).cumsum(0)]))


def test_padded_graph_is_well_formed():
    from equiformer_amd.capture import bucket_of
    from equiformer_amd.graph import EdgeGraph, GraphDoesNotFit, min_phantom_nodes
    from equiformer_amd.synthetic import qm9_like_batch
    for atoms, seed in ((10, 1), (12, 9), (14, 3)):
        d = _dev(qm9_like_batch(6, atoms, side=5.5, seed=seed))
        g0 = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=6)
        N, E = g0.N, g0.E
        _, nb, eb = bucket_of(6, N, E, NODE_STEP, EDGE_STEP)
        caps = [(N, E), (N + 3, E),            # Q = 0, without and with phantom nodes
                (N + 2, E + 1),                # Q = 1
                (N + 5, E + 20),               # the largest Q five phantom nodes allow: every ordered pair
                (N + 7, E + 5),                # fewer edges than phantom nodes: rows without edges
                (N + 9, E + 31),               # degrees that differ by one
                (nb, eb),                      # the batch's own bucket
                (nb, E + (nb - N) * (nb - N - 1))]  # the largest Q the bucket's nodes allow
        for n_cap, e_cap in caps:
            for z in (d["z"], None):
                g = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=6, capacity=(n_cap, e_cap), z=z)
                _check_padded(g, g0, d["pos"], N, E, n_cap, e_cap, 6)
                if z is not None:
                    assert torch.equal(g.z[:N], d["z"])
        # does not fit: too few phantom nodes for the phantom edges; fewer edges than the batch has -- `into` stays as it was
        g = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=6, capacity=(nb, eb), z=d["z"])
        before = [t.clone() for t in (g.row_ptr, g.src, g.dst, g.src_perm, g.src_ptr, g.pos, g.batch, g.mol_ptr)]
        for cap in ((N + 2, E + 3), (N + 40, E - 1), (N - 1, E), (N + min_phantom_nodes(50) - 1, E + 50)):
            with pytest.raises(GraphDoesNotFit):
                EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=6, capacity=cap, into=g, z=d["z"])
        for a, b in zip(before, (g.row_ptr, g.src, g.dst, g.src_perm, g.src_ptr, g.pos, g.batch, g.mol_ptr)):
            assert torch.equal(a, b)
        # capacity=None is the unpadded path
        g1 = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=6, capacity=None)
        assert torch.equal(g1.src, g0.src) and torch.equal(g1.src_perm, g0.src_perm) and not hasattr(g1, "node_mask")


def test_into_reuses_the_tensors_of_a_bucket_for_another_real_shape():
    from equiformer_amd.graph import EdgeGraph
    batches = _varying()
    keys = [_key(d) for d in batches]
    key = max(set(keys), key=keys.count)
    a, b = [d for d, k in zip(batches, keys) if k == key][:2]
    ga0 = EdgeGraph.from_radius(a["pos"], a["batch"], R, num_graphs=6)
    gb0 = EdgeGraph.from_radius(b["pos"], b["batch"], R, num_graphs=6)
    assert (ga0.N, ga0.E) != (gb0.N, gb0.E)
    names = ("row_ptr", "src", "dst", "src_perm", "src_ptr", "batch", "mol_ptr", "pos", "z", "node_mask", "graph_mask")
    g = EdgeGraph.from_radius(a["pos"], a["batch"], R, num_graphs=6, capacity=key[1:], z=a["z"])
    ptrs = [getattr(g, n).data_ptr() for n in names]
    g2 = EdgeGraph.from_radius(b["pos"], b["batch"], R, num_graphs=6, capacity=key[1:], into=g, z=b["z"])
    assert g2 is g and [getattr(g2, n).data_ptr() for n in names] == ptrs
    fresh = EdgeGraph.from_radius(b["pos"], b["batch"], R, num_graphs=6, capacity=key[1:], z=b["z"])
    for n in names:
        assert torch.equal(getattr(g2, n), getattr(fresh, n)), n
    _check_padded(g2, gb0, b["pos"], gb0.N, gb0.E, key[1], key[2], 6)
    g3 = EdgeGraph.from_radius(a["pos"], a["batch"], R, num_graphs=6, capacity=key[1:], into=g, z=a["z"])
    assert g3 is g
    _check_padded(g3, ga0, a["pos"], ga0.N, ga0.E, key[1], key[2], 6)


# ------------------------------------------------------------------------------------------------------------------ model parity
@pytest.mark.parametrize("cfg", ["SMALL_L2", "SMALL_E3_L2"])
def test_model_parity_under_padding(cfg):
    """Energies [:B] and every parameter gradient of the padded run against the unpadded run, at the project's bar for model
    comparisons (1e-4 relative, the norm of tests/test_gpu_model.py); the phantom row is finite.
    Measured on an MI355X: energies bit-equal, parameter gradients within 3.6e-7 (both variants)."""
    from equiformer_amd.graph import EdgeGraph
    m = _model(cfg)
    params = [p for p in m.parameters() if p.requires_grad]
    worst_y = worst_g = 0.0
    for d in _varying(3):
        key = _key(d)
        B = d["num_graphs"]
        for p in params:
            p.grad = None
        g0 = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=B)
        y0 = m(None, d["pos"], d["batch"], d["z"], graph=g0).squeeze(-1)
        (y0 - d["y"]).abs().mean().backward()
        grads0 = [None if p.grad is None else p.grad.detach().clone() for p in params]
        for cap in (key[1:], (key[1] + 7, key[2] + 33)):
            for p in params:
                p.grad = None
            g = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=B, capacity=cap, z=d["z"])
            y = m(None, g.pos, g.batch, g.z, graph=g).squeeze(-1)
            assert y.shape == (B + 1,) and bool(torch.isfinite(y).all())
            (y[:B] - d["y"]).abs().mean().backward()
            worst_y = max(worst_y, _rel(y[:B], y0))
            assert _rel(y[:B], y0) < 1e-4
            n = 0
            for p, a in zip(params, grads0):
                assert (p.grad is None) == (a is None)
                if a is None:
                    continue
                assert bool(torch.isfinite(p.grad).all())
                if float(a.abs().max()) > 0:
                    worst_g = max(worst_g, _rel(p.grad, a))
                    assert _rel(p.grad, a) < 1e-4, _rel(p.grad, a)
                    n += 1
                else:
                    assert float(p.grad.abs().max()) == 0.0
            assert n > 50
    print("%s: padded vs unpadded, worst rel err energies %.3e, parameter gradients %.3e" % (cfg, worst_y, worst_g))


# ------------------------------------------------------------------------------------------------------------------ training
def _train(batches, schedule, bucketed, alpha_drop=0.0, **kw):
    """len(schedule) steps over `batches` (cycled): eager unpadded steps (bucketed=False) or BucketedTrainStep.step."""
    from equiformer_amd.capture import BucketedTrainStep
    from equiformer_amd.optim import FlatAdamW
    m = _model(alpha_drop=alpha_drop)
    opt = FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)
    bs = BucketedTrainStep(opt, _padded_loss(m), R, node_step=NODE_STEP, edge_step=EDGE_STEP, **kw) if bucketed else None
    losses, live = [], []
    for it, lr in enumerate(schedule):
        d = batches[it % len(batches)]
        for gr in opt.param_groups:
            gr["lr"] = lr
        if bucketed:
            loss = bs.step(d)
            live.append(len(bs.live_graphs()))
        else:
            opt.zero_grad(set_to_none=True)
            loss = _unpadded_loss(m, d)
            loss.backward()
            opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return dict(losses=losses, p=opt.flat_p.detach().clone(), m=opt.flat_m.detach().clone(), step=opt._step, bs=bs, live=live)


def _assert_trains_as_eager(e, b, steps, max_lr):
    """the tolerances of test_captured_train_step_with_optimizer_equals_eager_over_two_batches_of_one_shape.  What separates two
    runs of the same steps is the summation order of the atomically accumulated weight gradients: Adam turns a noise-level
    gradient element into a full +-lr step of either sign (two eager runs differ likewise), so the drift of a trajectory grows
    with the learning rates it sums.  That test sums 1.08e-2 over its 8 steps; the trajectories here are longer, and their
    schedules are chosen to sum to no more than that, so that its tolerances mean here what they mean there."""
    assert e["step"] == b["step"] == steps
    worst = max(abs(x - y) / max(1.0, abs(x)) for x, y in zip(e["losses"], b["losses"]))
    big = e["m"].abs() > 1e-3 * e["m"].abs().max()
    print("bucketed vs eager over %d steps: losses %.3e, moments %.3e, parameters above noise %.3e, all parameters %.3e"
          % (steps, worst, _rel(b["m"], e["m"]), _rel(b["p"][big], e["p"][big]), _rel(b["p"], e["p"])))
    for x, y in zip(e["losses"], b["losses"]):
        assert abs(x - y) <= 2e-5 * max(1.0, abs(x)), (e["losses"], b["losses"])
    assert _rel(b["m"], e["m"]) < 5e-4, _rel(b["m"], e["m"])
    assert int(big.sum()) > 1000
    assert _rel(b["p"][big], e["p"][big]) < 1e-4, _rel(b["p"][big], e["p"][big])
    assert _rel(b["p"], e["p"]) < steps * 2 * max_lr


def test_varying_batches_train_as_eager_does():
    """20 different batches in 3 buckets, dropout off, a learning-rate schedule: one eager step and one capture per bucket, 17
    replays; losses, AdamW moments and parameters against 20 plain eager UNPADDED steps from the same initial weights."""
    batches = _varying(20)
    keys = [_key(d) for d in batches]
    assert len({(d["pos"].shape[0], k) for d, k in zip(batches, keys)}) > 3 and len(set(keys)) == 3, keys
    schedule = [3.5e-4 * (1.0 + 0.05 * it) for it in range(20)]  # (sums to 1.03e-2; every step's rate <= 2 x the base rate)
    e = _train(batches, schedule, False)
    b = _train(batches, schedule, True, min_eager=1)
    bs = b["bs"]
    assert bs.eager_steps == 3 and bs.replays == 17 and bs.captures == 3, (bs.eager_steps, bs.replays, bs.captures)
    assert bs.captures_of == {k: 1 for k in set(keys)}
    assert sorted(bs.live_graphs()) == sorted(set(keys))
    _assert_trains_as_eager(e, b, 20, 3.5e-4)


def _one_batch_per_bucket(n):
    batches = _varying(20)
    keys = [_key(d) for d in batches]
    picked = {}
    for d, k in zip(batches, keys):
        picked.setdefault(k, d)
    assert len(picked) >= n
    return [picked[k] for k in sorted(picked)][:n]


def test_alternating_shapes_keep_both_graphs():
    """Two buckets alternating for 10 steps: 2 eager steps, exactly 2 captures, 8 replays, both records alive at the end."""
    a, b = _one_batch_per_bucket(2)
    schedule = [5e-4] * 10
    e = _train([a, b], schedule, False)
    r = _train([a, b], schedule, True, min_eager=1)
    bs = r["bs"]
    assert bs.captures == 2 and bs.replays == 8 and bs.eager_steps == 2 and bs.evictions == 0
    assert sorted(bs.live_graphs()) == sorted({_key(a), _key(b)}) and len(bs.live_graphs()) == 2
    _assert_trains_as_eager(e, r, 10, 5e-4)


def test_max_graphs_is_honoured_by_evicting_the_least_recently_used():
    """max_graphs = 2, three buckets visited round-robin: never more than 2 live graphs, results still equal eager."""
    three = _one_batch_per_bucket(3)
    schedule = [5e-4] * 12
    e = _train(three, schedule, False)
    r = _train(three, schedule, True, min_eager=1, max_graphs=2)
    bs = r["bs"]
    assert max(r["live"]) == 2 and len(bs.live_graphs()) == 2
    assert bs.evictions > 0 and bs.replays + bs.eager_steps == 12 and bs.replays >= 2
    _assert_trains_as_eager(e, r, 12, 5e-4)


def test_dropout_fresh_mask_per_replay_and_real_edges_keep_their_draws():
    from equiformer_amd.capture import BucketedTrainStep
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW
    d = _varying(1)[0]
    key = _key(d)
    m = _model(alpha_drop=0.3)
    opt = FlatAdamW(m.parameters(), lr=0.0, weight_decay=0.0)
    # (1) same host seeds -> the layers draw the same mask seeds; the mask is indexed by edge * heads + head and the phantom edges
    # come last, so the padded eager loss is the unpadded eager loss
    torch.manual_seed(5)
    l0 = float(_unpadded_loss(m, d).detach())
    torch.manual_seed(6)
    l0_other = float(_unpadded_loss(m, d).detach())
    assert abs(l0 - l0_other) > 1e-4 * abs(l0)  # (dropout is on)
    g = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=6, capacity=key[1:], z=d["z"])
    torch.manual_seed(5)
    l1 = float((m(None, g.pos, g.batch, g.z, graph=g).squeeze(-1)[:6] - d["y"]).abs().mean().detach())
    assert abs(l1 - l0) <= 1e-6 * max(1.0, abs(l0)), (l0, l1)
    # (2) learning rate 0: replays of one batch differ by their masks only
    bs = BucketedTrainStep(opt, _padded_loss(m), R, node_step=NODE_STEP, edge_step=EDGE_STEP, min_eager=2)
    losses = [float(bs.step(d)) for _ in range(8)]
    assert bs.replays == 6 and bs.captures == 1
    assert len({round(v, 7) for v in losses[2:]}) >= 5, losses


def test_md17_force_loss_step_over_frames_with_different_edge_counts():
    """Aspirin two-frame batches whose edge counts differ, one bucket: 3 eager padded steps, one capture, 5 replays against 8
    eager unpadded steps, at the tolerances of test_captured_md17_force_loss_step_equals_eager."""
    from equiformer_amd import nets
    from equiformer_amd.capture import BucketedTrainStep, bucket_of
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW
    from equiformer_amd.synthetic import md17_aspirin_batch
    dev = torch.device("cuda:0")
    full = md17_aspirin_batch(8, jitter=0.05, seed=0)
    gen = torch.Generator().manual_seed(7)
    batches = []
    for i in range(4):
        sel = (full["batch"] >= 2 * i) & (full["batch"] < 2 * i + 2)
        batches.append(dict(pos=full["pos"][sel].to(dev), z=full["z"][sel].to(dev), batch=(full["batch"][sel] - 2 * i).to(dev),
                            num_graphs=2, y=torch.randn(2, 1, generator=gen).to(dev), f=torch.randn(42, 3, generator=gen).to(dev)))
    edges = [EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=2).E for d in batches]
    assert len(set(edges)) >= 2, edges
    assert len({bucket_of(2, 42, E, NODE_STEP, EDGE_STEP) for E in edges}) == 1
    results = []
    for bucketed in (False, True):
        torch.manual_seed(0)
        m = nets.model_entrypoint("graph_attention_transformer_nonlinear_exp_l2_md17")(irreps_in="64x0e", radius=R, num_basis=32)
        m = m.to(dev).train()
        opt = FlatAdamW(m.parameters(), lr=5e-4, weight_decay=1e-6)

        def forward_loss(g, v):
            E, F = m(node_atom=v.z, pos=v.pos, batch=v.batch, graph=g)
            return (E[:v.B] - v.y[:v.B]).abs().mean() + 80.0 * ((F - v.f).norm(dim=1) * v.node_mask).sum() / v.node_mask.sum()

        bs = BucketedTrainStep(opt, forward_loss, R, graph_targets=("y",), node_targets=("f",), min_eager=3,
                               node_step=NODE_STEP, edge_step=EDGE_STEP) if bucketed else None
        losses = []
        for it in range(8):
            d = batches[it % 4]
            if bucketed:
                loss = bs.step(d)
            else:
                opt.zero_grad(set_to_none=True)
                g = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=2)
                E, F = m(node_atom=d["z"], pos=d["pos"], batch=d["batch"], graph=g)
                loss = (E - d["y"]).abs().mean() + 80.0 * (F - d["f"]).norm(dim=1).mean()
                loss.backward()
                opt.step()
                loss = loss.detach()
            losses.append(float(loss))
        torch.cuda.synchronize()
        if bucketed:
            assert bs.eager_steps == 3 and bs.captures == 1 and bs.replays == 5, (bs.eager_steps, bs.captures, bs.replays)
        results.append((losses, opt.flat_m.detach().clone()))
    (le, me), (lg, mg_) = results
    print("md17 bucketed vs eager: losses %.3e, moments %.3e"
          % (max(abs(a - b) / max(1.0, abs(a)) for a, b in zip(le, lg)), _rel(mg_, me)))
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(a)), (le, lg)
    assert _rel(mg_, me) < 2e-3, _rel(mg_, me)
