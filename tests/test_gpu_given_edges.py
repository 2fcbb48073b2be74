"""OC20 batches that bring their own periodic edge list (otf_graph=False) on the GPU:

1. EdgeGraph.from_edges_pbc (csrc/graph.hip eqf_edges_pbc_count / eqf_edges_pbc_fill) returns, integer for integer, what
   tests/given_edges_inputs.py states in pure torch (fp64 get_pbc_distances + stable sorts) and what the parent's path
   (EdgeGraph.from_edges on the kept edges) returns; the fp32 offsets are within 4 * 2^-24 * sum_k |n_k cell_kj| of the fp64
   product (three exactly representable integers, three rounded products, two additions: gamma_3 ~ 3u, the fourth u covers its
   denominator);
2. capacity= pads with one phantom structure;  3. into= refills in place, exact-shape and padded;  4. bad inputs raise;
5. the OC20 model on the new graph gives what `model(data)` under otf_graph=False gives;
6. CapturedTrainStep, BucketedTrainStep, IS2RSTrainStep and evaluate_oc20 with the batch's edges train / evaluate as the eager
   loop (trajectory bounds: tests/test_gpu_periodic_capture.py _assert_trains_as_eager, restated; evaluation: tests/test_gpu_eval_step.py).
Inputs: tests/given_edges_inputs.py (tests/test_given_edges.py shows on the CPU that they hold what they are meant to exercise)."""
import collections
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import given_edges_inputs as gi  # noqa: E402
import periodic_inputs as pi  # noqa: E402

R = pi.R
NODE_STEP, EDGE_STEP = 64, 1024
INT_NAMES = ("src", "dst", "row_ptr", "cell_offsets", "order", "src_perm", "src_ptr", "batch", "mol_ptr")
ALL_NAMES = INT_NAMES + ("offsets",)
PADDED_NAMES = ALL_NAMES + ("pos", "z", "node_mask", "graph_mask")
CASES = ("in order", "shuffled", "empty structure", "empty structure first", "empty structure last", "dropped", "truncated",
         "no edges")


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _to_dev(d):
    dev = _dev()
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def _build(d, **kw):
    """d: tensors on the GPU"""
    from equiformer_amd.graph import EdgeGraph
    return EdgeGraph.from_edges_pbc(d["pos"], d["cell"], d["batch"], d["edge_index"], d["cell_offsets"], d["neighbors"],
                                    num_graphs=d["cell"].shape[0], **kw)


def _by_source(src, N):
    perm = torch.argsort(src.long(), stable=True).to(torch.int32)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=src.device), torch.bincount(src.long(), minlength=N).cumsum(0)])
    return perm, ptr.to(torch.int32)


# ------------------------------------------------------------------------------------------------------------------ 1. the builder
@pytest.mark.parametrize("name", CASES)
def test_builder_equals_the_expectation_and_the_parents_path(name):
    from equiformer_amd.graph import EdgeGraph
    d, x = gi.cases()[name], gi.expected(name)
    dd = _to_dev(d)
    g, offsets, cell_off = _build(dd)
    N, B, E = d["pos"].shape[0], d["cell"].shape[0], int(x["src"].numel())
    assert (g.N, g.E, g.num_graphs) == (N, E, B) and g._pbc and g._radius_static and not getattr(g, "_padded", False)
    assert offsets is g.offsets and cell_off is g.cell_offsets
    for n in INT_NAMES:
        t = getattr(g, n)
        assert t.dtype == torch.int32 and t.device.type == "cuda", n
        assert torch.equal(t.cpu(), x[n]), (name, n)
    assert g.offsets.dtype == torch.float32 and g.offsets.shape == (E, 3)
    err = (g.offsets.cpu().double() - x["offsets"]).abs()
    if E:
        print("%s: N %d, %d of %d edges kept, offsets off by up to %.3e (worst ratio to the bound %.3f)"
              % (name, N, E, d["edge_index"].shape[1], float(err.max()),
                 float((err / x["offsets_bound"].clamp_min(1e-300))[x["offsets_bound"] > 0].max()) if bool((x["offsets_bound"] > 0).any()) else 0.0))
    assert bool((err <= x["offsets_bound"]).all()), name
    # the parent's path: EdgeGraph.from_edges (device sort) on the kept edges
    keep = x["keep"].to(_dev())
    ei = dd["edge_index"].long()
    g0, order0 = EdgeGraph.from_edges(ei[0][keep], ei[1][keep], N, dd["batch"], B)
    for n in ("src", "dst", "row_ptr", "src_perm", "src_ptr", "batch", "mol_ptr"):
        assert torch.equal(getattr(g, n), getattr(g0, n)), (name, n)
    assert torch.equal(g.order.long(), keep.nonzero().view(-1)[order0])


# ------------------------------------------------------------------------------------------------------------------ 2. padding
def _check_padded(g, g0, pos_real, N, E, n_cap, e_cap, B):
    """the assertions of _check_padded in tests/test_gpu_periodic_capture.py, plus `order`"""
    assert (g.N, g.E, g.num_graphs, g.n_real, g.e_real, g.num_real_graphs) == (n_cap, e_cap, B + 1, N, E, B)
    assert g._padded and g._pbc and g._radius_static and g.capacity == (n_cap, e_cap)
    row_ptr, src, dst = g.row_ptr.cpu().long(), g.src.cpu().long(), g.dst.cpu().long()
    assert row_ptr.shape == (n_cap + 1,) and src.shape == dst.shape == (e_cap,)
    # the head is the un-padded graph, bit for bit
    assert torch.equal(g.row_ptr[:N + 1], g0.row_ptr) and torch.equal(g.src[:E], g0.src) and torch.equal(g.dst[:E], g0.dst)
    assert torch.equal(g.batch[:N], g0.batch) and torch.equal(g.mol_ptr[:B + 1], g0.mol_ptr)
    assert torch.equal(g.offsets[:E], g0.offsets) and torch.equal(g.cell_offsets[:E], g0.cell_offsets)
    assert torch.equal(g.order[:E], g0.order)
    assert g.offsets.shape == (e_cap, 3) and g.cell_offsets.shape == (e_cap, 3) and g.order.shape == (e_cap,)
    assert g.offsets.dtype == torch.float32 and g.cell_offsets.dtype == g.order.dtype == torch.int32
    assert not bool(g.offsets[E:].any()) and not bool(g.cell_offsets[E:].any()) and bool((g.order[E:] == -1).all())
    P, Q = n_cap - N, e_cap - E
    ts, td = src[E:], dst[E:]
    assert int(row_ptr[n_cap]) == e_cap and bool((row_ptr[1:] >= row_ptr[:-1]).all())
    if Q:
        assert int(ts.min()) >= N and int(ts.max()) < n_cap and int(td.min()) >= N and int(td.max()) < n_cap
        assert bool((td[1:] >= td[:-1]).all())
        assert bool((ts != td).all())
        assert torch.unique(ts * n_cap + td).numel() == Q
    deg = torch.bincount(td - N, minlength=P) if P else torch.zeros(0, dtype=torch.long)
    assert torch.equal(row_ptr[N:], E + torch.cat([torch.zeros(1, dtype=torch.long), deg.cumsum(0)]))
    if P:
        assert int(deg.max()) - int(deg.min()) <= 1
    same_row = td[1:] == td[:-1]
    assert bool((ts[1:][same_row] > ts[:-1][same_row]).all())
    assert bool((g.batch[N:] == B).all()) and int(g.mol_ptr[B + 1]) == n_cap
    pos = g.pos.cpu()
    assert torch.equal(pos[:N], pos_real.cpu()) and bool(torch.isfinite(pos).all())
    if Q:
        assert float((pos[ts] - pos[td]).norm(dim=1).min()) > 0.5  # every phantom edge vector is non-zero
    if g.z is not None:
        assert bool((g.z[N:] == 1).all())
    assert torch.equal(g.node_mask.cpu(), (torch.arange(n_cap) < N).float())
    assert torch.equal(g.graph_mask.cpu(), (torch.arange(B + 1) < B).float())
    perm, ptr = _by_source(g.src, n_cap)  # the by-source view over all B + 1 structures
    assert torch.equal(g.src_perm, perm) and torch.equal(g.src_ptr, ptr)


@pytest.mark.parametrize("name", ("shuffled", "empty structure last", "dropped", "no edges"))
def test_padded_graph_is_well_formed(name):
    from equiformer_amd.capture import bucket_of
    from equiformer_amd.graph import GraphDoesNotFit, min_phantom_nodes
    d = _to_dev(gi.cases()[name])
    B = d["cell"].shape[0]
    z = torch.randint(1, 84, (d["pos"].shape[0],), generator=torch.Generator().manual_seed(2)).to(_dev())
    g0, _, _ = _build(d)
    N, E = g0.N, g0.E
    _, nb, eb = bucket_of(B, N, E, NODE_STEP, EDGE_STEP)
    for n_cap, e_cap in ((N, E), (N + 3, E), (N + 2, E + 1), (N + 5, E + 20), (N + 7, E + 5), (N + 9, E + 31), (nb, eb)):
        for zz in (z, None):
            g, offsets, cell_off = _build(d, capacity=(n_cap, e_cap), z=zz)
            assert offsets is g.offsets and cell_off is g.cell_offsets
            _check_padded(g, g0, d["pos"], N, E, n_cap, e_cap, B)
            if zz is not None:
                assert torch.equal(g.z[:N], z)
    # a capacity too small: GraphDoesNotFit, `into` untouched
    g, _, _ = _build(d, capacity=(nb, max(eb, 1024)), z=z)
    before = [getattr(g, n).clone() for n in PADDED_NAMES]
    for bad in ((N + 2, E + 3), (N + 40, E - 1), (N - 1, E), (N + min_phantom_nodes(50) - 1, E + 50)):
        with pytest.raises(GraphDoesNotFit):
            _build(d, capacity=bad, into=g, z=z)
    for a, n in zip(before, PADDED_NAMES):
        assert torch.equal(a, getattr(g, n)), (name, n)


# ------------------------------------------------------------------------------------------------------------------ 3. refill
def test_padded_graph_is_refilled_in_place_with_fewer_and_more_edges():
    a, b = _to_dev(gi.cases()["dropped"]), _to_dev(gi.cases()["shuffled"])
    ea, eb = int(gi.expected("dropped")["src"].numel()), int(gi.expected("shuffled")["src"].numel())
    assert a["cell"].shape[0] == b["cell"].shape[0] == 4 and ea != eb and a["pos"].shape[0] != b["pos"].shape[0]
    cap = (64, 2048)
    gen = torch.Generator().manual_seed(5)
    za = torch.randint(1, 84, (a["pos"].shape[0],), generator=gen).to(_dev())
    zb = torch.randint(1, 84, (b["pos"].shape[0],), generator=gen).to(_dev())
    g, _, _ = _build(a, capacity=cap, z=za)
    tensors = [getattr(g, n) for n in PADDED_NAMES]
    ptrs = [t.data_ptr() for t in tensors]
    for d, z in ((b, zb), (a, za), (b, zb)):  # other real counts each time: fewer edges, more, fewer
        g2, off2, coff2 = _build(d, capacity=cap, into=g, z=z)
        assert g2 is g and off2 is g.offsets and coff2 is g.cell_offsets
        assert all(getattr(g2, n) is t for n, t in zip(PADDED_NAMES, tensors))  # the same objects ...
        assert [getattr(g2, n).data_ptr() for n in PADDED_NAMES] == ptrs         # ... at the same addresses
        fresh, _, _ = _build(d, capacity=cap, z=z)
        for n in PADDED_NAMES:
            assert torch.equal(getattr(g2, n), getattr(fresh, n)), n
        g0, _, _ = _build(d)
        _check_padded(g2, g0, d["pos"], g0.N, g0.E, cap[0], cap[1], 4)
    # a graph of the periodic SEARCH is not refilled by this builder (it has no `order`), nor one of another capacity
    from equiformer_amd.graph import EdgeGraph
    s, _, _ = EdgeGraph.from_radius_pbc(a["pos"], a["cell"], a["batch"], R, 50, num_graphs=4, capacity=cap, z=za)
    assert _build(a, capacity=cap, into=s, z=za)[0] is not s
    assert _build(a, capacity=(96, 2048), into=g, z=za)[0] is not g


def test_exact_shape_into_refills_on_the_same_counts_and_abandons_on_others():
    base = gi.cases()["truncated"]
    a = _to_dev(base)
    b = _to_dev(gi.shuffled(base, seed=3))  # the same counts, another input order
    g, offsets, _ = _build(a)
    first = {n: getattr(g, n).clone() for n in ALL_NAMES}
    tensors = [getattr(g, n) for n in ALL_NAMES]
    g2, off2, _ = _build(b, into=g)
    assert g2 is g and off2 is offsets and all(getattr(g2, n) is t for n, t in zip(ALL_NAMES, tensors))
    fresh, _, _ = _build(b)
    for n in ALL_NAMES:
        assert torch.equal(getattr(g2, n), getattr(fresh, n)), n
    assert not torch.equal(g2.order, first["order"]) and torch.equal(g2.row_ptr, first["row_ptr"])
    g3, _, _ = _build(a, into=g)  # and back
    assert g3 is g and all(torch.equal(getattr(g3, n), first[n]) for n in ALL_NAMES)
    # other kept-edge count (one edge fewer in the input): a fresh graph, `g` abandoned and not refilled any more
    c = dict(a, edge_index=a["edge_index"][:, :-1].contiguous(), cell_offsets=a["cell_offsets"][:-1].contiguous(),
             neighbors=a["neighbors"] - torch.tensor([0, 0, 1], device=_dev()))
    g4, _, _ = _build(c, into=g)
    assert g4 is not g and g4.E == g.E - 1 and not g._radius_static and g4._radius_static
    assert not ({getattr(g4, n).data_ptr() for n in ALL_NAMES} & {t.data_ptr() for t in tensors})
    assert _build(a, into=g)[0] is not g
    # other node count
    g5, _, _ = _build(_to_dev(gi.cases()["in order"]), into=g4)
    assert g5 is not g4 and g5.N != g4.N and not g4._radius_static


# ------------------------------------------------------------------------------------------------------------------ 4. errors
def test_bad_inputs_raise():
    from equiformer_amd.graph import GraphDoesNotFit
    d = _to_dev(gi.cases()["in order"])
    E_in = d["edge_index"].shape[1]
    short = d["neighbors"].clone()
    short[-1] -= 1
    with pytest.raises(ValueError, match="sums to %d.*has %d edges" % (E_in - 1, E_in)):
        _build(dict(d, neighbors=short))
    # an edge whose centre lies in the other structure: both indices stay inside [0, N)
    ei = d["edge_index"].clone()
    first_of_second = int(d["neighbors"][0])
    assert int(d["batch"][ei[1, first_of_second]]) == 1 and int(d["batch"][ei[1, 0]]) == 0
    ei[1, 0] = ei[1, first_of_second]
    assert 0 <= int(ei.min()) and int(ei.max()) < d["pos"].shape[0]
    with pytest.raises(ValueError, match="outside the structure"):
        _build(dict(d, edge_index=ei))
    ei = d["edge_index"].clone()
    ei[0, E_in - 1] = 0  # the neighbour of the last edge (structure 1) in structure 0
    with pytest.raises(ValueError, match="outside the structure"):
        _build(dict(d, edge_index=ei))
    with pytest.raises(ValueError):
        _build(dict(d, cell_offsets=d["cell_offsets"].float()))
    g, _, _ = _build(d, capacity=(64, 2048))
    before = [getattr(g, n).clone() for n in ALL_NAMES]
    with pytest.raises(GraphDoesNotFit):
        _build(d, capacity=(64, g.e_real - 1), into=g)
    assert all(torch.equal(a, getattr(g, n)) for a, n in zip(before, ALL_NAMES))
    g_ok, _, _ = _build(d)  # and the unmodified batch still builds
    assert g_ok.E == g.e_real


# ------------------------------------------------------------------------------------------------------------------ 5. the model
def _model(head=None, otf_graph=False, cap=pi.SLAB_CAP, seed=21):
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20
    cfg = dict(mg.SMALL_OC20, number_of_basis=32, otf_graph=otf_graph, use_pbc=True, max_neighbors=cap, **(head or {}))
    cfg["alpha_drop"] = 0.0
    m = GraphAttentionTransformerOC20(None, None, 1, **cfg)
    return fill_deterministic(m, seed).to(_dev()).train()


def _data(d):
    return SimpleNamespace(**{k: d[k] for k in ("pos", "batch", "atomic_numbers", "tags", "cell", "natoms", "edge_index",
                                                "cell_offsets", "neighbors")})


def _with_atoms(d, seed):
    """atomic numbers, tags and an energy target per structure for a case of given_edges_inputs"""
    gen = torch.Generator().manual_seed(seed)
    N, B = d["pos"].shape[0], d["cell"].shape[0]
    return dict(d, atomic_numbers=torch.randint(1, 84, (N,), generator=gen), tags=torch.randint(0, 3, (N,), generator=gen),
                y=torch.randn(B, generator=gen), num_graphs=B, natoms=torch.tensor(d["natoms"]))


@pytest.mark.parametrize("name", ("shuffled", "dropped"))
def test_model_on_the_new_graph_equals_the_eager_path(name):
    """`model(view, graph=g, offsets=g.offsets)` on the graph of from_edges_pbc, un-padded and padded, against `model(data)` under
    otf_graph=False: energies and every parameter gradient within 1e-4 relative (test_oc20_model_parity_under_padding); phantom
    rows add exact zeros."""
    m = _model()
    params = [p for p in m.parameters() if p.requires_grad]
    d = _to_dev(_with_atoms(gi.cases()[name], 3))
    N, B = d["pos"].shape[0], d["num_graphs"]
    for p in params:
        p.grad = None
    out0 = m(_data(d))
    (out0.squeeze(-1) - d["y"]).abs().mean().backward()
    grads0 = [None if p.grad is None else p.grad.detach().clone() for p in params]
    worst_y = worst_g = 0.0
    for cap in (None, (64, 2048), (64 + 7, 2048 + 33)):
        for p in params:
            p.grad = None
        g, _, _ = _build(d, capacity=cap, z=d["atomic_numbers"] if cap else None)
        if cap is None:
            v = SimpleNamespace(pos=d["pos"], batch=g.batch, atomic_numbers=d["atomic_numbers"], tags=d["tags"])
        else:
            v = SimpleNamespace(pos=g.pos, batch=g.batch, atomic_numbers=g.z, tags=torch.zeros(cap[0], dtype=torch.int64, device=_dev()))
            v.tags[:N] = d["tags"]
        out = m(v, graph=g, offsets=g.offsets)
        assert out.shape[0] == (B if cap is None else B + 1) and bool(torch.isfinite(out).all())
        (out.squeeze(-1)[:B] - d["y"]).abs().mean().backward()
        worst_y = max(worst_y, _rel(out[:B], out0))
        assert _rel(out[:B], out0) < 1e-4, (name, cap, _rel(out[:B], out0))
        n = 0
        for p, a in zip(params, grads0):
            assert (p.grad is None) == (a is None)
            if a is None:
                continue
            assert bool(torch.isfinite(p.grad).all())
            if float(a.abs().max()) > 0:
                worst_g = max(worst_g, _rel(p.grad, a))
                assert _rel(p.grad, a) < 1e-4, (name, cap, _rel(p.grad, a))
                n += 1
            else:
                assert float(p.grad.abs().max()) == 0.0
        assert n > 50
    print("%s: new graph vs model(data), worst rel err energies %.3e, parameter gradients %.3e" % (name, worst_y, worst_g))


# ------------------------------------------------------------------------------------------------------------------ 6. training
def _assert_trains_as_eager(e, b, steps, max_lr):
    """tests/test_gpu_periodic_capture.py _assert_trains_as_eager, restated: losses 2e-5 max(1, |loss|), first moments 5e-4,
    parameters whose moment is above noise 1e-4; the same learning-rate schedule on both sides."""
    assert e["step"] == b["step"] == steps
    worst = max(abs(x - y) / max(1.0, abs(x)) for x, y in zip(e["losses"], b["losses"]))
    big = e["m"].abs() > 1e-3 * e["m"].abs().max()
    print("captured vs eager over %d steps: losses %.3e, moments %.3e, parameters above noise %.3e, all parameters %.3e"
          % (steps, worst, _rel(b["m"], e["m"]), _rel(b["p"][big], e["p"][big]), _rel(b["p"], e["p"])))
    for x, y in zip(e["losses"], b["losses"]):
        assert abs(x - y) <= 2e-5 * max(1.0, abs(x)), (e["losses"], b["losses"])
    assert _rel(b["m"], e["m"]) < 5e-4, _rel(b["m"], e["m"])
    assert int(big.sum()) > 1000
    assert _rel(b["p"][big], e["p"][big]) < 1e-4, _rel(b["p"][big], e["p"][big])
    assert _rel(b["p"], e["p"]) < steps * 2 * max_lr


def test_exact_shape_captured_step_on_a_given_edge_list_trains_as_eager():
    """One edge list (every row truncated), three sets of jittered positions: with a given edge list the shape does not move with
    the positions.  CapturedTrainStep: 3 eager steps, one capture, 5 replays, against 8 eager steps of `model(data)`."""
    from equiformer_amd.capture import CapturedTrainStep
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW
    dev = _dev()
    d = _to_dev(_with_atoms(gi.cases()["truncated"], 4))
    variants = [d["pos"]] + [pi.dense_cells(jitter=0.05, jitter_seed=j)["pos"].to(dev) for j in (1, 2)]
    gen = torch.Generator().manual_seed(4)
    ys = [torch.randn(3, generator=gen).to(dev) for _ in variants]
    results = []
    for use_graph in (False, True):
        m = _model(cap=pi.DENSE_CAP)
        opt = FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)
        pos, y = variants[0].clone(), ys[0].clone()  # the static input tensors
        data = _data(dict(d, pos=pos))

        def forward_loss(g):
            return (m(data, graph=g, offsets=g.offsets).squeeze(-1) - y).abs().mean()

        def build(into):
            return EdgeGraph.from_edges_pbc(pos, d["cell"], d["batch"], d["edge_index"], d["cell_offsets"], d["neighbors"],
                                            num_graphs=3, into=into)[0]
        cs = CapturedTrainStep(opt, forward_loss, min_eager=3)
        losses = []
        for it in range(8):
            pos.copy_(variants[it % 3]), y.copy_(ys[it % 3])
            for gr in opt.param_groups:
                gr["lr"] = 1e-3 * (1.0 + 0.1 * it)  # (sums to 1.08e-2)
            if use_graph:
                loss = cs.step(build)
            else:
                opt.zero_grad(set_to_none=True)
                loss = (m(data).squeeze(-1) - y).abs().mean()
                loss.backward()
                opt.step()
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        if use_graph:
            assert cs.replays == 5 and cs.eager_steps == 3 and len(cs._graphs) == 1, (cs.replays, cs.eager_steps)
        results.append(dict(losses=losses, p=opt.flat_p.detach().clone(), m=opt.flat_m.detach().clone(), step=opt._step))
    assert len({round(v, 6) for v in results[0]["losses"][:3]}) == 3  # (the jitter is seen: three different losses)
    _assert_trains_as_eager(results[0], results[1], 8, 1e-3)


def _padded_loss(m):
    def forward_loss(g, v):
        return (m(v, graph=g, offsets=v.offsets).squeeze(-1)[:v.B] - v.y[:v.B]).abs().mean()
    return forward_loss


def _key(d):
    from equiformer_amd.capture import bucket_of
    from equiformer_amd.graph import EdgeGraph
    plan = EdgeGraph.edges_pbc_plan(d["pos"], d["cell"], d["batch"], d["edge_index"], d["cell_offsets"], d["neighbors"], d["num_graphs"])
    assert plan.E == plan.E_in  # (no zero-length edge among the searched ones)
    return bucket_of(d["num_graphs"], plan.N, plan.E, NODE_STEP, EDGE_STEP)


def _train_bucketed(batches, schedule, bucketed, **kw):
    from equiformer_amd.capture import BucketedTrainStep
    from equiformer_amd.optim import FlatAdamW
    m = _model()
    opt = FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)
    # (radius and max_num_neighbors do not enter the graph: values the edge lists were NOT made with)
    bs = BucketedTrainStep(opt, _padded_loss(m), 1.0, graph_targets=("y",), node_targets=("tags",), max_num_neighbors=1,
                           node_step=NODE_STEP, edge_step=EDGE_STEP, edges="batch", **kw) if bucketed else None
    losses = []
    for it, lr in enumerate(schedule):
        d = batches[it % len(batches)]
        for gr in opt.param_groups:
            gr["lr"] = lr
        if bucketed:
            loss = bs.step(d)
        else:
            opt.zero_grad(set_to_none=True)
            loss = (m(_data(d)).squeeze(-1) - d["y"]).abs().mean()
            loss.backward()
            opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return dict(losses=losses, p=opt.flat_p.detach().clone(), m=opt.flat_m.detach().clone(), step=opt._step, bs=bs)


def test_bucketed_step_on_the_batchs_edges_trains_as_eager_and_most_steps_replay():
    """16 slab batches of 4 structures with the oracle's edge lists (R, SLAB_CAP) attached on the CPU and shuffled inside every
    structure, against the eager loop on `model(data)` under otf_graph=False.  Expected eager / capture / replay counts: host
    arithmetic over bucket_of; by that arithmetic at least half of the steps replay."""
    batches = [_to_dev(d) for d in gi.slab_batches_with_edges(16)]
    min_eager = 1
    keys = [_key(d) for d in batches]
    count = collections.Counter(keys)
    assert len(count) <= 16
    want_captures = sum(1 for c in count.values() if c > min_eager)
    want_replays = sum(max(0, c - min_eager) for c in count.values())
    want_eager = sum(min(c, min_eager) for c in count.values())
    assert want_replays + want_eager == 16 and 2 * want_replays >= 16, count
    schedule = [4.5e-4 * (1.0 + 0.05 * it) for it in range(16)]
    e = _train_bucketed(batches, schedule, False)
    b = _train_bucketed(batches, schedule, True, min_eager=min_eager)
    bs = b["bs"]
    print("buckets %s: %d eager steps, %d captures, %d replays" % (dict(count), bs.eager_steps, bs.captures, bs.replays))
    assert (bs.eager_steps, bs.captures, bs.replays, bs.evictions) == (want_eager, want_captures, want_replays, 0)
    assert bs.real_nodes == sum(d["pos"].shape[0] for d in batches) and bs.padded_nodes == sum(k[1] for k in keys)
    assert bs.real_edges == sum(d["edge_index"].shape[1] for d in batches)
    _assert_trains_as_eager(e, b, 16, 4.5e-4)
    # a batch without its edge list, and a non-periodic one, are refused by name
    with pytest.raises(ValueError, match="cell_offsets, neighbors missing"):
        bs.step({k: v for k, v in batches[0].items() if k not in ("cell_offsets", "neighbors")})
    with pytest.raises(ValueError, match="cell missing"):
        bs.step({k: v for k, v in batches[0].items() if k != "cell"})


# ------------------------------------------------------------------------------------------------------------------ IS2RS, evaluation
def test_is2rs_step_on_the_batchs_edges_equals_the_searching_step():
    """IS2RSTrainStep(edges="batch") against the same class with edges="search" over 6 slab batches.  Step k perturbs batch k with
    step_seed(seed, k) BEFORE the graph, so the edge list attached to batch k is the search's on those perturbed positions
    (synthetic.attach_given_edges): both steps see one graph."""
    from equiformer_amd import ops
    from equiformer_amd.is2rs import IS2RSLoss, IS2RSTrainStep, step_seed
    from equiformer_amd.optim import FlatAdamW
    from equiformer_amd.synthetic import attach_given_edges
    seed, steps = 99, 6
    gen = torch.Generator().manual_seed(17)
    batches = []
    for k, d in enumerate(pi.slab_batches(steps)):
        free = (d["tags"] > 0).view(-1, 1)
        d["pos_relaxed"] = torch.where(free, d["pos"] + 0.2 * torch.randn(d["pos"].shape, generator=gen), d["pos"])
        d = _to_dev(d)
        moved = ops.is2rs_perturb(d["pos"], d["pos_relaxed"], d["tags"], d["batch"].to(torch.int32), seed=step_seed(seed, k))[0]
        e = attach_given_edges(dict(d, pos=moved), R, pi.SLAB_CAP)
        assert e["edge_index"].dtype == e["cell_offsets"].dtype == e["neighbors"].dtype == torch.int64
        assert int(e["neighbors"].sum()) == e["edge_index"].shape[1] > 0 and e["neighbors"].shape == (4,)
        batches.append(dict(d, edge_index=e["edge_index"], cell_offsets=e["cell_offsets"], neighbors=e["neighbors"]))
    norm = dict(target_mean=0.3, target_std=1.7, positions_mean=(0.01, -0.02, 0.03), positions_std=(0.4, 0.5, 0.6))
    runs = {}
    for edges in ("search", "batch"):
        m = _model(head=dict(use_auxiliary_task=True), otf_graph=(edges == "search"))
        opt = FlatAdamW(m.parameters(), lr=5e-4, weight_decay=1e-2)
        L = IS2RSLoss(auxiliary_task_weight=15.0, **norm)
        ts = IS2RSTrainStep(m, opt, L, R, pi.SLAB_CAP, interpolate=True, seed=seed, total_steps=steps, min_eager=1,
                            node_step=NODE_STEP, edge_step=8192, edges=edges)
        losses, stats = [], []
        for d in batches:
            losses.append(float(ts.step(d)))
            stats.append(L.stats.cpu().clone())
        torch.cuda.synchronize()
        runs[edges] = dict(losses=losses, stats=stats, counts=(ts.eager_steps, ts.captures, ts.replays))
    print("IS2RS search %s / batch %s; losses %s" % (runs["search"]["counts"], runs["batch"]["counts"], runs["batch"]["losses"]))
    assert runs["search"]["counts"] == runs["batch"]["counts"] and runs["batch"]["counts"][2] >= 1
    for a, b in zip(runs["search"]["losses"], runs["batch"]["losses"]):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(a)), (runs["search"]["losses"], runs["batch"]["losses"])
    for sa, sb in zip(runs["search"]["stats"], runs["batch"]["stats"]):
        for x, y in zip(sa[:7].tolist(), sb[:7].tolist()):
            assert abs(x - y) <= 2e-5 * max(1.0, abs(x)), (sa, sb)


def test_evaluate_oc20_on_the_batchs_edges_reports_the_eager_figures():
    """evaluate_oc20(..., edges="batch") against the reference-style totals on the eager predictions of `model(data)` under
    otf_graph=False: the tolerances of tests/test_gpu_eval_step.py (rows 1e-4 relative, totals 1e-4, the count exact)."""
    from equiformer_amd.evaluate import evaluate_oc20, oc20_eval_step
    mean, std, thr = 0.3, 1.7, 1.0
    m = _model().eval()
    batches = [_to_dev(d) for d in gi.slab_batches_with_edges(4)]
    with torch.no_grad():
        eager = [m(_data(d)).squeeze(-1).clone() for d in batches]
    tot, numel = {"energy_mae": 0.0, "energy_mse": 0.0, "energy_within_threshold": 0.0}, 0
    for p, d in zip(eager, batches):
        e = p.double().cpu() * std + mean - d["y"].double().cpu()
        tot["energy_mae"] += e.abs().sum().item()
        tot["energy_mse"] += (e ** 2).sum().item()
        tot["energy_within_threshold"] += (e.abs() < thr).sum().item()
        numel += e.numel()
        assert float((e.abs() - thr).abs().min()) > 1e-3  # (no error so near the threshold that 1e-4 could move the count)
    es = oc20_eval_step(m, 1.0, task_mean=mean, task_std=std, threshold=thr, min_eager=1, max_num_neighbors=1, node_step=16,
                        edge_step=128, edges="batch")
    for sweep in range(2):
        for d, e0 in zip(batches, eager):
            e, f = es.step(d)
            assert f is None and _rel(e.squeeze(-1), e0) < 1e-4, (sweep, _rel(e.squeeze(-1), e0))
    assert es.replays >= 4
    metrics = evaluate_oc20(m, batches, 1.0, step=es)
    fresh = evaluate_oc20(m, batches, 1.0, task_mean=mean, task_std=std, threshold=thr, min_eager=1, node_step=16, edge_step=128,
                          edges="batch")
    for got in (metrics, fresh):
        for k in tot:
            assert got[k]["numel"] == numel == 16
            assert abs(got[k]["total"] - tot[k]) <= 1e-4 * abs(tot[k]), (k, got[k], tot[k])
            assert abs(got[k]["metric"] - tot[k] / numel) <= 1e-4 * abs(tot[k] / numel)
        assert got["energy_within_threshold"]["total"] == tot["energy_within_threshold"]
