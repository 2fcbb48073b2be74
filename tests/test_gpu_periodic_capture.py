"""The periodic (OC20) train step as a HIP graph, exact-shape and bucketed, on the GPU:

1. eqf_csr_by_source_multi (csrc/graph.hip) gives the stable argsort of the sources and the scan of their counts for rows that
   hold a source once per periodic image (integers: torch.equal), while the periodic search still equals oracle/pbc.py;
2. EdgeGraph.from_radius_pbc(into=) refills a graph in place;  3. from_radius_pbc(capacity=) pads it with one phantom structure;
4. the OC20 model on the padded graph gives the real rows of the unpadded call (every head variant);
5. CapturedTrainStep / BucketedTrainStep train as the eager, unpadded loop;  6. and most of their steps really are replays.
Inputs: tests/periodic_inputs.py (tests/test_periodic_capture.py shows on the CPU that they repeat pairs and truncate rows).
Tolerances of the trajectory comparisons are those of tests/test_gpu_capture.py and tests/test_gpu_bucketed_capture.py."""
import collections
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import periodic_inputs as pi  # noqa: E402

R = pi.R
NODE_STEP, EDGE_STEP = 64, 1024  # the 16 slab batches (N = 95-131, E = 1 470-3 040) fall into three buckets: most steps replay
INDEX_NAMES = ("row_ptr", "src", "dst", "src_perm", "src_ptr", "batch", "mol_ptr", "offsets", "cell_offsets")
HEADS = {"energy": {}, "aux": dict(use_auxiliary_task=True), "attn": dict(use_attention_head=True),
         "attn_aux": dict(use_attention_head=True, use_auxiliary_task=True)}


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _to_dev(d):
    dev = _dev()
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in d.items()}


def _build(d, cap, **kw):
    """d: tensors on the GPU"""
    from equiformer_amd.graph import EdgeGraph
    return EdgeGraph.from_radius_pbc(d["pos"], d["cell"], d["batch"], R, max_num_neighbors=cap, num_graphs=len(d["natoms"]), **kw)


def _by_source(src, N):
    """what the kernel replaces: stable argsort of src, exclusive scan of its counts"""
    perm = torch.argsort(src.long(), stable=True).to(torch.int32)
    ptr = torch.cat([torch.zeros(1, dtype=torch.long, device=src.device), torch.bincount(src.long(), minlength=N).cumsum(0)])
    return perm, ptr.to(torch.int32)


def _cases():
    slab = pi.slab_batches(2)[1]
    return [("triclinic", pi.small_triclinic(), 500), ("triclinic, other seed", pi.small_triclinic(seed=11), 500),
            ("triclinic, capped", pi.small_triclinic(), 12), ("cubic", pi.small_cubic(), 50),
            ("with an empty structure", pi.with_an_empty_structure(), 50), ("dense, capped", pi.dense_cells(), pi.DENSE_CAP),
            ("slab batch", dict(slab, natoms=slab["natoms"].tolist()), pi.SLAB_CAP)]


# ------------------------------------------------------------------------------------------------------------------ 1. kernel contract
def test_by_source_view_of_periodic_graphs_is_the_stable_argsort_and_the_search_equals_the_oracle():
    from oracle import pbc
    for name, d, cap in _cases():
        ei, off, nb = pbc.radius_graph_pbc(d["pos"], d["cell"], [int(n) for n in d["natoms"]], R, cap)
        N = d["pos"].shape[0]
        g, offsets, cell_off = _build(_to_dev(d), cap)
        assert g.N == N and g.E == ei.shape[1] and g.num_graphs == len(d["natoms"]), name
        got = torch.cat([g.src.cpu().long()[:, None], g.dst.cpu().long()[:, None], cell_off.cpu().long()], dim=1)
        want = torch.cat([ei[0][:, None], ei[1][:, None], off], dim=1)
        assert torch.equal(got, want), name  # same order as well: by centre, neighbour, image
        cart = torch.bmm(off.float().view(-1, 1, 3), torch.repeat_interleave(d["cell"], nb, dim=0)).view(-1, 3)
        assert float((offsets.cpu() - cart).abs().max()) < 1e-5 if g.E else True
        rp = g.row_ptr.cpu().long()
        assert torch.equal(rp[1:] - rp[:-1], torch.bincount(ei[1], minlength=N)), name
        perm, ptr = _by_source(g.src, N)
        assert g.src_perm.dtype == g.src_ptr.dtype == torch.int32
        assert torch.equal(g.src_perm, perm), name
        assert torch.equal(g.src_ptr, ptr), name
        assert torch.equal(g.src_perm.cpu().long(), torch.argsort(ei[0], stable=True)), name
        assert g.offsets is offsets and g.cell_offsets is cell_off
        rep, mult = pi.repeated_pairs(g.src.cpu(), g.dst.cpu(), N)
        print("%s: N %d, E %d, %d repeated pairs (multiplicity up to %d)" % (name, N, g.E, rep, mult))
        assert rep >= 1


def test_entry_point_on_rows_whose_equal_sources_are_not_adjacent():
    from equiformer_amd.graph import _P, _stream
    from equiformer_amd.lib import call
    dev = _dev()
    gen = torch.Generator().manual_seed(0)
    for name, d, cap in _cases()[:4]:
        g, _, _ = _build(_to_dev(d), cap)
        src, rp = g.src.cpu().clone(), g.row_ptr.cpu().tolist()
        apart = 0
        for a, b in zip(rp[:-1], rp[1:]):  # permute the edges inside every row
            src[a:b] = src[a:b][torch.randperm(b - a, generator=gen)]
            row = src[a:b].tolist()
            apart += sum(1 for i, s in enumerate(row) if s in row[:i] and row[i - 1] != s)
        assert apart > 0, name  # equal sources with another source in between
        src = src.to(dev)
        perm = torch.full((g.E,), -1, dtype=torch.int32, device=dev)
        ptr = torch.full((g.N + 1,), -1, dtype=torch.int32, device=dev)
        largest = int((g.mol_ptr[1:] - g.mol_ptr[:-1]).max())
        call("eqf_csr_by_source_multi", _P(src), _P(g.row_ptr), _P(g.mol_ptr), g.num_graphs, largest, _P(perm), _P(ptr), _stream())
        want_perm, want_ptr = _by_source(src, g.N)
        assert torch.equal(perm, want_perm), name
        assert torch.equal(ptr, want_ptr), name
        # a larger bound of the nodes per structure is allowed; a radius graph without repeats gives what eqf_csr_by_source gives
        perm.fill_(-1), ptr.fill_(-1)
        call("eqf_csr_by_source_multi", _P(src), _P(g.row_ptr), _P(g.mol_ptr), g.num_graphs, 4096, _P(perm), _P(ptr), _stream())
        assert torch.equal(perm, want_perm) and torch.equal(ptr, want_ptr), name
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.synthetic import qm9_like_batch
    q = _to_dev(qm9_like_batch(6, 12, side=5.5, seed=9))
    g = EdgeGraph.from_radius(q["pos"], q["batch"], R, num_graphs=6)
    perm, ptr = torch.empty_like(g.src_perm), torch.empty_like(g.src_ptr)
    call("eqf_csr_by_source_multi", _P(g.src), _P(g.row_ptr), _P(g.mol_ptr), 6, 12, _P(perm), _P(ptr), _stream())
    assert torch.equal(perm, g.src_perm) and torch.equal(ptr, g.src_ptr)


# ------------------------------------------------------------------------------------------------------------------ 2. in-place refill
def test_from_radius_pbc_into_refills_in_place_and_abandons_on_other_counts():
    a = _to_dev(pi.dense_cells())
    b = _to_dev(pi.dense_cells(jitter=0.05, jitter_seed=1))
    g, offsets, cell_off = _build(a, pi.DENSE_CAP)
    assert g._radius_static
    ptrs = [getattr(g, n).data_ptr() for n in INDEX_NAMES]
    first = {n: getattr(g, n).clone() for n in INDEX_NAMES}
    g2, off2, coff2 = _build(b, pi.DENSE_CAP, into=g)
    assert g2 is g and off2 is g.offsets and coff2 is g.cell_offsets and off2.data_ptr() == offsets.data_ptr()
    assert [getattr(g2, n).data_ptr() for n in INDEX_NAMES] == ptrs
    fresh, _, _ = _build(b, pi.DENSE_CAP)
    assert (fresh.N, fresh.E) == (g.N, g.E)
    for n in INDEX_NAMES:
        assert torch.equal(getattr(g2, n), getattr(fresh, n)), n
    assert not torch.equal(g2.src, first["src"]) or not torch.equal(g2.offsets, first["offsets"])  # (another edge list)
    g3, _, _ = _build(a, pi.DENSE_CAP, into=g)  # and back
    assert g3 is g and all(torch.equal(getattr(g3, n), first[n]) for n in INDEX_NAMES)
    # other edge count (the same atoms, uncapped): a fresh graph, `g` abandoned
    g4, _, _ = _build(a, 500, into=g)
    assert g4 is not g and g4.E != g.E and not g._radius_static and g4._radius_static
    assert not ({getattr(g4, n).data_ptr() for n in INDEX_NAMES} & set(ptrs))
    perm, ptr = _by_source(g4.src, g4.N)
    assert torch.equal(g4.src_perm, perm) and torch.equal(g4.src_ptr, ptr)
    # an abandoned graph is not refilled any more
    g5, _, _ = _build(a, pi.DENSE_CAP, into=g)
    assert g5 is not g
    # other node count
    c = _to_dev(pi.small_cubic())
    g6, _, _ = _build(c, pi.DENSE_CAP, into=g5)
    assert g6 is not g5 and g6.N != g5.N and not g5._radius_static


# ------------------------------------------------------------------------------------------------------------------ 3. padded graph
def _check_padded(g, g0, pos_real, N, E, n_cap, e_cap, B):
    """the bullets of _check_padded in tests/test_gpu_bucketed_capture.py, for a graph whose REAL rows may repeat pairs, plus
    the per-edge offsets"""
    assert (g.N, g.E, g.num_graphs, g.n_real, g.e_real, g.num_real_graphs) == (n_cap, e_cap, B + 1, N, E, B)
    row_ptr, src, dst = g.row_ptr.cpu().long(), g.src.cpu().long(), g.dst.cpu().long()
    assert row_ptr.shape == (n_cap + 1,) and src.shape == dst.shape == (e_cap,)
    # the real part is the unpadded graph, bit for bit
    assert torch.equal(g.row_ptr[:N + 1], g0.row_ptr) and torch.equal(g.src[:E], g0.src) and torch.equal(g.dst[:E], g0.dst)
    assert torch.equal(g.batch[:N], g0.batch) and torch.equal(g.mol_ptr[:B + 1], g0.mol_ptr)
    assert torch.equal(g.offsets[:E], g0.offsets) and torch.equal(g.cell_offsets[:E], g0.cell_offsets)
    assert g.offsets.shape == (e_cap, 3) and g.cell_offsets.shape == (e_cap, 3)
    assert g.offsets.dtype == torch.float32 and g.cell_offsets.dtype == torch.int32
    assert not bool(g.offsets[E:].any()) and not bool(g.cell_offsets[E:].any())  # phantom edges: zero offsets
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
    same_row = td[1:] == td[:-1]
    assert bool((ts[1:][same_row] > ts[:-1][same_row]).all())  # sources ascend inside a phantom row
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
    # by-source view over all B + 1 structures
    perm, ptr = _by_source(g.src, n_cap)
    assert torch.equal(g.src_perm, perm) and torch.equal(g.src_ptr, ptr)


def test_padded_periodic_graph_is_well_formed():
    from equiformer_amd.capture import bucket_of
    from equiformer_amd.graph import GraphDoesNotFit, min_phantom_nodes
    gen = torch.Generator().manual_seed(2)
    for name, d, cap in (_cases()[0], _cases()[2], _cases()[4], _cases()[6]):
        B = len(d["natoms"])
        d = _to_dev(d)
        z = torch.randint(1, 84, (d["pos"].shape[0],), generator=gen).to(_dev())
        g0, _, _ = _build(d, cap)
        N, E = g0.N, g0.E
        _, nb, eb = bucket_of(B, N, E, NODE_STEP, EDGE_STEP)
        caps = [(N, E), (N + 3, E),            # Q = 0, without and with phantom nodes
                (N + 2, E + 1),                # Q = 1
                (N + 5, E + 20),               # the largest Q five phantom nodes allow: every ordered pair
                (N + 7, E + 5),                # fewer edges than phantom nodes: rows without edges
                (N + 9, E + 31),               # degrees that differ by one
                (nb, eb)]                      # the batch's own bucket
        for n_cap, e_cap in caps:
            for zz in (z, None):
                g, offsets, cell_off = _build(d, cap, capacity=(n_cap, e_cap), z=zz)
                assert offsets is g.offsets and cell_off is g.cell_offsets
                _check_padded(g, g0, d["pos"], N, E, n_cap, e_cap, B)
                if zz is not None:
                    assert torch.equal(g.z[:N], z)
        # does not fit: `into` stays as it was
        names = INDEX_NAMES + ("pos", "z", "node_mask", "graph_mask")
        g, _, _ = _build(d, cap, capacity=(nb, eb), z=z)
        before = [getattr(g, n).clone() for n in names]
        for bad in ((N + 2, E + 3), (N + 40, E - 1), (N - 1, E), (N + min_phantom_nodes(50) - 1, E + 50)):
            with pytest.raises(GraphDoesNotFit):
                _build(d, cap, capacity=bad, into=g, z=z)
        for a, n in zip(before, names):
            assert torch.equal(a, getattr(g, n)), (name, n)
        # capacity=None is the unpadded path
        g1, _, _ = _build(d, cap, capacity=None)
        assert torch.equal(g1.src, g0.src) and torch.equal(g1.src_perm, g0.src_perm) and not hasattr(g1, "node_mask")


def _slab(n=16):
    return [_to_dev(d) for d in pi.slab_batches(n)]


def _key(d):
    from equiformer_amd.capture import bucket_of
    from equiformer_amd.graph import EdgeGraph
    plan = EdgeGraph.radius_pbc_plan(d["pos"], d["cell"], d["batch"], R, pi.SLAB_CAP, d["num_graphs"])
    return bucket_of(d["num_graphs"], plan.N, plan.E, NODE_STEP, EDGE_STEP)


def test_padded_periodic_graph_is_refilled_in_place_for_another_real_shape():
    batches = _slab()
    keys = [_key(d) for d in batches]
    key = max(set(keys), key=keys.count)
    a, b = [d for d, k in zip(batches, keys) if k == key][:2]
    a, b = dict(a, natoms=a["natoms"].tolist()), dict(b, natoms=b["natoms"].tolist())
    ga0, gb0 = _build(a, pi.SLAB_CAP)[0], _build(b, pi.SLAB_CAP)[0]
    assert (ga0.N, ga0.E) != (gb0.N, gb0.E)
    names = INDEX_NAMES + ("pos", "z", "node_mask", "graph_mask")
    g, _, _ = _build(a, pi.SLAB_CAP, capacity=key[1:], z=a["atomic_numbers"])
    ptrs = [getattr(g, n).data_ptr() for n in names]
    g2, _, _ = _build(b, pi.SLAB_CAP, capacity=key[1:], into=g, z=b["atomic_numbers"])
    assert g2 is g and [getattr(g2, n).data_ptr() for n in names] == ptrs
    fresh, _, _ = _build(b, pi.SLAB_CAP, capacity=key[1:], z=b["atomic_numbers"])
    for n in names:
        assert torch.equal(getattr(g2, n), getattr(fresh, n)), n
    _check_padded(g2, gb0, b["pos"], gb0.N, gb0.E, key[1], key[2], 4)
    g3, _, _ = _build(a, pi.SLAB_CAP, capacity=key[1:], into=g, z=a["atomic_numbers"])
    assert g3 is g
    _check_padded(g3, ga0, a["pos"], ga0.N, ga0.E, key[1], key[2], 4)


# ------------------------------------------------------------------------------------------------------------------ 4. model parity
def _model(head="energy", alpha_drop=0.0, cap=pi.SLAB_CAP, seed=21):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20
    cfg = dict(mg.SMALL_OC20, number_of_basis=32, otf_graph=True, use_pbc=True, max_neighbors=cap, **HEADS[head])
    cfg["alpha_drop"] = alpha_drop
    m = GraphAttentionTransformerOC20(None, None, 1, **cfg)
    return fill_deterministic(m, seed).to(_dev()).train()


def _data(d):
    return SimpleNamespace(pos=d["pos"], batch=d["batch"], atomic_numbers=d["atomic_numbers"], tags=d["tags"], cell=d["cell"],
                           natoms=d["natoms"])


def _unpadded_loss(m, d, aux_target=None):
    """the eager step's loss: the model builds its own periodic graph (otf_graph=True)"""
    out = m(_data(d))
    if isinstance(out, tuple):
        return (out[0].squeeze(-1) - d["y"]).abs().mean() + 0.5 * (out[1] - aux_target).abs().mean(), out
    return (out.squeeze(-1) - d["y"]).abs().mean(), out


def _padded_loss(m, aux=False):
    """what a captured step runs: no neighbour search inside, phantom rows kept out of the loss through [:B] and node_mask"""
    def forward_loss(g, v, return_out=False):
        out = m(v, graph=g, offsets=v.offsets)
        if isinstance(out, tuple):
            loss = ((out[0].squeeze(-1)[:v.B] - v.y[:v.B]).abs().mean()
                    + 0.5 * ((out[1] - v.aux).abs() * v.node_mask[:, None]).sum() / (3.0 * v.node_mask.sum()))
        else:
            loss = (out.squeeze(-1)[:v.B] - v.y[:v.B]).abs().mean()
        return (loss, out) if return_out else loss
    return forward_loss


@pytest.mark.parametrize("head", sorted(HEADS))
def test_oc20_model_parity_under_padding(head):
    """Energies of the real structures (and the auxiliary vectors of the real atoms) and every parameter gradient of the padded
    call `model(view, graph=g, offsets=g.offsets)` against the unpadded `model(data)`: 1e-4 relative, the bound of
    test_model_parity_under_padding."""
    from equiformer_amd.graph import EdgeGraph
    m = _model(head)
    params = [p for p in m.parameters() if p.requires_grad]
    fl = _padded_loss(m)
    gen = torch.Generator().manual_seed(3)
    worst_y = worst_g = 0.0
    for d in _slab(2):
        key, B, N = _key(d), d["num_graphs"], d["pos"].shape[0]
        aux_t = torch.randn(N, 3, generator=gen).to(_dev())
        for p in params:
            p.grad = None
        loss0, out0 = _unpadded_loss(m, d, aux_t)
        loss0.backward()
        grads0 = [None if p.grad is None else p.grad.detach().clone() for p in params]
        for cap in (key[1:], (key[1] + 7, key[2] + 33)):
            for p in params:
                p.grad = None
            g, _, _ = EdgeGraph.from_radius_pbc(d["pos"], d["cell"], d["batch"], R, pi.SLAB_CAP, num_graphs=B, capacity=cap,
                                                z=d["atomic_numbers"])
            v = SimpleNamespace(pos=g.pos, batch=g.batch, atomic_numbers=g.z, offsets=g.offsets, node_mask=g.node_mask, B=B,
                                tags=torch.zeros(cap[0], dtype=torch.int64, device=_dev()),
                                y=torch.cat([d["y"], d["y"].new_zeros(1)]), aux=torch.zeros(cap[0], 3, device=_dev()))
            v.tags[:N] = d["tags"]
            v.aux[:N] = aux_t
            loss, out = fl(g, v, return_out=True)
            loss.backward()
            pairs = [(out, out0)] if not isinstance(out, tuple) else [(out[0], out0[0]), (out[1], out0[1])]
            assert pairs[0][0].shape[0] == B + 1 and all(bool(torch.isfinite(a).all()) for a, _ in pairs)
            for (a, b), rows in zip(pairs, (B, N)):
                assert a.shape[0] == (B + 1, cap[0])[rows == N]
                worst_y = max(worst_y, _rel(a[:rows], b))
                assert _rel(a[:rows], b) < 1e-4, (head, _rel(a[:rows], b))
            n = 0
            for p, a in zip(params, grads0):
                assert (p.grad is None) == (a is None)
                if a is None:
                    continue
                assert bool(torch.isfinite(p.grad).all())
                if float(a.abs().max()) > 0:
                    worst_g = max(worst_g, _rel(p.grad, a))
                    assert _rel(p.grad, a) < 1e-4, (head, _rel(p.grad, a))
                    n += 1
                else:
                    assert float(p.grad.abs().max()) == 0.0
            assert n > 50
    print("oc20 %s: padded vs unpadded, worst rel err outputs %.3e, parameter gradients %.3e" % (head, worst_y, worst_g))


# ------------------------------------------------------------------------------------------------------------------ 5. / 6. training
def _assert_trains_as_eager(e, b, steps, max_lr):
    """tests/test_gpu_capture.py:154-162 and tests/test_gpu_bucketed_capture.py:248-251: losses 2e-5 max(1, |loss|), first moments
    5e-4, parameters whose moment is above noise 1e-4; the learning rates of a trajectory sum to at most 1.08e-2 as there."""
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


def test_exact_shape_captured_periodic_step_trains_as_eager():
    """CapturedTrainStep over three sets of jittered positions that keep (N, E) (every row truncated, another edge list each):
    3 eager steps, the capture, 4 replays against 8 eager steps in which the model builds its own graph."""
    from equiformer_amd.capture import CapturedTrainStep
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW
    dev = _dev()
    base = pi.dense_cells()
    variants = [base["pos"].to(dev)] + [pi.dense_cells(jitter=0.05, jitter_seed=j)["pos"].to(dev) for j in (1, 2)]
    cell, batch = base["cell"].to(dev), base["batch"].to(dev)
    gen = torch.Generator().manual_seed(4)
    z = torch.randint(1, 84, (36,), generator=gen).to(dev)
    tags = torch.randint(0, 3, (36,), generator=gen).to(dev)
    ys = [torch.randn(3, generator=gen).to(dev) for _ in variants]
    results = []
    for use_graph in (False, True):
        m = _model(cap=pi.DENSE_CAP)
        opt = FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)
        pos, y = variants[0].clone(), ys[0].clone()  # the static input tensors
        data = SimpleNamespace(pos=pos, batch=batch, atomic_numbers=z, tags=tags, cell=cell, natoms=torch.tensor([12, 12, 12]))

        def forward_loss(g):
            return (m(data, graph=g, offsets=g.offsets).squeeze(-1) - y).abs().mean()

        def build(into):
            return EdgeGraph.from_radius_pbc(pos, cell, batch, R, pi.DENSE_CAP, num_graphs=3, into=into)[0]
        cs = CapturedTrainStep(opt, forward_loss, min_eager=3)
        losses, lists = [], []
        for it in range(8):
            pos.copy_(variants[it % 3]), y.copy_(ys[it % 3])
            for gr in opt.param_groups:
                gr["lr"] = 1e-3 * (1.0 + 0.1 * it)  # (sums to 1.08e-2)
            if use_graph:
                loss = cs.step(build)
                sg = next(iter(cs._graphs.values()))["sg"] if cs._graphs else None
                if sg is not None:
                    lists.append(sg.src.clone())
            else:
                opt.zero_grad(set_to_none=True)
                loss = (m(data).squeeze(-1) - y).abs().mean()
                loss.backward()
                opt.step()
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        if use_graph:
            assert cs.replays == 5 and cs.eager_steps == 3, (cs.replays, cs.eager_steps)
            assert len(cs._graphs) == 1 and any(not torch.equal(a, lists[0]) for a in lists[1:])  # one graph, refilled edge lists
        results.append(dict(losses=losses, p=opt.flat_p.detach().clone(), m=opt.flat_m.detach().clone(), step=opt._step))
    _assert_trains_as_eager(results[0], results[1], 8, 1e-3)


def _train_bucketed(batches, schedule, bucketed, alpha_drop=0.0, **kw):
    from equiformer_amd.capture import BucketedTrainStep
    from equiformer_amd.optim import FlatAdamW
    m = _model(alpha_drop=alpha_drop)
    opt = FlatAdamW(m.parameters(), lr=1e-3, weight_decay=1e-2)
    bs = BucketedTrainStep(opt, _padded_loss(m), R, graph_targets=("y",), node_targets=("tags",), max_num_neighbors=pi.SLAB_CAP,
                           node_step=NODE_STEP, edge_step=EDGE_STEP, **kw) if bucketed else None
    losses = []
    for it, lr in enumerate(schedule):
        d = batches[it % len(batches)]
        for gr in opt.param_groups:
            gr["lr"] = lr
        if bucketed:
            loss = bs.step(d)
        else:
            opt.zero_grad(set_to_none=True)
            loss, _ = _unpadded_loss(m, d)
            loss.backward()
            opt.step()
        losses.append(float(loss.detach()))
    torch.cuda.synchronize()
    return dict(losses=losses, p=opt.flat_p.detach().clone(), m=opt.flat_m.detach().clone(), step=opt._step, bs=bs)


def test_bucketed_periodic_batches_train_as_eager_and_most_steps_replay():
    """16 slab batches of 4 structures, every one with its own (N, E) and `cell` in the batch.  The expected numbers of eager
    steps, captures and replays are host arithmetic over bucket_of; by that arithmetic alone at least half of the steps replay."""
    batches = _slab(16)
    min_eager = 1
    keys = [_key(d) for d in batches]
    assert len({(d["pos"].shape[0], k) for d, k in zip(batches, keys)}) > 8
    count = collections.Counter(keys)
    assert len(count) <= 16  # (every bucket within max_graphs: nothing is evicted)
    want_captures = sum(1 for c in count.values() if c > min_eager)
    want_replays = sum(max(0, c - min_eager) for c in count.values())
    want_eager = sum(min(c, min_eager) for c in count.values())
    assert want_replays + want_eager == 16 and 2 * want_replays >= 16, count
    schedule = [4.5e-4 * (1.0 + 0.05 * it) for it in range(16)]  # (sums to 9.9e-3; every step's rate <= 2 x the base rate)
    e = _train_bucketed(batches, schedule, False)
    b = _train_bucketed(batches, schedule, True, min_eager=min_eager)
    bs = b["bs"]
    print("buckets %s: %d eager steps, %d captures, %d replays" % (dict(count), bs.eager_steps, bs.captures, bs.replays))
    assert (bs.eager_steps, bs.captures, bs.replays, bs.evictions) == (want_eager, want_captures, want_replays, 0)
    assert bs.captures_of == {k: 1 for k, c in count.items() if c > min_eager}
    assert sorted(bs.live_graphs()) == sorted(k for k, c in count.items() if c > min_eager)
    assert bs.real_nodes == sum(d["pos"].shape[0] for d in batches) and bs.padded_nodes == sum(k[1] for k in keys)
    _assert_trains_as_eager(e, b, 16, 4.5e-4)


def test_bucketed_periodic_step_draws_a_fresh_dropout_mask_per_replay():
    """alpha_drop > 0, learning rate 0 (the weights do not move): replays on the same batch differ by their masks only"""
    from equiformer_amd.capture import BucketedTrainStep
    from equiformer_amd.optim import FlatAdamW
    d = _slab(1)[0]
    m = _model(alpha_drop=0.3)
    opt = FlatAdamW(m.parameters(), lr=0.0, weight_decay=0.0)
    bs = BucketedTrainStep(opt, _padded_loss(m), R, graph_targets=("y",), node_targets=("tags",), max_num_neighbors=pi.SLAB_CAP,
                           node_step=NODE_STEP, edge_step=EDGE_STEP, min_eager=2)
    losses = [float(bs.step(d)) for _ in range(8)]
    assert bs.replays == 6 and bs.captures == 1 and bs.eager_steps == 2
    assert len({round(v, 7) for v in losses[2:]}) >= 5, losses
    # one instance serves periodic or non-periodic batches, not both
    with pytest.raises(ValueError):
        bs.step({k: v for k, v in d.items() if k != "cell"})
