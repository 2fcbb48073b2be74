"""Per-graph stochastic depth drawn on the device (equiformer_amd/droppath.py, csrc/edge.hip eqf_segment_droppath) on the GPU:

1. the operator is bit-equal to eqf_segment_scale fed `keep_factors` -- forward, gradient, create_graph second derivative -- at
   ragged shapes, and the seed may be split between the by-value argument and the device word;
2. the OC20 model in training mode under `device_draws` against the fp64 oracle whose stochastic depth applies `keep_factors`;
3. the padded view of a batch drops the real graphs the unpadded batch drops;
4. the captured IS2RS step trains as the eager loop under `device_draws(step_seed(s, k))`, with another mask per replay;
5. the same for a non-periodic BucketedTrainStep.
Bounds: those of test_drop_path_training_matches_oracle (outputs 1e-4, probed gradient 2e-4) and of
tests/test_gpu_is2rs_step.py / tests/test_gpu_bucketed_capture.py (losses 2e-5 max(1, |loss|), moments 5e-4, parameters above
noise 1e-4), unchanged.
Wall time of this file on an MI355X, one run each (pytest's figure): 4.8 s at the parent commit, 4.8 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py)."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import periodic_inputs as pi  # noqa: E402
from poison import poisoned_ops  # noqa: E402,F401  (the fixture of the tests that run on poisoned, guarded allocations)
import test_gpu_bucketed_capture as tb  # noqa: E402  (the QM9 batches, losses and trajectory bounds)
import test_gpu_is2rs_step as t6  # noqa: E402  (the slab batch, the loss normalisation and the trajectory bounds)
import test_gpu_oc20_heads as th  # noqa: E402  (the explicit-edge slabs)

DEV = torch.device("cuda:0")
P = 0.4
R = pi.R


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- 1. operator
def _seg(counts):
    return torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).to(torch.int32)


# rows x D: the issue's 37 x 64 (graph 3 owns no row), one row of one float4, more float4 columns than a wavefront has lanes
# (65), more rows than one launch has wavefronts (2 048 workgroups x 4: the grid stride)
SHAPES = {"37x64": ([9, 1, 14, 0, 13], 64), "1x4": ([0, 0, 1], 4), "9x260": ([2, 3, 0, 1, 3], 260),
          "8229x4": ([4000, 7, 0, 4200, 22], 4)}


@pytest.mark.usefixtures("poisoned_ops")
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_operator_is_segment_scale_of_keep_factors_at_every_order(shape):
    from equiformer_amd import droppath, ops
    counts, D = SHAPES[shape]
    seed, call = 7, 2  # keep_factors(7, 2, 5, 0.4) = keep [0, 0, 1, 0, 1]
    seg = _seg(counts).to(DEV)
    rows = int(seg.shape[0])
    f = droppath.keep_factors(seed, call, len(counts), P)
    assert (f > 0).tolist() == [False, False, True, False, True][:len(counts)]
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, D, generator=g)
    x[0, 0] = float("nan")  # a NaN in a row (dropped, except in the one-row case) stays a NaN: a multiply, not a select
    x = x.to(DEV).requires_grad_(True)
    x2 = x.detach().clone().requires_grad_(True)
    dy = torch.randn(rows, D, generator=g).to(DEV).requires_grad_(True)
    dy2 = dy.detach().clone().requires_grad_(True)
    w = torch.randn(rows, D, generator=g).to(DEV)
    fd = f.to(DEV)
    y = droppath.segment_droppath(x, seg, P, seed, call)
    y2 = ops.segment_scale(x2, fd, seg)
    assert torch.isnan(y[0, 0]) and torch.equal(_bits(y), _bits(y2))
    kept = fd[seg.long()] > 0
    assert bool((y[~kept][:, 1:] == 0).all())  # (+-0: the product with the factor 0)
    (dx,) = torch.autograd.grad(y, x, dy, create_graph=True)
    (dx2,) = torch.autograd.grad(y2, x2, dy2, create_graph=True)
    assert torch.equal(_bits(dx), _bits(dx2))
    (ddy,) = torch.autograd.grad((dx * w).sum(), dy)
    (ddy2,) = torch.autograd.grad((dx2 * w).sum(), dy2)
    assert torch.equal(_bits(ddy), _bits(ddy2)) and torch.equal(_bits(ddy), _bits(w * fd[seg.long()][:, None]))
    # plain first-order backward as well
    x3 = x.detach().clone().requires_grad_(True)
    droppath.segment_droppath(x3, seg, P, seed, call).backward(dy.detach())
    assert torch.equal(_bits(x3.grad), _bits(dx))
    # another call index: another mask
    assert (droppath.keep_factors(seed, 3, 5, P) > 0).tolist() == [True, True, False, False, True]
    y3 = droppath.segment_droppath(x.detach(), seg, P, seed, 3)
    assert torch.equal(_bits(y3), _bits(ops.segment_scale(x.detach(), droppath.keep_factors(seed, 3, 5, P).to(DEV), seg)))


@pytest.mark.usefixtures("poisoned_ops")
def test_operator_edges_no_rows_refused_width_and_split_seed():
    from equiformer_amd import droppath, lib, ops
    seg = _seg([9, 1, 14, 0, 13]).to(DEV)
    # rows = 0: nothing launched, an empty result with a gradient
    x0 = torch.zeros(0, 8, device=DEV, requires_grad=True)
    y0 = droppath.segment_droppath(x0, seg[:0], P, 7, 0)
    assert y0.shape == (0, 8)
    y0.sum().backward()
    assert x0.grad.shape == (0, 8)
    # D = 6: refused by status before any launch, the output buffer untouched
    x6 = torch.randn(37, 6, device=DEV)
    out = torch.full((37, 6), 3.5, device=DEV)
    with pytest.raises(lib.HipLibraryError):
        lib.call("eqf_segment_droppath", ops._p(x6), ops._p(seg), ops._p(out), 37, 6, P, 1.0 / (1.0 - P), 7, None, 0, ops._stream())
    with pytest.raises(lib.HipLibraryError):
        droppath.segment_droppath(x6, seg, P, 7, 0)
    torch.cuda.synchronize()
    assert bool((out == 3.5).all())
    # one total seed, by value or split between the by-value part and the device word (mod 2^64, the word read as unsigned)
    x = torch.randn(37, 64, generator=torch.Generator().manual_seed(1)).to(DEV)
    total = 2 ** 63 + 12345  # (beyond int64's positive range)

    def word(v):
        v &= (1 << 64) - 1
        return torch.tensor([v - (1 << 64) if v >= (1 << 63) else v], dtype=torch.int64, device=DEV)

    want = droppath.segment_droppath(x, seg, P, total, 1)
    assert torch.equal(want, ops.segment_scale(x, droppath.keep_factors(total, 1, 5, P).to(DEV), seg))
    splits = [(0, total), (total - 99, 99), (5, total - 5), ((1 << 64) - 3, total + 3), (total + 10, (1 << 64) - 10)]
    for by_value, w in splits:
        assert (by_value + w) % (1 << 64) == total
        got = droppath.segment_droppath(x, seg, P, by_value, 1, seed_word=word(w))
        assert torch.equal(got, want), (by_value, w)
    assert any(by_value + w >= (1 << 64) for by_value, w in splits), "no split wraps"
    assert not torch.equal(droppath.segment_droppath(x, seg, P, total + 1, 1), want)
    # the word is read when the kernel runs: rewriting it changes the next launch, the backward of an earlier forward follows it
    wd = word(total)
    xr = x.clone().requires_grad_(True)
    y = droppath.segment_droppath(xr, seg, P, 0, 1, seed_word=wd)
    (dx,) = torch.autograd.grad(y, xr, torch.ones_like(y))
    assert torch.equal(dx, droppath.keep_factors(total, 1, 5, P).to(DEV)[seg.long()][:, None].expand(37, 64))
    with pytest.raises(ops.HipOnlyError):
        droppath.segment_droppath(x, seg, P, 0, 1, seed_word=torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ops.HipOnlyError):
        droppath.segment_droppath(x, seg, P, 0, 1, seed_word=torch.zeros(1, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------------------------------------------------------- 2. model
class _Calls:
    def __init__(self):
        self.n = 0

    def next(self):
        self.n += 1
        return self.n - 1


def _oracle_draws(monkeypatch, seed, calls):
    """the fp64 oracle's stochastic depth, replaced for this test by the factors of `keep_factors` with a call counter"""
    from oracle import nets as onets
    from equiformer_amd import droppath

    def _drop_path(self, x, batch):
        if self.drop_path_rate == 0.0 or not self.training:
            return x
        f = droppath.keep_factors(seed, calls.next(), int(batch.max()) + 1, self.drop_path_rate)
        return x * f.to(x.dtype)[batch][:, None]

    monkeypatch.setattr(onets.TransBlock, "_drop_path", _drop_path)


def test_model_under_device_draws_matches_the_oracle(monkeypatch):
    import make_golden as mg
    from equiformer_amd import droppath
    seed = 7
    cfg = dict(mg.SMALL_OC20, number_of_basis=32, drop_path_rate=P, use_auxiliary_task=True)
    ref, mod = th._models(cfg)
    inp = th._slab(4, 16, seed=9)
    n_calls = 2 * cfg["num_layers"]
    keep = torch.stack([droppath.keep_factors(seed, c, 4, P) > 0 for c in range(n_calls)])
    assert bool(keep.any()) and not bool(keep.all()), "the test needs a dropped and a kept (call, graph)"
    ref.eval(); mod.eval()
    _, (e_eval, _) = th._run(ref, mod, inp)
    ref.train(); mod.train()
    calls = _Calls()
    _oracle_draws(monkeypatch, seed, calls)
    out_r = ref(inp[2], inp[3], inp[0].double(), inp[1], edge_index=inp[4], offsets=inp[5].double())
    assert calls.n == n_calls
    data = SimpleNamespace(pos=inp[0].to(DEV), batch=inp[1].to(DEV), atomic_numbers=inp[2].to(DEV), tags=inp[3].to(DEV),
                           edge_index=inp[4].to(DEV), offsets=inp[5].to(DEV))
    state = torch.get_rng_state()
    with droppath.device_draws(seed) as d:
        out = mod(data)
        assert d.calls == n_calls
    assert torch.equal(torch.get_rng_state(), state), "device draws consumed the CPU generator"
    print("device-drawn stochastic depth vs oracle: energy %.2e, vectors %.2e, train vs eval %.2e"
          % (th._rel(out[0], out_r[0]), th._rel(out[1], out_r[1]), th._rel(out[0], e_eval)))
    assert th._rel(out[0], out_r[0]) < 1e-4 and th._rel(out[1], out_r[1]) < 1e-4
    assert th._rel(out[0], e_eval) > 1e-3  # some branch was really dropped
    p_r = ref.blocks[0].ga.sep_act.lin.tp.weight
    p = mod.blocks[0].ga.sep_act.lin.tp.weight
    (gr,) = torch.autograd.grad(out_r[0].sum() + out_r[1].sum(), [p_r])
    (gg,) = torch.autograd.grad(out[0].sum() + out[1].sum(), [p])
    print("   probed parameter gradient %.2e" % th._rel(gg, gr))
    assert th._rel(gg, gr) < 2e-4
    # the same seed again: the same bits; another seed: other energies
    with droppath.device_draws(seed):
        again = mod(data)
    assert torch.equal(again[0], out[0]) and torch.equal(again[1], out[1])
    with droppath.device_draws(seed + 1):
        other = mod(data)
    assert not torch.equal(other[0], out[0])


# ------------------------------------------------------------------------------------------------ 3. padded equals unpadded
def _slab_model():
    """SMALL_OC20 with the IS2RS head and drop_path_rate 0.4 on its own periodic radius graph: tests/test_gpu_is2rs_step.py's
    model with stochastic depth switched on, the same initial weights at every call."""
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20
    cfg = dict(mg.SMALL_OC20, number_of_basis=32, alpha_drop=0.0, drop_path_rate=P, use_auxiliary_task=True)
    m = GraphAttentionTransformerOC20(None, None, 1, otf_graph=True, use_pbc=True, max_neighbors=pi.SLAB_CAP, **cfg)
    return fill_deterministic(m, 21).to(DEV).train()


_PADDED = {}
PAD_STEPS = (16, 256)  # node / edge steps of the bucket the padded view is built for: 2 446 edges -> 2 560


def _padded_and_unpadded(seed=7):
    """one forward of the slab model on the unpadded batch (its own periodic graph) and on the padded bucket view, both under
    device_draws(seed), and the padded one under seed + 1; the rows every GraphDropPath call zeroed.  Computed once."""
    from equiformer_amd import droppath
    from equiformer_amd.capture import bucket_of
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.nets.layers import GraphDropPath
    if _PADDED:
        return _PADDED
    m = _slab_model()
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in t6._slab_batch().items()}
    B, N = d["num_graphs"], d["pos"].shape[0]
    zeroed = []
    hooks = [mod.register_forward_hook(lambda mod, inp, out: zeroed.append((out == 0).all(dim=1)))
             for mod in m.modules() if isinstance(mod, GraphDropPath)]
    with torch.no_grad():
        with droppath.device_draws(seed):
            e0, v0 = m(SimpleNamespace(**d))
        z0 = list(zeroed)
        plan = EdgeGraph.radius_pbc_plan(d["pos"], d["cell"], d["batch"], R, pi.SLAB_CAP, B)
        cap = bucket_of(B, plan.N, plan.E, *PAD_STEPS)[1:]
        assert plan.E < cap[1] < 4000  # (batch and bucket on one side of the kernel-dispatch thresholds: see the bit-equality test)
        g, _, _ = EdgeGraph.from_radius_pbc(d["pos"], d["cell"], d["batch"], R, pi.SLAB_CAP, num_graphs=B, capacity=cap,
                                            z=d["atomic_numbers"])
        assert g.N > N and int(g.batch.max()) == B
        view = SimpleNamespace(pos=g.pos, batch=g.batch, atomic_numbers=g.z, offsets=g.offsets,
                               tags=torch.zeros(cap[0], dtype=torch.int64, device=DEV))
        view.tags[:N] = d["tags"]
        del zeroed[:]
        with droppath.device_draws(seed):
            e1, v1 = m(view, graph=g, offsets=g.offsets)
        z1 = list(zeroed)
        with droppath.device_draws(seed + 1):
            e2, _ = m(view, graph=g, offsets=g.offsets)
    for h in hooks:
        h.remove()
    _PADDED.update(B=B, N=N, batch=d["batch"], pbatch=g.batch, e0=e0, v0=v0, e1=e1, v1=v1, e2=e2, z0=z0, z1=z1, seed=seed)
    return _PADDED


def test_padded_view_drops_the_real_graphs_the_unpadded_batch_drops():
    """Call by call, the rows stochastic depth zeroes on the padded view are those it zeroes on the unpadded batch, and those
    `keep_factors` names -- the phantom molecule, graph B, has a draw of its own; the outputs of the real rows agree within
    the bound of test_oc20_model_parity_under_padding (1e-4)."""
    from equiformer_amd import droppath
    r = _padded_and_unpadded()
    B, N = r["B"], r["N"]
    keep = torch.stack([droppath.keep_factors(r["seed"], c, B + 1, P) > 0 for c in range(4)])
    assert bool(keep[:, :B].any()) and not bool(keep[:, :B].all())
    assert not bool(keep[:, B].all()), "the phantom molecule is dropped in some call of its own"
    assert len(r["z0"]) == len(r["z1"]) == 4
    for c in range(4):
        want = ~keep[c].to(DEV)
        assert torch.equal(r["z0"][c], want[r["batch"].long()]), c
        assert torch.equal(r["z1"][c], want[r["pbatch"].long()]), c
        assert torch.equal(r["z1"][c][:N], r["z0"][c]), c
    assert r["e1"].shape[0] == B + 1 and not torch.equal(r["e2"][:B], r["e1"][:B])
    print("padded vs unpadded under one seed: energies %.3e, vectors %.3e" % (t6._rel(r["e1"][:B], r["e0"]), t6._rel(r["v1"][:N], r["v0"])))
    assert t6._rel(r["e1"][:B], r["e0"]) < 1e-4 and t6._rel(r["v1"][:N], r["v0"]) < 1e-4


def test_padded_energies_are_bit_equal_to_unpadded():
    """The energies of the real structures (and the auxiliary vectors of the real atoms), padded against unpadded under one
    seed: bit-equal -- the phantom molecule takes no draw away from a real one.

    The bucket (PAD_STEPS: 2 446 edges padded to 2 560) lies on the batch's side of the kernel-dispatch thresholds, so both
    forwards run the same kernels.  A bucket beyond one is another matter, and not one of stochastic depth: with the 8 192-edge
    bucket of tests/test_gpu_is2rs_step.py the energies differ by 1.4e-6 (measured on an MI355X), in eval mode -- GraphDropPath
    the identity -- by 1.5e-6, while the zeroed rows stay equal call by call.  Every operator output before it being bit-equal on
    the real rows, the first to differ there (3.9e-7) is the gated fused SeparableFCTP forward of the first block:
    eqf_sfcx_fwd_gated serves fewer than 4 000 edges (Y_MIN_EDGES_GATED, csrc/sfcx.hip) with its one-wave kernel and more with the
    multi-wave kernel of sfcy.hip, which sums in another order (a measured speed choice that tests/test_gpu_sfc_edges.py pins)."""
    r = _padded_and_unpadded()
    e1, e0 = r["e1"][:r["B"]], r["e0"]
    print("padded vs unpadded energies: %s / %s, rel %.3e" % (e1.flatten().tolist(), e0.flatten().tolist(), t6._rel(e1, e0)))
    assert torch.equal(_bits(e1), _bits(e0)), (e1.flatten().tolist(), e0.flatten().tolist())
    assert torch.equal(_bits(r["v1"][:r["N"]]), _bits(r["v0"]))


# ---------------------------------------------------------------------------------------------------------- 4. captured step
def _train_slab(steps, captured, seed, lr=t6.LR, interpolate=True, weight=t6.W0, decay=True, min_eager=3, explicit=True):
    """tests/test_gpu_is2rs_step.py's `_train` on the model with stochastic depth: IS2RSTrainStep, or the eager unpadded loop
    whose step k runs under device_draws(step_seed(seed, k))"""
    from equiformer_amd import droppath
    from equiformer_amd.is2rs import (IS2RSLoss, IS2RSTrainStep, auxiliary_task_weight, interpolate_init_relaxed_pos, step_seed)
    from equiformer_amd.optim import FlatAdamW
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in t6._slab_batch().items()}
    m = _slab_model()
    opt = FlatAdamW(m.parameters(), lr=lr, weight_decay=1e-2)
    L = IS2RSLoss(auxiliary_task_weight=weight, **t6.NORM)
    total = steps if decay else None
    ts = None
    if captured:
        kw = dict(drop_path_seed=seed) if explicit else {}
        ts = IS2RSTrainStep(m, opt, L, R, pi.SLAB_CAP, interpolate=interpolate, seed=seed if not explicit else seed + 1,
                            total_steps=total, min_eager=min_eager, node_step=t6.NODE_STEP, edge_step=t6.EDGE_STEP, **kw)
    losses = []
    for k in range(steps):
        if captured:
            loss = ts.step(batch)
        else:
            data = SimpleNamespace(**batch)
            if interpolate:
                interpolate_init_relaxed_pos(data, seed=step_seed(seed if not explicit else seed + 1, k))
            if decay:
                L.set_weights(auxiliary_task_weight=auxiliary_task_weight(weight, k, steps))
            opt.zero_grad(set_to_none=True)
            with droppath.device_draws(step_seed(seed, k)):
                out = m(data)
                loss = L(out[0], out[1], data)
                loss.backward()
            opt.step()
            loss = loss.detach()
        losses.append(float(loss))
    torch.cuda.synchronize()
    return dict(losses=losses, ts=ts, p=opt.flat_p.detach().clone(), m=opt.flat_m.detach().clone(), step=opt._step)


def _masks(seed, steps, B=4, calls=4):
    """[step][call] -> kept real graphs, from keep_factors"""
    from equiformer_amd import droppath
    from equiformer_amd.is2rs import step_seed
    return [[(droppath.keep_factors(step_seed(seed, k), c, B, P) > 0).tolist() for c in range(calls)] for k in range(steps)]


def test_captured_step_with_stochastic_depth_equals_eager_loop():
    """The 8-step protocol of test_captured_step_equals_eager_loop with drop_path_rate 0.4: 3 eager padded steps, one capture,
    5 replays against 8 eager unpadded steps under device_draws(step_seed(s, k)).  Measured on an MI355X: losses 8.2e-6
    (bound 2e-5), first moments 3.8e-6 (5e-4), parameters above noise 1.4e-5 (1e-4)."""
    s = 4242
    masks = _masks(s, 8)
    replayed = masks[3:]
    assert any(a != b for i, a in enumerate(replayed) for b in replayed[i + 1:]), "the replayed steps share one mask"
    assert any(not kept for step in replayed for call in step for kept in call), "no real graph is dropped during the replays"
    assert any(kept for step in replayed for call in step for kept in call)
    e = _train_slab(8, False, s)
    b = _train_slab(8, True, s)
    ts = b["ts"]
    assert (ts.eager_steps, ts.captures, ts.replays) == (3, 1, 5), (ts.eager_steps, ts.captures, ts.replays)
    print("losses eager %s\n    captured %s" % (e["losses"], b["losses"]))
    t6._assert_trains_as_eager(e, b, 8, t6.LR)


def test_replays_draw_fresh_masks():
    """Learning rate 0, no perturbation, a constant loss weight: the replays of one batch differ by their masks only.  Each
    loss equals the eager unpadded loss under that step's seed within 2e-5 (the auxiliary weight is 1: losses of order one).
    `drop_path_seed` is left to its default, the step's own seed."""
    s = 99
    steps = 6
    masks = _masks(s, steps)
    assert any(a != b for i, a in enumerate(masks[2:]) for b in masks[2:][i + 1:])
    kw = dict(lr=0.0, interpolate=False, weight=1.0, decay=False, explicit=False)
    b = _train_slab(steps, True, s, min_eager=1, **kw)
    ts = b["ts"]
    assert (ts.eager_steps, ts.captures, ts.replays) == (1, 1, steps - 1)
    e = _train_slab(steps, False, s, **kw)
    print("losses eager %s\n    captured %s" % (e["losses"], b["losses"]))
    assert len({round(x, 6) for x in b["losses"][1:]}) >= 2, "every replay returned one loss: a frozen mask"
    for k, (x, y) in enumerate(zip(e["losses"], b["losses"])):
        assert abs(x) < 10 and abs(x - y) <= 2e-5, (k, x, y)
    # two steps with the same masks give the same loss, two with different masks a different one
    for i in range(steps):
        for j in range(i + 1, steps):
            if masks[i] == masks[j]:
                assert abs(b["losses"][i] - b["losses"][j]) <= 2e-5


# ------------------------------------------------------------------------------------------------------------ 5. non-periodic
def test_bucketed_step_on_molecules_equals_eager_loop():
    """SMALL_L2 on a QM9-like batch, drop_path_rate 0.4, min_eager=1: one eager padded step, the capture, 3 replays against 4
    eager unpadded steps; the bounds of tests/test_gpu_bucketed_capture.py.  Measured on an MI355X: losses 6.5e-6, moments
    2.5e-6, parameters above noise 1.5e-6."""
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd import droppath
    from equiformer_amd.capture import BucketedTrainStep
    from equiformer_amd.dens import step_seed
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    from equiformer_amd.optim import FlatAdamW
    s, steps, lr = 31, 4, 1e-3
    d = tb._varying(1)[0]
    B = d["num_graphs"]
    masks = _masks(s, steps, B=B, calls=2 * mg.SMALL_L2["num_layers"])
    assert any(a != b for i, a in enumerate(masks[1:]) for b in masks[1:][i + 1:]), "the replayed steps share one mask"
    assert any(not kept for step in masks[1:] for call in step for kept in call)

    def train(bucketed):
        m = GraphAttentionTransformer(irreps_in="5x0e", max_radius=tb.R, number_of_basis=32,
                                      **dict(mg.SMALL_L2, alpha_drop=0.0, drop_path_rate=P))
        m = fill_deterministic(m, 21).to(DEV).train()
        opt = FlatAdamW(m.parameters(), lr=lr, weight_decay=1e-2)
        bs = BucketedTrainStep(opt, tb._padded_loss(m), tb.R, node_step=tb.NODE_STEP, edge_step=tb.EDGE_STEP, min_eager=1,
                               drop_path_seed=s) if bucketed else None
        losses = []
        for k in range(steps):
            if bucketed:
                loss = bs.step(d)
            else:
                opt.zero_grad(set_to_none=True)
                with droppath.device_draws(step_seed(s, k)):
                    loss = tb._unpadded_loss(m, d)
                    loss.backward()
                opt.step()
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        return dict(losses=losses, p=opt.flat_p.detach().clone(), m=opt.flat_m.detach().clone(), step=opt._step, bs=bs)

    e, b = train(False), train(True)
    bs = b["bs"]
    assert (bs.eager_steps, bs.captures, bs.replays) == (1, 1, 3), (bs.eager_steps, bs.captures, bs.replays)
    print("losses eager %s\n    captured %s" % (e["losses"], b["losses"]))
    tb._assert_trains_as_eager(e, b, steps, lr)


def test_default_seed_is_drawn_once_and_only_by_a_model_that_drops():
    """drop_path_seed=None: the base seed comes from torch's CPU generator when the first GraphDropPath runs under the instance;
    a model without stochastic depth leaves the generator alone (alpha_drop is 0 here: nothing else draws)."""
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.capture import BucketedTrainStep
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    from equiformer_amd.optim import FlatAdamW
    d = tb._varying(1)[0]

    def run(rate, steps=3):
        m = GraphAttentionTransformer(irreps_in="5x0e", max_radius=tb.R, number_of_basis=32,
                                      **dict(mg.SMALL_L2, alpha_drop=0.0, drop_path_rate=rate))
        m = fill_deterministic(m, 21).to(DEV).train()
        opt = FlatAdamW(m.parameters(), lr=0.0, weight_decay=0.0)
        bs = BucketedTrainStep(opt, tb._padded_loss(m), tb.R, node_step=tb.NODE_STEP, edge_step=tb.EDGE_STEP, min_eager=1)
        torch.manual_seed(11)
        losses = [float(bs.step(d)) for _ in range(steps)]
        return bs, losses, torch.get_rng_state()

    torch.manual_seed(11)
    for _ in range(3 + 1):  # the attention-dropout seed word: one draw per step and one more at the capture, as before
        torch.randint(0, 2 ** 62, (1,))
    plain_state = torch.get_rng_state()
    torch.randint(0, 2 ** 62, (1,))
    one_more = torch.get_rng_state()
    bs0, _, state0 = run(0.0)
    assert torch.equal(state0, plain_state), "a model without stochastic depth consumed the generator"
    assert bs0._drop_path._drawn is None
    bs1, losses1, state1 = run(P)
    assert bs1._drop_path._drawn is not None and len(set(losses1)) > 1, losses1
    assert torch.equal(state1, one_more), "the base seed is one draw, taken once"
