"""The IS2RE + IS2RS training step on the GPU (equiformer_amd/is2rs.py, csrc/is2rs.hip): the perturbation's exact invariants and
its sampling statistics, the fused loss + metrics and its gradient against the float64 restatement of tests/fp64_is2rs.py, no
hidden host synchronisation, the model with the fused loss against the fp64 oracle, and the captured step against the eager
loop.  Statistical bounds are five standard deviations of the exact sampling distribution; the loss tolerance (1e-6) is fp64
arithmetic up to the final fp32 store (2^-24); the trajectory bounds are those of tests/test_gpu_periodic_capture.py.
Wall time of this file on an MI355X, one run each (pytest's figure): 5.7 s at the parent commit, 5.2 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py)."""
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import fp64_is2rs as fi  # noqa: E402
import periodic_inputs as pi  # noqa: E402
from poison import poisoned_ops  # noqa: E402,F401  (the fixture of the tests that run on poisoned, guarded allocations)

R = pi.R
DEV = torch.device("cuda:0")


def _structures(N):
    """batch [N] of structures of unequal size, a one-atom structure among them."""
    sizes, left = [], N
    for s in (1, 7, 20, 36):
        if left <= 0:
            break
        sizes.append(min(s, left))
        left -= sizes[-1]
    if left > 0:
        sizes.append(left)
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def _perturb_inputs(N, tags, seed=0):
    g = torch.Generator().manual_seed(seed)
    pos = torch.randn(N, 3, generator=g) * 2
    pos_relaxed = pos + 0.3 * torch.randn(N, 3, generator=g)
    t = {"mixed": torch.randint(0, 3, (N,), generator=g), "none": torch.zeros(N, dtype=torch.int64),
         "all": torch.randint(1, 3, (N,), generator=g)}[tags]
    return pos, pos_relaxed, t, _structures(N)


def _perturb(pos, pos_relaxed, tags, batch, seed, **kw):
    from equiformer_amd.is2rs import interpolate_init_relaxed_pos
    dpos = pos.to(DEV)
    data = SimpleNamespace(pos=dpos, pos_relaxed=pos_relaxed.to(DEV), tags=tags.to(DEV), batch=batch.to(DEV))
    out = interpolate_init_relaxed_pos(data, seed=seed, **kw)
    assert out is data and data.pos is not dpos
    assert torch.equal(dpos.cpu().view(torch.int32), pos.view(torch.int32)), "the caller's pos was written"
    assert torch.equal(data.pos_relaxed.cpu(), pos_relaxed) and torch.equal(data.tags.cpu(), tags)
    return tuple(t.cpu() for t in (data.pos, data.interpolate_factor, data.noise_vec, data.perturbed))


# -------------------------------------------------------------------------------------------------- 1. perturbation, exact
@pytest.mark.usefixtures("poisoned_ops")
@pytest.mark.parametrize("p_perturb", [0.5, 1.0, 0.0])
@pytest.mark.parametrize("tags", ["mixed", "none", "all"])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_perturbation_invariants(N, tags, p_perturb):
    pos, pos_relaxed, t, batch = _perturb_inputs(N, tags, seed=N)
    f_min = 0.25 if N == 65 else 0.0
    kw = dict(p_perturb=p_perturb, f_min=f_min)
    a = _perturb(pos, pos_relaxed, t, batch, 1234, **kw)
    b = _perturb(pos, pos_relaxed, t, batch, 1234, **kw)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "the same seed gave other bits"
    c = _perturb(pos, pos_relaxed, t, batch, 1235, **kw)
    assert not torch.equal(a[2], c[2]) and not torch.equal(a[1], c[1]), "another seed gave the same noise"
    moved = fi.check_perturbation(pos, pos_relaxed, t, batch, a, f_min)
    assert (a[2] != 0).any(dim=1).all(), "noise_vec is filled on every row, moved or not"
    selected = a[3]
    if p_perturb == 1.0:
        assert selected.all() and torch.equal(moved, t > 0)
    if p_perturb == 0.0:
        assert not selected.any() and torch.equal(a[0].view(torch.int32), pos.view(torch.int32))
    if tags == "none":
        assert not moved.any() and torch.equal(a[0].view(torch.int32), pos.view(torch.int32))
    if tags == "all":
        assert torch.equal(moved, selected)
    # int32 tags: the same bits
    if N == 257:
        d = _perturb(pos, pos_relaxed, t.to(torch.int32), batch, 1234, **kw)
        assert all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for x, y in zip(a, d))


# -------------------------------------------------------------------------------------------- 2. perturbation, statistical
def test_perturbation_statistics():
    B, A, p, std = 4096, 16, 0.5, 0.3
    g = torch.Generator().manual_seed(0)
    pos = torch.randn(B * A, 3, generator=g)
    pos_relaxed = pos + 0.3 * torch.randn(B * A, 3, generator=g)
    tags = torch.randint(0, 3, (B * A,), generator=g)
    batch = torch.repeat_interleave(torch.arange(B), A)
    _, factor, noise_vec, selected = _perturb(pos, pos_relaxed, tags, batch, 20240607, p_perturb=p, noise_std=std)
    share = selected.view(B, A)[:, 0].double().mean().item()
    bound = 5 * math.sqrt(p * (1 - p) / B)
    print("selected structures %.4f (0.5 +- %.4f)" % (share, bound))
    assert abs(share - p) <= bound
    f = factor.double()
    n = f.numel()
    # a uniform on [0, 1): mean 1/2, variance 1/12, fourth central moment 1/80 -> Var(s^2) = (1/80 - 1/144) / n = 1 / (180 n)
    print("factor mean %.5f (0.5 +- %.5f), variance %.6f (%.6f +- %.6f)"
          % (f.mean().item(), 5 * math.sqrt(1 / (12 * n)), f.var().item(), 1 / 12, 5 * math.sqrt(1 / (180 * n))))
    assert abs(f.mean().item() - 0.5) <= 5 * math.sqrt(1 / (12 * n))
    assert abs(f.var().item() - 1 / 12) <= 5 * math.sqrt(1 / (180 * n))
    x = noise_vec.double().flatten()
    n = x.numel()
    mean, s = x.mean().item(), x.std().item()
    print("noise mean %.3e (+- %.3e), std / 0.3 - 1 = %.3e (+- %.3e)" % (mean, 5 * std / math.sqrt(n), s / std - 1, 5 / math.sqrt(2 * n)))
    assert abs(mean) <= 5 * std / math.sqrt(n)
    assert abs(s / std - 1) <= 5 / math.sqrt(2 * n)
    p2 = math.erfc(2 / math.sqrt(2))  # 0.0455
    tail = (x.abs() > 2 * std).double().mean().item()
    bound = 5 * math.sqrt(p2 * (1 - p2) / n)
    print("share beyond two sigma %.5f (%.5f +- %.5f)" % (tail, p2, bound))
    assert abs(p2 - 0.0455) < 1e-4 and abs(tail - p2) <= bound
    c = x - x.mean()
    lag1 = ((c[:-1] * c[1:]).sum() / (c * c).sum()).item()
    print("lag-1 correlation %.3e (+- %.3e)" % (lag1, 5 / math.sqrt(n)))
    assert abs(lag1) <= 5 / math.sqrt(n)


# ------------------------------------------------------------------------------------------------- 3. loss against fp64
E_MEAN, E_STD = 0.4, 1.7
P_MEAN = (0.25, -0.5, 0.125)  # exact in fp32: a row whose displacement is P_MEAN has a target of exactly 0


def _loss_inputs(N, nB, tags, phantom, seed):
    g = torch.Generator().manual_seed(seed)
    d = dict(pred_y=torch.randn(nB, 1, generator=g), pred_pos=torch.randn(N, 3, generator=g),
             y=torch.randn(nB, generator=g) * 3 + 0.4, pos=torch.randn(N, 3, generator=g) * 2)
    d["pos_relaxed"] = d["pos"] + 0.4 * torch.randn(N, 3, generator=g)
    d["tags"] = {"mixed": torch.randint(0, 3, (N,), generator=g), "all": torch.randint(1, 3, (N,), generator=g),
                 "none": torch.zeros(N, dtype=torch.int64)}[tags]
    if nB == 3:  # one structure inside the threshold, two (almost surely) outside
        d["pred_y"][0, 0] = (d["y"][0] - E_MEAN) / E_STD
    d["row_mask"] = None
    if phantom and N > 1:
        k = max(1, N // 8)
        d["row_mask"] = torch.ones(N)
        d["row_mask"][-k:] = 0.0
        d["pred_pos"][-k:] = 3.0e37  # large finite garbage on the phantom rows
        d["tags"][-k:] = 1           # which would count as free
    if N > 1:  # one real free row whose difference is exactly zero in fp64
        d["pos"][0] = 0.0
        d["pos_relaxed"][0] = torch.tensor(P_MEAN)
        d["pred_pos"][0] = 0.0
        if tags != "none":
            d["tags"][0] = 1
    return d


def _close(got, want, what, tol=1e-6):
    got, want = got.detach().double().cpu(), want.detach().double()
    err = (got - want).abs().max().item()
    assert err <= tol * want.abs().max().item(), (what, err, want.abs().max().item())


@pytest.mark.usefixtures("poisoned_ops")
@pytest.mark.parametrize("phantom", [False, True])
@pytest.mark.parametrize("tags", ["mixed", "all", "none"])
@pytest.mark.parametrize("nB", [1, 3])
@pytest.mark.parametrize("N", [1, 64, 65, 256, 257, 1025])
def test_loss_forward_backward_against_fp64(N, nB, tags, phantom):
    from equiformer_amd.is2rs import IS2RSLoss
    d = _loss_inputs(N, nB, tags, phantom, seed=7 * N + nB)
    up = 0.37  # upstream gradient
    p_std = (0.4, 0.7, 1.3) if N == 65 else 0.6
    tag_dtype = torch.int32 if N == 257 else torch.int64
    L = IS2RSLoss(E_MEAN, E_STD, P_MEAN, p_std, 15.0, energy_weight=1.0, threshold=0.02)
    w32 = [float(torch.tensor(w, dtype=torch.float32)) for w in (1.0, 15.0)]  # the device words are fp32

    def run(weights):
        py, pp = d["pred_y"].double().requires_grad_(True), d["pred_pos"].double().requires_grad_(True)
        rm = None if d["row_mask"] is None else d["row_mask"] > 0
        loss, stats = fi.is2rs_loss(py, pp, d["y"], d["pos"], d["pos_relaxed"], d["tags"], weights, E_MEAN, E_STD, P_MEAN, p_std,
                                    threshold=0.02, row_mask=rm)
        gy, gp = torch.autograd.grad(loss * up, [py, pp], allow_unused=True)
        gp = torch.zeros_like(pp) if gp is None else gp
        if rm is not None:  # rows the restatement dropped: zero gradient
            assert gp[~rm].abs().sum() == 0
        return loss.detach(), stats, gy, gp

    def run_gpu():
        py, pp = d["pred_y"].to(DEV).requires_grad_(True), d["pred_pos"].to(DEV).requires_grad_(True)
        data = SimpleNamespace(y=d["y"].to(DEV), pos=d["pos"].to(DEV), pos_relaxed=d["pos_relaxed"].to(DEV),
                               tags=d["tags"].to(DEV, tag_dtype))
        loss = L(py, pp, data, row_mask=None if d["row_mask"] is None else d["row_mask"].to(DEV))
        assert loss.dim() == 0 and loss.dtype == torch.float32
        stats = L.stats.clone()
        (loss * up).backward()
        return loss.detach(), stats, py.grad, pp.grad

    want = run(w32)
    got = run_gpu()
    again = run_gpu()
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two calls differ"
    loss, stats, gy, gp = got
    assert torch.isfinite(loss) and torch.isfinite(stats).all() and torch.isfinite(gy).all() and torch.isfinite(gp).all()
    _close(loss, want[0], "loss")
    for i, name in enumerate(fi.STATS):
        _close(stats[i], want[1][i], name)
    assert stats[2].item() == want[1][2].item(), "n_free"
    assert stats[7].item() == 0
    if nB == 3:
        assert stats[5].item() > 0, "one structure lies inside the threshold"
    if tags == "none":
        assert stats[2].item() == 0 and stats[1].item() == 0 and stats[6].item() == 0
        assert gp.abs().sum().item() == 0, "no free atom: exactly zero position gradients"
    _close(gy, want[2], "d_pred_y")
    _close(gp, want[3], "d_pred_pos")
    if d["row_mask"] is not None:
        assert gp[d["row_mask"].to(DEV) == 0].abs().sum().item() == 0, "phantom rows must get exact zeros"
    assert gp[(d["tags"] <= 0).to(DEV)].abs().sum().item() == 0, "fixed atoms must get exact zeros"
    if N > 1:
        assert gp[0].abs().sum().item() == 0, "zero difference: the subgradient is 0"
        if tags != "none":
            assert want[1][2].item() >= 1
    # other device weights, nothing rebuilt
    L.set_weights(2.0, 8.0)
    want2 = run([2.0, 8.0])
    got2 = run_gpu()
    _close(got2[0], want2[0], "loss after set_weights")
    _close(got2[3], want2[3], "d_pred_pos after set_weights")
    L.set_weights(auxiliary_task_weight=1.0)
    want3 = run([2.0, 1.0])
    _close(run_gpu()[0], want3[0], "loss after a partial set_weights")


# ------------------------------------------------------------------------------------------------------ 4. no hidden syncs
def test_no_host_synchronisation():
    from equiformer_amd.is2rs import IS2RSLoss, interpolate_init_relaxed_pos
    pos, pos_relaxed, tags, batch = _perturb_inputs(65, "mixed", seed=3)
    data = SimpleNamespace(pos=pos.to(DEV), pos_relaxed=pos_relaxed.to(DEV), tags=tags.to(DEV), batch=batch.to(DEV),
                           y=torch.randn(5).to(DEV))
    py = torch.randn(5, 1).to(DEV).requires_grad_(True)
    pp = torch.randn(65, 3).to(DEV).requires_grad_(True)
    row_mask = torch.ones(65, device=DEV)
    L = IS2RSLoss(E_MEAN, E_STD, P_MEAN, 0.6, 15.0)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        interpolate_init_relaxed_pos(data, seed=11)
        L.set_weights(1.0, 8.0)
        loss = L(py, pp, data, row_mask=row_mask)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(pp.grad).all() and L.stats[2].item() == int((tags > 0).sum())


# -------------------------------------------------------------------------------------------------------- 5. model level
NORM = dict(target_mean=0.3, target_std=1.7, positions_mean=(0.01, -0.02, 0.03), positions_std=(0.4, 0.5, 0.6))
HEADS = {"aux": dict(use_auxiliary_task=True), "attn_aux": dict(use_attention_head=True, use_auxiliary_task=True)}
_REF = {}  # the fp64 oracle models, built once (nothing trains them: their gradients come from autograd.grad)


def _models(head="aux"):
    import make_golden as mg
    from oracle import nets as onets
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20
    cfg = dict(mg.SMALL_OC20, number_of_basis=32, alpha_drop=0.0, drop_path_rate=0.0, **HEADS[head])
    if head not in _REF:
        _REF[head] = fill_deterministic(onets.GraphAttentionTransformerOC20(**cfg), 21).double().train()
    ref = _REF[head]
    mod = GraphAttentionTransformerOC20(None, None, 1, otf_graph=True, use_pbc=True, max_neighbors=pi.SLAB_CAP, **cfg)
    mod.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return ref, mod.to(DEV).train()


_BATCH = []


def _slab_batch():
    """the first slab batch (4 structures) with relaxed positions: pos + 0.2 randn on the free atoms, the others unchanged"""
    if not _BATCH:
        d = pi.slab_batches(2)[0]
        g = torch.Generator().manual_seed(17)
        free = (d["tags"] > 0).view(-1, 1)
        d["pos_relaxed"] = torch.where(free, d["pos"] + 0.2 * torch.randn(d["pos"].shape, generator=g), d["pos"])
        _BATCH.append(d)
    return _BATCH[0]


def _data(d, **over):
    b = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}
    b.update(over)
    return SimpleNamespace(**b)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def test_model_with_fused_loss_against_fp64_oracle():
    from oracle import pbc
    from equiformer_amd.is2rs import IS2RSLoss, interpolate_init_relaxed_pos
    ref, mod = _models()
    d = _slab_batch()
    N = d["pos"].shape[0]
    data = _data(d)
    interpolate_init_relaxed_pos(data, seed=5, p_perturb=1.0)
    n_free = int((d["tags"] > 0).sum())
    assert 0 < n_free < N and bool(data.perturbed.all())
    assert int((data.pos.cpu() != d["pos"]).any(dim=1).sum()) == n_free
    weights = (1.0, 15.0)
    L = IS2RSLoss(auxiliary_task_weight=weights[1], energy_weight=weights[0], **NORM)
    E, V = mod(data)  # the model's own periodic radius graph
    loss = L(E, V, data)
    gg = torch.autograd.grad(loss, list(mod.parameters()), allow_unused=True)
    pos_cpu = data.pos.detach().cpu()
    ei, off, nb = pbc.radius_graph_pbc(pos_cpu, d["cell"], [int(n) for n in d["natoms"]], R, pi.SLAB_CAP)
    cart = torch.bmm(off.double().view(-1, 1, 3), torch.repeat_interleave(d["cell"].double(), nb, dim=0)).view(-1, 3)
    Er, Vr = ref(d["atomic_numbers"], d["tags"], pos_cpu.double(), d["batch"], edge_index=ei, offsets=cart)
    loss_r, stats_r = fi.is2rs_loss(Er, Vr, d["y"], pos_cpu, d["pos_relaxed"], d["tags"], weights, NORM["target_mean"],
                                    NORM["target_std"], NORM["positions_mean"], NORM["positions_std"])
    gr = torch.autograd.grad(loss_r, list(ref.parameters()), allow_unused=True)
    print("E rel %.2e, vectors rel %.2e, loss rel %.2e, %d edges" % (_rel(E, Er), _rel(V, Vr), _rel(loss, loss_r), ei.shape[1]))
    assert _rel(E, Er) < 1e-4 and _rel(V, Vr) < 1e-4 and _rel(loss, loss_r) < 1e-4
    assert L.stats[2].item() == stats_r[2].item() == n_free
    for i in (0, 1, 3, 4, 6):
        assert abs(L.stats[i].item() - stats_r[i].item()) <= 1e-4 * abs(stats_r[i].item()), (fi.STATS[i], L.stats, stats_r)
    gg_by_name = dict(zip([n for n, _ in mod.named_parameters()], gg))
    scale = max(r.abs().max().item() for r in gr if r is not None)
    worst = ("", 0.0)
    for (n, _), r in zip(ref.named_parameters(), gr):
        x = gg_by_name[n]
        if r is None or r.abs().max() == 0:
            assert x is None or x.abs().max().item() <= 1e-6 * scale, n
            continue
        assert x is not None, n
        e = (x.double().cpu() - r).abs().max().item() / max(r.abs().max().item(), 1e-3 * scale)
        if e > worst[1]:
            worst = (n, e)
    print("   worst parameter gradient of the fused loss %s %.2e" % worst)
    assert worst[1] < 2e-4, worst


# ------------------------------------------------------------------------------------------------------ 6. captured step
NODE_STEP, EDGE_STEP = 64, 8192  # N <= 144 atoms, at most N * SLAB_CAP = 7 200 edges: one bucket whatever the noise does
W0, LR = 15.0, 5e-4  # (the learning rate of the DeNS step's test)


def _assert_trains_as_eager(e, b, steps, max_lr):
    """tests/test_gpu_periodic_capture.py (copied): losses 2e-5 max(1, |loss|), first moments 5e-4, parameters whose moment is
    above noise 1e-4"""
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


def _train(head, steps, captured, interpolate=True, min_eager=3, seed=99):
    """`steps` steps on the slab batch, the auxiliary weight decaying from W0 over `steps` steps: IS2RSTrainStep, or the eager
    loop in which the model builds its own unpadded periodic graph"""
    from equiformer_amd.is2rs import (IS2RSLoss, IS2RSTrainStep, auxiliary_task_weight, interpolate_init_relaxed_pos, step_seed)
    from equiformer_amd.optim import FlatAdamW
    d = _slab_batch()
    batch = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}
    _, m = _models(head)
    opt = FlatAdamW(m.parameters(), lr=LR, weight_decay=1e-2)
    L = IS2RSLoss(auxiliary_task_weight=W0, **NORM)
    ts = IS2RSTrainStep(m, opt, L, R, pi.SLAB_CAP, interpolate=interpolate, seed=seed, total_steps=steps, min_eager=min_eager,
                        node_step=NODE_STEP, edge_step=EDGE_STEP) if captured else None
    losses, stats, positions, moved = [], [], [], []
    for k in range(steps):
        if captured:
            loss = ts.step(batch)
            last = ts.last
            positions.append(last["pos"].cpu())
            moved.append((last["perturbed"] & (batch["tags"] > 0)).cpu() if interpolate else None)
        else:
            data = SimpleNamespace(**batch)
            if interpolate:
                interpolate_init_relaxed_pos(data, seed=step_seed(seed, k))
            L.set_weights(auxiliary_task_weight=auxiliary_task_weight(W0, k, steps))
            opt.zero_grad(set_to_none=True)
            out = m(data)
            loss = L(out[0], out[1], data)
            loss.backward()
            opt.step()
            loss = loss.detach()
            positions.append(data.pos.cpu())
            moved.append((data.perturbed & (data.tags > 0)).cpu() if interpolate else None)
        losses.append(float(loss))
        stats.append(L.stats.cpu())
    torch.cuda.synchronize()
    assert torch.equal(batch["pos"].cpu(), d["pos"]), "the step must not move the caller's atoms"
    return dict(losses=losses, stats=stats, positions=positions, moved=moved, ts=ts, p=opt.flat_p.detach().clone(),
                m=opt.flat_m.detach().clone(), step=opt._step)


def test_captured_step_equals_eager_loop():
    """One slab batch of 4 structures, 8 steps, the auxiliary weight decaying from 15 on every step: 3 eager padded steps, one
    capture, 5 replays against 8 eager unpadded steps with the same seeds.  Measured on an MI355X: losses 5.8e-6 (bound 2e-5),
    first moments 6.5e-6 (5e-4), parameters above noise 1.3e-5 (1e-4): the bounds of the periodic capture tests, unchanged."""
    from equiformer_amd.capture import bucket_of
    from equiformer_amd.is2rs import auxiliary_task_weight
    d = _slab_batch()
    N = d["pos"].shape[0]
    assert N <= 144 and bucket_of(4, N, 1, NODE_STEP, EDGE_STEP) == bucket_of(4, N, N * pi.SLAB_CAP, NODE_STEP, EDGE_STEP)
    e = _train("aux", 8, False)
    b = _train("aux", 8, True)
    ts = b["ts"]
    assert (ts.eager_steps, ts.captures, ts.replays) == (3, 1, 5), (ts.eager_steps, ts.captures, ts.replays)
    n_free = int((d["tags"] > 0).sum())
    for k in range(8):
        assert torch.equal(e["moved"][k], b["moved"][k]), "step %d moved other atoms" % k
        assert torch.equal(e["positions"][k].view(torch.int32), b["positions"][k].view(torch.int32)), "step %d: other positions" % k
        assert e["stats"][k][2].item() == b["stats"][k][2].item() == n_free, (k, e["stats"][k], b["stats"][k])
        # the loss a replay returns is made of the device weight of that step
        w_k = auxiliary_task_weight(W0, k, 8)
        made = b["stats"][k][0].item() + w_k * b["stats"][k][1].item()
        assert abs(made - b["losses"][k]) <= 1e-5 * max(1.0, abs(b["losses"][k])), (k, w_k, made, b["losses"][k])
    assert [auxiliary_task_weight(W0, k, 8) for k in (0, 4, 7)] == [15.0, 8.0, 2.75]
    assert any(not torch.equal(b["positions"][i], b["positions"][j]) for i in range(3, 8) for j in range(i + 1, 8)), \
        "the replays saw one set of positions"
    assert any(bool(mk.any()) for mk in b["moved"][3:]), "no replay moved an atom"
    _assert_trains_as_eager(e, b, 8, LR)


# ------------------------------------------------------------------------------------------------------------ 7. variants
@pytest.mark.parametrize("head,interpolate", [("attn_aux", True), ("aux", False)])
def test_captured_step_variants(head, interpolate):
    """The attention-head model (its vectors are a column slice of the head's output), and the _aux configurations that do not
    perturb: 4 steps, one eager, the capture, 3 replays."""
    d = _slab_batch()
    e = _train(head, 4, False, interpolate=interpolate)
    b = _train(head, 4, True, interpolate=interpolate, min_eager=1)
    ts = b["ts"]
    assert (ts.eager_steps, ts.captures, ts.replays) == (1, 1, 3), (ts.eager_steps, ts.captures, ts.replays)
    print("%s, interpolate=%s: losses eager %s captured %s" % (head, interpolate, e["losses"], b["losses"]))
    for x, y in zip(e["losses"], b["losses"]):
        assert abs(x - y) <= 2e-5 * max(1.0, abs(x)), (e["losses"], b["losses"])
    if not interpolate:
        n_free = int((d["tags"] > 0).sum())
        for k in range(4):
            assert torch.equal(b["positions"][k], d["pos"]), "positions moved without the perturbation"
            assert b["stats"][k][2].item() == n_free
        assert "perturbed" not in ts.last
