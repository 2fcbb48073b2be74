"""The DeNS training step on the GPU (equiformer_amd/dens.py, csrc/dens.hip): the corruption's exact invariants and its
sampling statistics, the fused loss + metrics and its gradient against the float64 restatement of tests/fp64_dens.py, no
hidden host synchronisation, the model with the fused loss against the fp64 oracle, and the captured step against the eager
loop.  Statistical bounds are five standard deviations of the exact sampling distribution; the loss tolerance (1e-6) is fp64
arithmetic up to the final fp32 store (2^-24).
Wall time of this file on an MI355X, one run each (pytest's figure): 5.6 s at the parent commit, 5.8 s with every allocation
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
import fp64_dens as fd  # noqa: E402
from poison import poisoned_ops  # noqa: E402,F401  (the fixture of the tests that run on poisoned, guarded allocations)

R = 5.0
DEV = torch.device("cuda:0")


def _molecules(N):
    """batch [N] of molecules of unequal size, a one-atom molecule among them."""
    sizes, left = [], N
    for s in (1, 7, 20, 36):
        if left <= 0:
            break
        sizes.append(min(s, left))
        left -= sizes[-1]
    if left > 0:
        sizes.append(left)
    return torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


def _corrupt_inputs(N, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, 3, generator=g) * 2, torch.randn(N, 3, generator=g), _molecules(N)


def _corrupt(pos, dy, batch, std, prob, ratio, seed):
    from equiformer_amd.dens import add_masked_gaussian_noise_to_pos
    data = SimpleNamespace(pos=pos.to(DEV), dy=dy.to(DEV), batch=batch.to(DEV))
    out = add_masked_gaussian_noise_to_pos(data, std, prob, ratio, seed=seed)
    assert out is data and torch.equal(data.dy.cpu(), dy)
    return tuple(t.cpu() for t in (data.pos, data.force, data.noise_vec, data.noise_mask, data.denoising_pos_mask))


# ---------------------------------------------------------------------------------------------------- 1. corruption, exact
@pytest.mark.usefixtures("poisoned_ops")
@pytest.mark.parametrize("prob,ratio", [(0.5, None), (0.5, 0.5), (1.0, None), (0.0, None), (1.0, 1.0), (1.0, 0.0), (0.0, 1.0)])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_corruption_invariants(N, prob, ratio):
    pos, dy, batch = _corrupt_inputs(N, seed=N)
    a = _corrupt(pos, dy, batch, 0.1, prob, ratio, seed=1234)
    b = _corrupt(pos, dy, batch, 0.1, prob, ratio, seed=1234)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "the same seed gave other bits"
    c = _corrupt(pos, dy, batch, 0.1, prob, ratio, seed=1235)
    assert not torch.equal(a[2], c[2]), "another seed gave the same noise"
    assert a[0].shape == (N, 3) and a[1].shape == (N, 3) and a[2].shape == (N, 3) and a[3].shape == (N,) and a[4].shape == (N,)
    fd.check_corruption(pos, dy, batch, a, ratio)
    assert (a[2] != 0).any(dim=1).all(), "noise_vec is filled on every row, masked or not"
    _, _, _, noise_mask, dpm = a
    if prob == 1.0:
        assert dpm.all()
    if prob == 0.0:
        assert not dpm.any() and not noise_mask.any()
    if prob == 1.0 and ratio in (None, 1.0):
        assert noise_mask.all()
    if ratio == 0.0:
        assert not noise_mask.any()


# ---------------------------------------------------------------------------------------------- 2. corruption, statistical
def test_corruption_statistics():
    B, A, prob, ratio, std = 4096, 16, 0.25, 0.5, 0.1
    g = torch.Generator().manual_seed(0)
    pos, dy = torch.randn(B * A, 3, generator=g), torch.randn(B * A, 3, generator=g)
    batch = torch.repeat_interleave(torch.arange(B), A)
    _, _, noise_vec, noise_mask, dpm = _corrupt(pos, dy, batch, std, prob, ratio, seed=20240607)
    mol = dpm.view(B, A)[:, 0]
    share_mol = mol.double().mean().item()
    bound = 5 * math.sqrt(prob * (1 - prob) / B)
    print("selected molecules %.4f (0.25 +- %.4f)" % (share_mol, bound))
    assert abs(share_mol - prob) <= bound
    n_sel = int(dpm.sum())
    share_atom = noise_mask[dpm].double().mean().item()
    bound = 5 * math.sqrt(ratio * (1 - ratio) / n_sel)
    print("corrupted atoms of selected molecules %.4f (0.5 +- %.4f), n = %d" % (share_atom, bound, n_sel))
    assert abs(share_atom - ratio) <= bound
    x = noise_vec.double().flatten()
    n = x.numel()
    mean, s = x.mean().item(), x.std().item()
    print("noise mean %.3e (+- %.3e), std / 0.1 - 1 = %.3e (+- %.3e)" % (mean, 5 * std / math.sqrt(n), s / std - 1, 5 / math.sqrt(2 * n)))
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
MEAN, STD, NSTD = 5.0, 1.7, 0.05


def _loss_inputs(N, nB, mask, phantom, seed):
    g = torch.Generator().manual_seed(seed)
    d = dict(pred_y=torch.randn(nB, 1, generator=g), pred_dy=torch.randn(N, 3, generator=g),
             y=torch.randn(nB, generator=g) * 3 + 5, dy=torch.randn(N, 3, generator=g) * 2,
             noise_vec=torch.randn(N, 3, generator=g) * 0.05)
    d["noise_mask"] = {"mixed": torch.rand(N, generator=g) < 0.4, "all": torch.ones(N, dtype=torch.bool),
                       "none": torch.zeros(N, dtype=torch.bool)}[mask]
    d["row_mask"] = None
    if phantom and N > 1:
        k = max(1, N // 8)
        d["row_mask"] = torch.ones(N)
        d["row_mask"][-k:] = 0.0
        d["pred_dy"][-k:] = 3.0e37  # large finite garbage on the phantom rows
    if N > 1:  # one real row whose difference is exactly zero in fp64: dy = 0 = pred, or noise_vec = 0 = pred
        d["pred_dy"][0] = 0.0
        d["dy"][0] = 0.0
        d["noise_vec"][0] = 0.0
    return d


def _close(got, want, what, tol=1e-6):
    got, want = got.detach().double().cpu(), want.detach().double()
    err = (got - want).abs().max().item()
    assert err <= tol * want.abs().max().item(), (what, err, want.abs().max().item())


@pytest.mark.usefixtures("poisoned_ops")
@pytest.mark.parametrize("phantom", [False, True])
@pytest.mark.parametrize("mask", ["mixed", "all", "none"])
@pytest.mark.parametrize("nB", [1, 3])
@pytest.mark.parametrize("N", [1, 64, 65, 256, 257, 1025])
def test_loss_forward_backward_against_fp64(N, nB, mask, phantom):
    from equiformer_amd.dens import DeNSLoss
    d = _loss_inputs(N, nB, mask, phantom, seed=7 * N + nB)
    up = 0.37  # upstream gradient
    L = DeNSLoss(MEAN, STD, NSTD, 1.0, 80.0, 0.3)
    w32 = [float(torch.tensor(w, dtype=torch.float32)) for w in (1.0, 80.0, 0.3)]  # the device words are fp32

    def run(weights):
        py, pdy = d["pred_y"].double().requires_grad_(True), d["pred_dy"].double().requires_grad_(True)
        rm = None if d["row_mask"] is None else d["row_mask"] > 0
        loss, stats = fd.dens_loss(py, pdy, d["y"], d["dy"], d["noise_vec"], d["noise_mask"], weights, MEAN, STD, NSTD, row_mask=rm)
        gy, gdy = torch.autograd.grad(loss * up, [py, pdy])
        if rm is not None:  # rows the restatement dropped: zero gradient
            assert gdy[~rm].abs().sum() == 0
        return loss.detach(), stats, gy, gdy

    def run_gpu():
        py, pdy = d["pred_y"].to(DEV).requires_grad_(True), d["pred_dy"].to(DEV).requires_grad_(True)
        data = SimpleNamespace(y=d["y"].to(DEV), dy=d["dy"].to(DEV), noise_vec=d["noise_vec"].to(DEV),
                               noise_mask=d["noise_mask"].to(DEV))
        loss = L(py, pdy, data, row_mask=None if d["row_mask"] is None else d["row_mask"].to(DEV))
        assert loss.dim() == 0 and loss.dtype == torch.float32
        stats = L.stats.clone()
        (loss * up).backward()
        return loss.detach(), stats, py.grad, pdy.grad

    want = run(w32)
    got = run_gpu()
    again = run_gpu()
    for a, b in zip(got, again):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), "two calls differ"
    loss, stats, gy, gdy = got
    assert torch.isfinite(loss) and torch.isfinite(stats).all() and torch.isfinite(gy).all() and torch.isfinite(gdy).all()
    _close(loss, want[0], "loss")
    for i, name in enumerate(fd.STATS):
        _close(stats[i], want[1][i], name)
    assert stats[3].item() == want[1][3].item() and stats[4].item() == want[1][4].item()
    if mask == "all":
        assert stats[3].item() == 0 and stats[1].item() == 0 and stats[6].item() == 0
    if mask == "none":
        assert stats[4].item() == 0 and stats[2].item() == 0 and stats[7].item() == 0
    _close(gy, want[2], "d_pred_y")
    _close(gdy, want[3], "d_pred_dy")
    if d["row_mask"] is not None:
        assert gdy[d["row_mask"].to(DEV) == 0].abs().sum().item() == 0, "phantom rows must get exact zeros"
    if N > 1:
        assert gdy[0].abs().sum().item() == 0, "zero difference: the subgradient is 0, not NaN"
    # other device weights, nothing rebuilt
    L.set_weights(2.0, 40.0, 0.5)
    want2 = run([2.0, 40.0, 0.5])
    got2 = run_gpu()
    _close(got2[0], want2[0], "loss after set_weights")
    _close(got2[3], want2[3], "d_pred_dy after set_weights")
    L.set_weights(denoising_pos_weight=0.0)
    want3 = run([2.0, 40.0, 0.0])
    _close(run_gpu()[0], want3[0], "loss after a partial set_weights")


# ------------------------------------------------------------------------------------------------------ 4. no hidden syncs
def test_no_host_synchronisation():
    from equiformer_amd.dens import DeNSLoss, add_masked_gaussian_noise_to_pos
    pos, dy, batch = _corrupt_inputs(65, seed=3)
    data = SimpleNamespace(pos=pos.to(DEV), dy=dy.to(DEV), batch=batch.to(DEV), y=torch.randn(5).to(DEV))
    py = torch.randn(5, 1).to(DEV).requires_grad_(True)
    pdy = torch.randn(65, 3).to(DEV).requires_grad_(True)
    row_mask = torch.ones(65, device=DEV)
    L = DeNSLoss(MEAN, STD, NSTD, 1.0, 80.0, 10.0)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        add_masked_gaussian_noise_to_pos(data, 0.05, 0.5, 0.5, seed=11)
        L.set_weights(1.0, 80.0, 5.0)
        loss = L(py, pdy, data, row_mask=row_mask)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and torch.isfinite(pdy.grad).all() and L.stats[3].item() + L.stats[4].item() == 65


# -------------------------------------------------------------------------------------------------------- 5. model level
def _dens_kw(encode=True):
    import make_golden as mg
    base = mg.SMALL_L2
    emb = base["irreps_node_embedding"]
    feature = "+".join("%dx%de" % (2 * m, l) for l, m in enumerate(int(t.split("x")[0]) for t in emb.split("+")))
    return dict(base, number_of_basis=32, irreps_feature=feature, irreps_pre_attn=emb, use_force_encoding=encode,
                irreps_equivariant_inputs="+".join("1x%de" % l for l in range(len(emb.split("+")))))


_REF = []  # the fp64 oracle model, built once (nothing trains it: its gradients come from autograd.grad)


def _models():
    from oracle import nets as onets
    from weights import fill_deterministic
    from equiformer_amd.nets.equiformer_md17_dens import Equiformer_MD17_DeNS
    kw = _dens_kw()
    if not _REF:
        _REF.append(fill_deterministic(onets.Equiformer_MD17_DeNS(**kw), 41).double().train())
    ref = _REF[0]
    mod = Equiformer_MD17_DeNS(**kw)
    mod.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return ref, mod.to(DEV).train()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def test_model_with_fused_loss_against_fp64_oracle():
    from equiformer_amd.dens import DeNSLoss, add_masked_gaussian_noise_to_pos
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.synthetic import md17_aspirin_batch
    ref, mod = _models()
    d = md17_aspirin_batch(2, seed=3)
    data = SimpleNamespace(z=d["z"].to(DEV), pos=d["pos"].to(DEV), batch=d["batch"].to(DEV), y=d["y"].to(DEV), dy=d["dy"].to(DEV))
    add_masked_gaussian_noise_to_pos(data, 0.05, 1.0, 0.5, seed=5)
    n_d = int(data.noise_mask.sum())
    assert 0 < n_d < 42
    weights = (1.0, 80.0, 10.0)
    L = DeNSLoss(0.3, 1.7, 0.05, *weights)
    g = EdgeGraph.from_radius(data.pos, data.batch, R, num_graphs=2)
    E, Y = mod(data, graph=g)
    E0, Y0 = mod(data)  # graph=None: the model's own radius graph, the same kernels on the same edges
    assert _rel(E0, E) < 1e-5 and _rel(Y0, Y) < 1e-5
    loss = L(E, Y, data)
    gg = torch.autograd.grad(loss, list(mod.parameters()), allow_unused=True)
    dr = SimpleNamespace(z=d["z"], pos=data.pos.detach().double().cpu(), batch=d["batch"], force=data.force.double().cpu(),
                         noise_mask=data.noise_mask.cpu())
    Er, Yr = ref(dr)
    loss_r, stats_r = fd.dens_loss(Er, Yr, d["y"], d["dy"], data.noise_vec.cpu(), data.noise_mask.cpu(), weights, 0.3, 1.7, 0.05)
    gr = torch.autograd.grad(loss_r, list(ref.parameters()), allow_unused=True)
    print("E rel %.2e, dy rel %.2e, loss rel %.2e" % (_rel(E, Er), _rel(Y, Yr), _rel(loss, loss_r)))
    assert _rel(E, Er) < 1e-4 and _rel(Y, Yr) < 1e-4 and _rel(loss, loss_r) < 1e-4
    assert L.stats[3].item() == stats_r[3].item() and L.stats[4].item() == stats_r[4].item() == n_d
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
def test_captured_step_equals_eager_loop():
    """Two aspirin frames, 42 atoms: at most 42 * 20 = 840 directed edges, so edge_step = 1024 puts every corrupted batch in one
    bucket.  3 eager padded steps, one capture, 5 replays against 8 eager unpadded steps with the same seeds."""
    from equiformer_amd.capture import bucket_of
    from equiformer_amd.dens import DeNSLoss, DeNSTrainStep, add_masked_gaussian_noise_to_pos, step_seed
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW
    from equiformer_amd.synthetic import md17_aspirin_batch
    d = md17_aspirin_batch(2, seed=3)
    batch = {k: d[k].to(DEV) for k in ("pos", "z", "batch", "y", "dy")}
    batch["num_graphs"] = 2
    std, prob, ratio, seed = 0.05, 0.75, 0.5, 99
    assert bucket_of(2, 42, 1, 64, 1024) == bucket_of(2, 42, 840, 64, 1024)
    results = []
    for captured in (False, True):
        _, m = _models()
        opt = FlatAdamW(m.parameters(), lr=5e-4, weight_decay=1e-6)
        L = DeNSLoss(0.3, 1.7, std, 1.0, 80.0, 10.0)
        ts = DeNSTrainStep(m, opt, L, R, std, prob, ratio, seed=seed, min_eager=3, edge_step=1024) if captured else None
        losses, stats, masks, edges = [], [], [], []
        for k in range(8):
            if k == 6:  # between two replays: the decayed denoising weight
                L.set_weights(denoising_pos_weight=4.0)
            if captured:
                loss = ts.step(batch)
                masks.append(ts.last["noise_mask"].cpu())
            else:
                data = SimpleNamespace(**{n: batch[n] for n in ("pos", "z", "batch", "y", "dy")})
                add_masked_gaussian_noise_to_pos(data, std, prob, ratio, seed=step_seed(seed, k))
                opt.zero_grad(set_to_none=True)
                g = EdgeGraph.from_radius(data.pos, data.batch, R, num_graphs=2)
                edges.append(g.E)
                E, Y = m(data, graph=g)
                loss = L(E, Y, data)
                loss.backward()
                opt.step()
                loss = loss.detach()
                masks.append(data.noise_mask.cpu())
            losses.append(float(loss))
            stats.append(L.stats.cpu())
        torch.cuda.synchronize()
        if captured:
            assert (ts.eager_steps, ts.captures, ts.replays) == (3, 1, 5), (ts.eager_steps, ts.captures, ts.replays)
        results.append((losses, stats, masks, opt.flat_m.detach().clone(), edges))
    (le, se, ke, me, edges), (lg, sg, kg, mg_, _) = results
    print("edges per step", edges)
    print("dens captured vs eager: losses %.3e, moments %.3e"
          % (max(abs(a - b) / max(1.0, abs(a)) for a, b in zip(le, lg)), _rel(mg_, me)))
    assert torch.equal(batch["pos"].cpu(), d["pos"]), "the step must not move the caller's atoms"
    for k in range(8):
        assert torch.equal(ke[k], kg[k]), "step %d corrupted other atoms" % k
        assert se[k][3].item() == sg[k][3].item() and se[k][4].item() == sg[k][4].item(), (k, se[k], sg[k])
        assert sg[k][3].item() + sg[k][4].item() == 42 and sg[k][4].item() == int(kg[k].sum())
        assert abs(le[k] - lg[k]) <= 1e-4 * max(1.0, abs(le[k])), (le, lg)
        # the loss a replay returns is made of the device weights of that moment
        w_d = 10.0 if k < 6 else 4.0
        made = 1.0 * sg[k][0].item() + 80.0 * sg[k][1].item() + w_d * sg[k][2].item()
        assert abs(made - lg[k]) <= 1e-5 * max(1.0, abs(lg[k])), (k, made, lg[k])
    assert sg[6][2].item() > 0, "the reweighted step needs corrupted atoms"
    assert any(not torch.equal(kg[i], kg[j]) for i in range(3, 8) for j in range(i + 1, 8)), "the replays saw one mask"
    assert _rel(mg_, me) < 2e-3, _rel(mg_, me)
