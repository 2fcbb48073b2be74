"""The captured evaluation step (equiformer_amd/evaluate.py BucketedEvalStep, Meter and the three drivers) on the GPU: padded,
bucketed and replayed evaluation returns the real rows the eager, unpadded model gives (1e-4 relative: the bar of
tests/test_gpu_bucketed_capture.py for padded against unpadded runs), most steps are replays, the drivers report what the
reference-style loops report on the eager predictions, and a replay sees parameters that were modified in place.
Two-layer SMALL_* models with deterministic weights; buckets of 16 nodes / 128 edges."""
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
import periodic_inputs as pi  # noqa: E402

R = 5.0
STEPS = dict(node_step=16, edge_step=128)
MEAN, STD, THR = 0.3, 1.7, 1.0
DEV = torch.device("cuda:0")


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _close(a, b, tol=1e-4):
    return abs(a - b) <= tol * abs(b)


def _dev(d):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}


def _perturb(model):
    """an optimizer step's worth of in-place change, large enough to show at the 1e-4 bar"""
    with torch.no_grad():
        for i, p in enumerate(model.parameters()):
            p.mul_(0.9 if i % 2 else 1.1)


def _expected_counters(keys, min_eager=1):
    count = collections.Counter(keys)
    return (sum(min(c, min_eager) for c in count.values()), sum(1 for c in count.values() if c > min_eager),
            sum(max(0, c - min_eager) for c in count.values()))


def _key(d, periodic=False, cap=1000):
    from equiformer_amd.capture import bucket_of
    from equiformer_amd.graph import EdgeGraph
    if periodic:
        plan = EdgeGraph.radius_pbc_plan(d["pos"], d["cell"], d["batch"], R, cap, d["num_graphs"])
    else:
        plan = EdgeGraph.radius_plan(d["pos"], d["batch"], R, cap, d["num_graphs"])
    return bucket_of(d["num_graphs"], plan.N, plan.E, 16, 128)


class AverageMeter:
    """the reference's: a running average of per-batch means weighted by n (fp64 on the host)"""

    def __init__(self):
        self.sum, self.count, self.avg = 0.0, 0, 0.0

    def update(self, val, n=1):
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


# ------------------------------------------------------------------------------------------------------------------ QM9: forward only
def _qm9_model(seed=21):
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    m = GraphAttentionTransformer(irreps_in="5x0e", max_radius=R, number_of_basis=32, **mg.SMALL_L2)
    return fill_deterministic(m, seed).to(DEV).eval()


def _qm9_batches(n=12):
    from equiformer_amd.synthetic import qm9_like_varying_batches
    return [_dev(d) for d in qm9_like_varying_batches(n, 6, (9, 15), side=5.5, seed=0)]


def _qm9_eager(m, batches):
    from equiformer_amd.graph import EdgeGraph
    out = []
    with torch.no_grad():
        for d in batches:
            g = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=d["num_graphs"])
            out.append(m(None, d["pos"], d["batch"], d["z"], graph=g).squeeze(-1).clone())
    return out


def _qm9_reference_loop(preds, batches):
    """engine.evaluate's meters (engine.py:136-141) on the eager predictions, in fp64"""
    loss_m, mae_m = AverageMeter(), AverageMeter()
    for p, d in zip(preds, batches):
        p, y = p.double().cpu(), d["y"].double().cpu()
        loss_m.update(torch.nn.functional.l1_loss(p, (y - MEAN) / STD).item(), n=p.shape[0])
        mae_m.update(torch.mean(torch.abs(p * STD + MEAN - y)).item(), n=p.shape[0])
    return mae_m.avg, loss_m.avg, mae_m.count


def test_qm9_eval_step_returns_the_eager_rows_replays_and_sees_new_weights():
    from equiformer_amd.evaluate import evaluate_qm9, qm9_eval_step
    m = _qm9_model()
    batches = _qm9_batches()
    keys = [_key(d) for d in batches]
    assert len(set(keys)) >= 2 and len({d["pos"].shape[0] for d in batches}) > 3, keys
    eager = _qm9_eager(m, batches)
    es = qm9_eval_step(m, (MEAN, STD), R, threshold=THR, min_eager=1, **STEPS)
    worst = 0.0
    for d, e0 in zip(batches, eager):
        e, f = es.step(d)
        assert f is None and e.shape[0] == 6 and not e.requires_grad
        worst = max(worst, _rel(e.squeeze(-1), e0))
        assert _rel(e.squeeze(-1), e0) < 1e-4
    want = _expected_counters(keys)
    assert (es.eager_steps, es.captures, es.replays, es.evictions) == want + (0,), (es.eager_steps, es.captures, es.replays)
    assert 2 * es.replays >= len(batches) and sorted(es.live_graphs()) == sorted(k for k in set(keys) if keys.count(k) > 1)
    # the meter has seen every batch once, eager steps and replays alike (capturing itself enqueues nothing)
    sums = es.meter.read()
    assert sums["graphs"] == 6.0 * len(batches) and sums["atoms"] == 0.0
    # the driver against the reference-style loop on the eager predictions
    mae0, loss0, n0 = _qm9_reference_loop(eager, batches)
    mae, loss = evaluate_qm9(m, (MEAN, STD), 0, batches, R, step=es)
    assert es.meter.read()["graphs"] == n0 == 72
    assert _close(mae, mae0) and _close(loss, loss0), (mae, mae0, loss, loss0)
    assert es.eager_steps == want[0]  # the second pass: replays only (buckets seen once stay eager until seen again)
    print("qm9: worst rel err of a replayed row %.3e; mae %.6f vs %.6f, loss %.6f vs %.6f" % (worst, mae, mae0, loss, loss0))
    # [B, T] targets: column `target`
    two = [dict(d, y=torch.stack([d["y"] + 3.0, d["y"]], dim=1)) for d in batches]
    mae2, loss2 = evaluate_qm9(m, (MEAN, STD), 1, two, R, step=es)
    assert _close(mae2, mae, 1e-5) and _close(loss2, loss, 1e-5)
    # parameters modified in place between two passes: the replays compute with the new values
    _perturb(m)
    eager_new = _qm9_eager(m, batches)
    assert max(_rel(a, b) for a, b in zip(eager_new, eager)) > 1e-2
    before = es.replays
    for d, e0 in zip(batches, eager_new):
        e, _ = es.step(d)
        assert _rel(e.squeeze(-1), e0) < 1e-4
    assert es.replays - before == len(batches)  # (every bucket had its graph by now: nothing ran eagerly)


def test_a_model_in_training_mode_is_refused_and_max_graphs_evicts():
    from equiformer_amd.evaluate import qm9_eval_step
    m = _qm9_model()
    batches = _qm9_batches()
    keys = [_key(d) for d in batches]
    picked = {}
    for d, k in zip(batches, keys):
        picked.setdefault(k, d)
    a, b = list(picked.values())[:2]
    es = qm9_eval_step(m, (MEAN, STD), R, min_eager=1, max_graphs=1, **STEPS)
    m.train()
    with pytest.raises(ValueError, match="training mode"):
        es.step(a)
    m.eval()
    assert es.eager_steps == es.replays == 0
    ea, eb = _qm9_eager(m, [a, b])
    live = []
    for it in range(8):
        d, e0 = ((a, ea), (b, eb))[it % 2]
        e, _ = es.step(d)
        assert _rel(e.squeeze(-1), e0) < 1e-4, it
        live.append(len(es.live_graphs()))
    assert max(live) == 1 and es.evictions > 0 and es.replays >= 2 and es.replays + es.eager_steps == 8
    assert es.meter.read()["graphs"] == 48.0


# ------------------------------------------------------------------------------------------------------------------ MD17: force pass
def _md17_model(seed=12):
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer_md17 import GraphAttentionTransformerMD17
    m = GraphAttentionTransformerMD17(irreps_in="64x0e", max_radius=R, number_of_basis=32, basis_type="exp", mean=MEAN, std=STD,
                                      **mg.SMALL_L2)
    return fill_deterministic(m, seed).to(DEV).eval()


def _md17_batches():
    """aspirin frames with jitter in batches of 2 and 3 frames: y [B, 1] and dy [N, 3] as targets"""
    from equiformer_amd.synthetic import md17_aspirin_batch
    full = md17_aspirin_batch(20, jitter=0.05, seed=0)
    out, first = [], 0
    for frames in (2, 3, 2, 3, 2, 3, 2, 3):
        sel = (full["batch"] >= first) & (full["batch"] < first + frames)
        out.append(_dev(dict(pos=full["pos"][sel], z=full["z"][sel], batch=full["batch"][sel] - first, num_graphs=frames,
                             y=full["y"][first:first + frames].view(-1, 1), dy=full["dy"][sel])))
        first += frames
    return out


def _md17_eager(m, batches):
    from equiformer_amd.graph import EdgeGraph
    out = []
    for d in batches:
        g = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=d["num_graphs"])
        E, F = m(node_atom=d["z"], pos=d["pos"], batch=d["batch"], graph=g)
        out.append((E.detach().clone(), F.detach().clone()))
    return out


def _md17_reference_loop(preds, batches):
    """main_md17.evaluate's four meters (main_md17.py:451-462, criterion L2MAELoss) on the eager predictions, in fp64"""
    def l2mae(a, b):
        return torch.mean(torch.norm(a - b, p=2, dim=-1))
    lm = {"energy": AverageMeter(), "force": AverageMeter()}
    mm = {"energy": AverageMeter(), "force": AverageMeter()}
    for (py, pdy), d in zip(preds, batches):
        py, pdy, y, dy = py.double().cpu(), pdy.double().cpu(), d["y"].double().cpu(), d["dy"].double().cpu()
        lm["energy"].update(l2mae(py, (y - MEAN) / STD).item(), n=py.shape[0])
        lm["force"].update(l2mae(pdy, dy / STD).item(), n=pdy.shape[0])
        mm["energy"].update(torch.mean(torch.abs(py * STD + MEAN - y)).item(), n=py.shape[0])
        mm["force"].update(torch.mean(torch.abs(pdy * STD - dy)).item(), n=pdy.shape[0])
    return mm, lm


def test_md17_eval_step_captures_the_first_order_force_pass():
    from equiformer_amd.evaluate import evaluate_md17, md17_eval_step
    m = _md17_model()
    batches = _md17_batches()
    keys = [_key(d) for d in batches]
    assert len(set(keys)) >= 2
    eager = _md17_eager(m, batches)
    es = md17_eval_step(m, R, min_eager=1, **STEPS)
    assert (es.meter.task_mean, es.meter.task_std) == (MEAN, STD)
    worst_e = worst_f = 0.0
    for d, (e0, f0) in zip(batches, eager):
        e, f = es.step(d)
        assert e.shape == e0.shape and f.shape == f0.shape and not e.requires_grad and not f.requires_grad
        worst_e, worst_f = max(worst_e, _rel(e, e0)), max(worst_f, _rel(f, f0))
        assert _rel(e, e0) < 1e-4 and _rel(f, f0) < 1e-4, (_rel(e, e0), _rel(f, f0))
    want = _expected_counters(keys)
    assert (es.eager_steps, es.captures, es.replays, es.evictions) == want + (0,), (es.eager_steps, es.captures, es.replays)
    assert 2 * es.replays >= len(batches)
    sums = es.meter.read()
    assert sums["graphs"] == 20.0 and sums["atoms"] == 20.0 * 21
    mm, lm = _md17_reference_loop(eager, batches)
    mae_metrics, loss_metrics = evaluate_md17(m, batches, R, step=es)
    for k in ("energy", "force"):
        assert mae_metrics[k].count == mm[k].count and loss_metrics[k].count == lm[k].count
        assert _close(mae_metrics[k].avg, mm[k].avg), (k, mae_metrics[k].avg, mm[k].avg)
        assert _close(loss_metrics[k].avg, lm[k].avg), (k, loss_metrics[k].avg, lm[k].avg)
    print("md17: worst rel err energies %.3e, forces %.3e; e_mae %.6f vs %.6f, f_mae %.6f vs %.6f" % (
        worst_e, worst_f, mae_metrics["energy"].avg, mm["energy"].avg, mae_metrics["force"].avg, mm["force"].avg))
    # parameters modified in place: replays (no bucket is new) with the new weights
    _perturb(m)
    eager_new = _md17_eager(m, batches)
    assert max(_rel(a[1], b[1]) for a, b in zip(eager_new, eager)) > 1e-2
    before = es.replays
    for d, (e0, f0) in zip(batches, eager_new):
        e, f = es.step(d)
        assert _rel(e, e0) < 1e-4 and _rel(f, f0) < 1e-4, (_rel(e, e0), _rel(f, f0))
    assert es.replays - before == len(batches)
    m.train()
    with pytest.raises(ValueError, match="training mode"):
        es.step(batches[0])


# ------------------------------------------------------------------------------------------------------------------ OC20: periodic
def _oc20_model(seed=21):
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20
    cfg = dict(mg.SMALL_OC20, number_of_basis=32, otf_graph=True, use_pbc=True, max_neighbors=pi.SLAB_CAP)
    return fill_deterministic(GraphAttentionTransformerOC20(None, None, 1, **cfg), seed).to(DEV).eval()


def test_oc20_eval_step_on_periodic_slab_batches():
    from equiformer_amd.evaluate import evaluate_oc20, oc20_eval_step
    m = _oc20_model()
    batches = [_dev(d) for d in pi.slab_batches(4)]
    keys = [_key(d, periodic=True, cap=pi.SLAB_CAP) for d in batches]
    with torch.no_grad():
        eager = [m(SimpleNamespace(pos=d["pos"], batch=d["batch"], atomic_numbers=d["atomic_numbers"], tags=d["tags"],
                                   cell=d["cell"], natoms=d["natoms"])).squeeze(-1).clone() for d in batches]
    es = oc20_eval_step(m, R, task_mean=MEAN, task_std=STD, threshold=THR, min_eager=1, max_num_neighbors=pi.SLAB_CAP, **STEPS)
    # the reference's running totals on the eager predictions (denormalised), fp64
    tot, numel = {"energy_mae": 0.0, "energy_mse": 0.0, "energy_within_threshold": 0.0}, 0
    for p, d in zip(eager, batches):
        e = p.double().cpu() * STD + MEAN - d["y"].double().cpu()
        tot["energy_mae"] += e.abs().sum().item()
        tot["energy_mse"] += (e ** 2).sum().item()
        tot["energy_within_threshold"] += (e.abs() < THR).sum().item()
        numel += e.numel()
        assert float((e.abs() - THR).abs().min()) > 1e-3  # (no error so near the threshold that 1e-4 could move the count)
    for sweep in range(2):  # the first pass runs every bucket eagerly once; the second replays what the first saw
        for d, e0 in zip(batches, eager):
            e, f = es.step(d)
            assert f is None and _rel(e.squeeze(-1), e0) < 1e-4, (sweep, _rel(e.squeeze(-1), e0))
    want = _expected_counters(keys + keys)
    assert (es.eager_steps, es.captures, es.replays) == want and es.replays >= 4, (es.eager_steps, es.captures, es.replays)
    metrics = evaluate_oc20(m, batches, R, step=es)
    assert es.replays >= 8
    for k in tot:
        assert metrics[k]["numel"] == numel == 16
        assert _close(metrics[k]["total"], tot[k]) and _close(metrics[k]["metric"], tot[k] / numel), (k, metrics[k], tot[k])
    assert metrics["energy_within_threshold"]["total"] == tot["energy_within_threshold"]
    with pytest.raises(ValueError):  # one instance serves periodic or non-periodic batches, not both
        es.step({k: v for k, v in batches[0].items() if k != "cell"})


# ------------------------------------------------------------------------------------------------------------------ in a train loop
def test_meter_inside_a_bucketed_train_step_counts_the_real_steps():
    """Meter.update under no_grad inside forward_loss: the running MAE of the train loop without a read-back per step.  Learning
    rate 0 (the weights do not move), so the eager loop's MAE is that of the fixed weights on the same batches."""
    from equiformer_amd.capture import BucketedTrainStep
    from equiformer_amd.evaluate import Meter
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW
    m = _qm9_model().train()
    batches = _qm9_batches()
    keys = [_key(d) for d in batches]
    key = max(set(keys), key=keys.count)
    same = [d for d, k in zip(batches, keys) if k == key][:3]
    assert len(same) == 3
    opt = FlatAdamW(m.parameters(), lr=0.0, weight_decay=0.0)
    meter = Meter(MEAN, STD, THR, device=DEV)

    def forward_loss(g, v):
        pred = m(None, v.pos, v.batch, v.z, graph=g).squeeze(-1)
        with torch.no_grad():
            meter.update(pred, v.y, v.B)
        return (pred[:v.B] - (v.y[:v.B] - MEAN) / STD).abs().mean()

    bs = BucketedTrainStep(opt, forward_loss, R, min_eager=2, **STEPS)
    K = 7
    mae_m = AverageMeter()
    for it in range(K):
        d = same[it % 3]
        bs.step(d)
        with torch.no_grad():
            g = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=6)
            p = m(None, d["pos"], d["batch"], d["z"], graph=g).squeeze(-1).double().cpu()
        mae_m.update(torch.mean(torch.abs(p * STD + MEAN - d["y"].double().cpu())).item(), n=6)
    assert (bs.eager_steps, bs.captures, bs.replays) == (2, 1, K - 2)
    sums = meter.read()
    assert sums["graphs"] == float(K * 6)  # the capture itself enqueued nothing
    mae = Meter.figures(sums)["qm9"][0]
    assert _close(mae, mae_m.avg), (mae, mae_m.avg)
