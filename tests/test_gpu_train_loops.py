"""The training loops of equiformer_amd/train.py on the GPU: each against an eager, unpadded loop whose loss is written in ATen
(the reference's loop body), from the same initial weights.

  * QM9 (SMALL_L2, alpha_drop 0): train_one_epoch_qm9 over 6 batches of 4 to 6 molecules (min_eager 2) -- loss trajectory,
    AdamW moments and parameters at the tolerances of `_assert_trains_as_eager` of tests/test_gpu_bucketed_capture.py, and its
    MAE against the one the eager loop's own predictions give.
  * MD17 (nonlinear_exp_l2_md17, two-frame aspirin batches): train_one_epoch_md17 with energy weight 1, force weight 80 and
    the L2MAE criterion, at the tolerances of test_captured_md17_force_loss_step_equals_eager; all four averages.
  * OC20 (periodic slab batches, energy head): train_one_epoch_oc20 with a cosine lr_lambda, searched and given edges: the lr
    written before step k is lr_initial * lr_lambda_cosine(k), and two replays at lr 0 leave the parameters unchanged.
  * A model with the auxiliary IS2RS head is refused.
Measured on an MI355X: QM9 losses 2.7e-6, moments 1.7e-6, parameters above noise 1.0e-7, MAE 1.3e-6 apart; MD17 averages
at most 3.2e-5 (4.7e-6 relative) from the eager loop's."""
import functools
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import periodic_inputs as pi  # noqa: E402

DEV = torch.device("cuda:0")
R = 5.0


def _rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _dev(d):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}


def _recording(ts):
    """per-step losses (and the lr each step saw) of a train step, read back by the test, not by the loop"""
    rec = dict(losses=[], lr=[])
    step = ts.step

    def recorded(batch):
        rec["lr"].append(ts.optimizer.param_groups[0]["lr"])
        loss = step(batch)
        rec["losses"].append(float(loss))
        return loss
    ts.step = recorded
    return rec


# ------------------------------------------------------------------------------------------------------------------------ QM9
QM9_NORM = (0.3, 1.7)


def _qm9_model():
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    m = GraphAttentionTransformer(irreps_in="5x0e", max_radius=R, number_of_basis=32, **dict(mg.SMALL_L2, alpha_drop=0.0))
    return fill_deterministic(m, 21).to(DEV).train()


def _qm9_batches():
    """6 batches, every one of other atom counts: 5, 4, 5, 6, 5, 5 molecules of 9-15 atoms (the four of 5 molecules share the
    default bucket, so with min_eager 2 the step captures and replays)"""
    from equiformer_amd.synthetic import qm9_like_varying_batches
    five = qm9_like_varying_batches(4, 5, (9, 15), side=5.5, seed=5)
    four, six = (qm9_like_varying_batches(1, B, (9, 15), side=5.5, seed=B)[0] for B in (4, 6))
    return [_dev(d) for d in (five[0], four, five[1], six, five[2], five[3])]


def test_qm9_loop_trains_as_the_eager_loop():
    from equiformer_amd import train
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW
    batches, lr = _qm9_batches(), 5e-4
    mean, std = QM9_NORM
    # eager, unpadded, ATen loss (engine.py:71 with L1Loss)
    m = _qm9_model()
    opt = FlatAdamW(m.parameters(), lr=lr, weight_decay=1e-2)
    e = dict(losses=[])
    abs_err = n = 0.0
    for d in batches:
        opt.zero_grad(set_to_none=True)
        g = EdgeGraph.from_radius(d["pos"], d["batch"], R, num_graphs=d["num_graphs"])
        pred = m(None, d["pos"], d["batch"], d["z"], graph=g).squeeze(-1)
        loss = (pred - (d["y"] - mean) / std).abs().mean()
        loss.backward()
        opt.step()
        e["losses"].append(float(loss))
        abs_err += float((pred.detach().double() * std + mean - d["y"].double()).abs().sum())
        n += d["num_graphs"]
    torch.cuda.synchronize()
    e.update(p=opt.flat_p.detach().clone(), m=opt.flat_m.detach().clone(), step=opt._step)
    mae_eager = abs_err / n
    # the loop
    m = _qm9_model()
    opt = FlatAdamW(m.parameters(), lr=lr, weight_decay=1e-2)
    ts = train.qm9_train_step(m, opt, QM9_NORM, R, min_eager=2)
    rec = _recording(ts)
    mae = train.train_one_epoch_qm9(ts, batches, target=None)
    torch.cuda.synchronize()
    assert ts.replays > 0 and ts.replays + ts.eager_steps == 6, (ts.replays, ts.eager_steps)
    b = dict(losses=rec["losses"], p=opt.flat_p.detach().clone(), m=opt.flat_m.detach().clone(), step=opt._step)
    _assert_trains_as_eager(e, b, 6, lr)
    # mae = std * (mean |d|) per batch: the trajectory's tolerance (2e-5 of max(1, loss)) carried through that identity
    bound = 2e-5 * std * max(1.0, max(e["losses"]))
    print("QM9 MAE: loop %.9f, eager predictions %.9f, bound %.2e" % (mae, mae_eager, bound))
    assert abs(mae - mae_eager) <= bound


def _assert_trains_as_eager(e, b, steps, max_lr):
    """the assertions of tests/test_gpu_bucketed_capture.py `_assert_trains_as_eager`, restated"""
    assert e["step"] == b["step"] == steps
    worst = max(abs(x - y) / max(1.0, abs(x)) for x, y in zip(e["losses"], b["losses"]))
    big = e["m"].abs() > 1e-3 * e["m"].abs().max()
    print("loop vs eager over %d steps: losses %.3e, moments %.3e, parameters above noise %.3e, all parameters %.3e"
          % (steps, worst, _rel(b["m"], e["m"]), _rel(b["p"][big], e["p"][big]), _rel(b["p"], e["p"])))
    for x, y in zip(e["losses"], b["losses"]):
        assert abs(x - y) <= 2e-5 * max(1.0, abs(x)), (e["losses"], b["losses"])
    assert _rel(b["m"], e["m"]) < 5e-4, _rel(b["m"], e["m"])
    assert int(big.sum()) > 1000
    assert _rel(b["p"][big], e["p"][big]) < 1e-4, _rel(b["p"][big], e["p"][big])
    assert _rel(b["p"], e["p"]) < steps * 2 * max_lr


# ----------------------------------------------------------------------------------------------------------------------- MD17
def _md17_model():
    from equiformer_amd import nets
    torch.manual_seed(0)
    m = nets.model_entrypoint("graph_attention_transformer_nonlinear_exp_l2_md17")(irreps_in="64x0e", radius=5.0, num_basis=32)
    return m.to(DEV).train()


def test_md17_loop_trains_as_the_eager_loop():
    from equiformer_amd import train
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW
    from equiformer_amd.synthetic import md17_aspirin_batch
    batches = [_dev(dict(md17_aspirin_batch(2, seed=3 + i % 2), num_graphs=2)) for i in range(7)]
    w_e, w_f = 1.0, 80.0
    m = _md17_model()
    mean, std = float(m.task_mean or 0.0), float(m.task_std or 1.0)
    opt = FlatAdamW(m.parameters(), lr=5e-4, weight_decay=1e-6)
    losses_e = []
    acc = dict(loss_e=0.0, loss_f=0.0, mae_e=0.0, mae_f=0.0, B=0, N=0)
    for d in batches:  # main_md17.py:382-400, unpadded
        opt.zero_grad(set_to_none=True)
        g = EdgeGraph.from_radius(d["pos"], d["batch"], 5.0, num_graphs=2)
        pred_y, pred_dy = m(node_atom=d["z"], pos=d["pos"], batch=d["batch"], graph=g)
        loss_e = (pred_y - (d["y"].view(-1, 1) - mean) / std).abs().mean()
        loss_f = (pred_dy - d["dy"] / std).norm(dim=1).mean()
        loss = w_e * loss_e + w_f * loss_f
        loss.backward()
        opt.step()
        losses_e.append(float(loss))
        B, N = pred_y.shape[0], pred_dy.shape[0]
        acc["loss_e"] += float(loss_e) * B
        acc["loss_f"] += float(loss_f) * N
        acc["mae_e"] += float((pred_y.detach() * std + mean - d["y"].view(-1, 1)).abs().mean()) * B
        acc["mae_f"] += float((pred_dy.detach() * std - d["dy"]).abs().mean()) * N
        acc["B"] += B
        acc["N"] += N
    torch.cuda.synchronize()
    me = opt.flat_m.detach().clone()
    m = _md17_model()
    opt = FlatAdamW(m.parameters(), lr=5e-4, weight_decay=1e-6)
    ts = train.md17_train_step(m, opt, 5.0, w_e, w_f, criterion="l2mae", task_mean=mean, task_std=std, min_eager=3)
    rec = _recording(ts)
    mae_metrics, loss_metrics = train.train_one_epoch_md17(ts, batches)
    torch.cuda.synchronize()
    assert ts.replays >= 1 and ts.replays + ts.eager_steps == 7, (ts.replays, ts.eager_steps)
    for a, b in zip(losses_e, rec["losses"]):
        assert abs(a - b) <= 1e-4 * max(1.0, abs(a)), (losses_e, rec["losses"])
    assert _rel(opt.flat_m, me) < 2e-3, _rel(opt.flat_m, me)
    # the four averages: means of the same steps' predictions, at the per-step loss tolerance
    want = {("loss", "energy"): acc["loss_e"] / acc["B"], ("loss", "force"): acc["loss_f"] / acc["N"],
            ("mae", "energy"): acc["mae_e"] / acc["B"], ("mae", "force"): acc["mae_f"] / acc["N"]}
    got = {("loss", k): loss_metrics[k].avg for k in ("energy", "force")}
    got.update({("mae", k): mae_metrics[k].avg for k in ("energy", "force")})
    for key in want:
        print("MD17 %s %s: loop %.9f, eager %.9f" % (key + (got[key], want[key])))
        assert abs(got[key] - want[key]) <= 1e-4 * max(1.0, abs(want[key])), key
    assert loss_metrics["energy"].count == 14 and loss_metrics["force"].count == 7 * 42


# ----------------------------------------------------------------------------------------------------------------------- OC20
def _oc20_model(head=None):
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20
    cfg = dict(mg.SMALL_OC20, number_of_basis=32, otf_graph=True, use_pbc=True, max_neighbors=pi.SLAB_CAP, **(head or {}))
    m = GraphAttentionTransformerOC20(None, None, 1, **cfg)
    return fill_deterministic(m, 21).to(DEV).train()


@pytest.mark.parametrize("edges", ["search", "batch"])
def test_oc20_loop_writes_the_scheduled_lr_and_the_replay_sees_it(edges):
    from equiformer_amd import train
    from equiformer_amd.optim import FlatAdamW
    from equiformer_amd.synthetic import attach_given_edges
    raw = [_dev(d) for d in pi.slab_batches(2)]
    batches = [attach_given_edges(d, R, pi.SLAB_CAP) if edges == "batch" else d for d in raw]
    m = _oc20_model()
    opt = FlatAdamW(m.parameters(), lr=2e-4, weight_decay=1e-2)
    ts = train.oc20_train_step(m, opt, R, task_mean=0.1, task_std=2.0, max_num_neighbors=pi.SLAB_CAP, node_step=64,
                               edge_step=1024, min_eager=1, edges=edges)
    # warm-up over 1 step, cosine to 0 at step 4: steps 4 and 5 run at lr 0
    lam = functools.partial(train.lr_lambda_cosine, warmup=1, warmup_factor=0.2, total=4, lr_min_factor=0.0)
    rec = _recording(ts)
    params = []
    step = ts.step

    def keep(batch):
        out = step(batch)
        params.append((opt.flat_p.detach().clone(), ts.replays))
        return out
    ts.step = keep
    metrics, loss = train.train_one_epoch_oc20(ts, [batches[i % 2] for i in range(6)], lr_lambda=lam)
    torch.cuda.synchronize()
    want = [2e-4 * lam(k) for k in range(6)]
    print("lr written: %s" % rec["lr"])
    assert rec["lr"] == want and want[4] == want[5] == 0.0 and min(want[:4]) > 0
    assert params[4][1] == params[3][1] + 1 and params[5][1] == params[4][1] + 1, "steps 4 and 5 must be replays"
    assert torch.equal(params[5][0], params[3][0]), "two replays at lr 0 changed the parameters"
    assert not torch.equal(params[3][0], params[2][0]), "a replay at lr > 0 must move the parameters"
    n = sum(int(batches[i % 2]["num_graphs"]) for i in range(6))
    assert metrics["energy_mae"]["numel"] == n and all(v["metric"] == v["metric"] for v in metrics.values())
    assert loss == loss and loss > 0 and abs(metrics["energy_mae"]["metric"] - 2.0 * loss) <= 1e-9 * abs(loss)


def test_oc20_step_refuses_the_auxiliary_head():
    from equiformer_amd import train
    from equiformer_amd.optim import FlatAdamW
    m = _oc20_model(dict(use_auxiliary_task=True))
    opt = FlatAdamW(m.parameters(), lr=1e-4)
    with pytest.raises(ValueError, match="IS2RSTrainStep"):
        train.oc20_train_step(m, opt, R, max_num_neighbors=pi.SLAB_CAP)
