"""train_one_epoch_is2rs (equiformer_amd/train.py) on the GPU, with the model and the slab batch of tests/test_gpu_is2rs_step.py
(4 structures, one bucket): 8 steps, min_eager 3 (3 eager steps, one capture, 5 replays), a cosine lr_lambda and the auxiliary
weight decaying from w0 = 15 over total_steps = 8.

  * before step k the loop wrote lr = lr_initial lr_lambda(k) and the auxiliary weight auxiliary_task_weight(15, k + 1, 8) (the
    reference's 1-based self.step); every step's loss is stats[0] + w stats[1] (energy weight 1) within 1e-5: the replays see
    the weight the loop wrote;
  * the averages equal a host AverageMeter fed the loop's own per-step figures (read back by the test) bit for bit;
  * they are within the trajectory bound of that file (2e-5 of max(1, |x|)) of an eager, unpadded loop with the same seeds,
    lr and weights."""
import functools
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import periodic_inputs as pi  # noqa: E402
import test_gpu_is2rs_step as t6  # noqa: E402  (the model, the slab batch, the normalisation, the bucket steps)

DEV = torch.device("cuda:0")
W0, LR, STEPS, SEED = 15.0, 5e-4, 8, 99
NAMES = ("loss", "energy_mae", "energy_mse", "energy_within_threshold", "pos_mae")


class AverageMeter:
    """engine.py:12-27"""

    def __init__(self):
        self.sum, self.count = 0, 0

    def update(self, val, n=1):
        self.sum += val * n
        self.count += n


def _lam():
    from equiformer_amd import train
    return functools.partial(train.lr_lambda_cosine, warmup=2, warmup_factor=0.2, total=STEPS, lr_min_factor=0.01)


def _host_meters(losses, stats_list):
    """energy_trainer_v2.py:275-288: one update per step of the loss and the evaluator's three metrics; pos_mae by the free atoms"""
    m = {n: AverageMeter() for n in NAMES}
    for loss, s in zip(losses, stats_list):
        s = s.tolist()
        m["loss"].update(loss)
        for n, i in (("energy_mae", 3), ("energy_mse", 4), ("energy_within_threshold", 5)):
            m[n].update(s[i])
        if s[2] != 0:
            m["pos_mae"].update(s[6], s[2])
    return m


def _batch():
    d = t6._slab_batch()
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in d.items()}


def test_is2rs_loop_schedules_and_meters():
    from equiformer_amd import train
    from equiformer_amd.is2rs import IS2RSLoss, auxiliary_task_weight, interpolate_init_relaxed_pos, step_seed
    from equiformer_amd.optim import FlatAdamW
    lam = _lam()
    batch = _batch()
    # the loop
    _, m = t6._models("aux")
    opt = FlatAdamW(m.parameters(), lr=LR, weight_decay=1e-2)
    ts = train.is2rs_train_step(m, opt, t6.R, pi.SLAB_CAP, auxiliary_task_weight=W0, seed=SEED, min_eager=3,
                                node_step=t6.NODE_STEP, edge_step=t6.EDGE_STEP, **t6.NORM)
    rec = dict(lr=[], w=[], losses=[], stats=[])
    step = ts.step

    def recorded(b):
        rec["lr"].append(opt.param_groups[0]["lr"])
        rec["w"].append(float(ts.loss._w_host[1]))
        loss = step(b)
        rec["losses"].append(float(loss))
        rec["stats"].append(ts.loss.stats.cpu())
        return loss
    ts.step = recorded
    lines = []
    got = train.train_one_epoch_is2rs(ts, [batch] * STEPS, lr_lambda=lam, total_steps=STEPS, print_freq=4, log=lines.append)
    torch.cuda.synchronize()
    assert (ts.eager_steps, ts.captures, ts.replays) == (3, 1, 5), (ts.eager_steps, ts.captures, ts.replays)
    # eager, unpadded: the same perturbation seeds, lr and weights
    _, m = t6._models("aux")
    opt = FlatAdamW(m.parameters(), lr=LR, weight_decay=1e-2)
    L = IS2RSLoss(auxiliary_task_weight=W0, **t6.NORM)
    e_losses, e_stats = [], []
    for k in range(STEPS):
        data = SimpleNamespace(**batch)
        interpolate_init_relaxed_pos(data, seed=step_seed(SEED, k))
        for g in opt.param_groups:
            g["lr"] = LR * lam(k)
        L.set_weights(auxiliary_task_weight=auxiliary_task_weight(W0, k + 1, STEPS))
        opt.zero_grad(set_to_none=True)
        out = m(data)
        loss = L(out[0], out[1], data)
        loss.backward()
        opt.step()
        e_losses.append(float(loss.detach()))
        e_stats.append(L.stats.cpu())
    torch.cuda.synchronize()
    # the schedules
    w = [auxiliary_task_weight(W0, k + 1, STEPS) for k in range(STEPS)]
    print("lr written %s\naux weight written %s" % (rec["lr"], rec["w"]))
    assert rec["lr"] == [LR * lam(k) for k in range(STEPS)] and len(set(rec["lr"])) > 4
    assert rec["w"] == w and w[0] == W0 - (W0 - 1.0) / STEPS and w[-1] == 1.0
    for k in range(STEPS):
        s = rec["stats"][k]
        made = s[0].item() + w[k] * s[1].item()
        assert abs(made - rec["losses"][k]) <= 1e-5 * max(1.0, abs(rec["losses"][k])), (k, w[k], made, rec["losses"][k])
    # bit for bit against the host restatement of the loop's own figures
    want = _host_meters(rec["losses"], rec["stats"])
    eager = _host_meters(e_losses, e_stats)
    assert set(got) == set(NAMES)
    for n in NAMES:
        g, h, x = got[n], want[n], eager[n]
        print("%s: loop %r / %r, host %r / %r, eager avg %.9f" % (n, g.sum, g.count, float(h.sum), float(h.count), x.sum / x.count))
        assert g.sum == float(h.sum) and g.count == float(h.count), n
        assert g.count == float(x.count) and g.count > 0, n
        want_avg = x.sum / x.count
        assert abs(g.avg - want_avg) <= 2e-5 * max(1.0, abs(want_avg)), (n, g.avg, want_avg)
    assert got["loss"].count == STEPS
    # log lines at the 1-based steps 1 (the first), 4, 8 (a multiple of print_freq and the last): three reads and the end
    assert len(lines) == 3 and ts.loss.meters.reads == 4 and "aux_weight: 1.00e+00" in lines[-1], lines
