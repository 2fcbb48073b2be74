"""train_one_epoch_dens (equiformer_amd/train.py) on the GPU, with the model and the two-frame aspirin batch of
tests/test_gpu_dens_step.py (42 atoms, one bucket at edge_step 1024):

  * two epochs of 4 steps with the linear decay (epochs = 2: denoising weight 10, then 5), min_eager 3: 3 eager steps, one
    capture, 5 replays.  The returned sums and counts equal a host AverageMeter fed the loop's own per-step stats (read back by
    the test, after every step) bit for bit; they are within the per-step loss bound of test_captured_step_equals_eager_loop
    (1e-4 of max(1, |x|)) of an eager, unpadded loop with the same seeds, the counts equal; every replay's loss is made of the
    decayed weight (the `made =` identity of that test, 1e-5).
  * the meters are read once per log line and once at the end of each epoch.
  * prob 1 without corrupt_ratio (every atom corrupted): the force meters never move (count 0, avg NaN); prob 0: the denoising
    meters never move."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import test_gpu_dens_step as tds  # noqa: E402  (the model, R, the captured-step protocol)

DEV = torch.device("cuda:0")
MEAN, STD = 0.3, 1.7
NSTD, PROB, RATIO, SEED = 0.05, 0.75, 0.5, 99
W_E, W_F, W_D = 1.0, 80.0, 10.0
PARTS = ("energy", "force", "denoising_pos")


class AverageMeter:
    """engine.py:12-27"""

    def __init__(self):
        self.sum, self.count = 0, 0

    def update(self, val, n=1):
        self.sum += val * n
        self.count += n


def _batch():
    from equiformer_amd.synthetic import md17_aspirin_batch
    d = md17_aspirin_batch(2, seed=3)
    return dict({k: d[k].to(DEV) for k in ("pos", "z", "batch", "y", "dy")}, num_graphs=2)


def _host_meters(stats_list):
    """main_md17_dens.py:411-427 on per-step stats (dens.STATS order), B = 2 molecules; a zero count skips the update"""
    loss = {p: AverageMeter() for p in PARTS}
    mae = {p: AverageMeter() for p in PARTS}
    for s in stats_list:
        s = s.tolist()
        for i, p in enumerate(PARTS):
            n = 2 if p == "energy" else s[3 if p == "force" else 4]
            if n != 0:
                loss[p].update(s[i], n)
                mae[p].update(s[5 + i], n)
    return mae, loss


def _recording(ts):
    rec = dict(w=[], losses=[], stats=[])
    step = ts.step

    def recorded(batch):
        rec["w"].append(float(ts.loss._w_host[2]))
        loss = step(batch)
        rec["losses"].append(float(loss))
        rec["stats"].append(ts.loss.stats.cpu())
        return loss
    ts.step = recorded
    return rec


def _loop(prob, ratio, epochs, steps_per_epoch, min_eager, print_freq=2):
    from equiformer_amd import train
    from equiformer_amd.optim import FlatAdamW
    _, m = tds._models()
    opt = FlatAdamW(m.parameters(), lr=5e-4, weight_decay=1e-6)
    ts = train.dens_train_step(m, opt, tds.R, NSTD, prob, W_E, W_F, W_D, corrupt_ratio=ratio, task_mean=MEAN, task_std=STD,
                               seed=SEED, min_eager=min_eager, edge_step=1024)
    rec = _recording(ts)
    batch = _batch()
    out, lines, reads = [], [], []
    for epoch in range(epochs):
        before = (len(lines), ts.loss.meters.reads)
        out.append(train.train_one_epoch_dens(ts, [batch] * steps_per_epoch, epoch, epochs, W_D, linear_decay=True,
                                              print_freq=print_freq, log=lines.append))
        reads.append((len(lines) - before[0], ts.loss.meters.reads - before[1]))
    torch.cuda.synchronize()
    return dict(out=out, rec=rec, ts=ts, lines=lines, reads=reads, m=opt.flat_m.detach().clone())


def _eager(epochs, steps_per_epoch):
    """test_captured_step_equals_eager_loop's eager branch, the weight decayed per epoch, the reference's meters per epoch"""
    from equiformer_amd import train
    from equiformer_amd.dens import DeNSLoss, add_masked_gaussian_noise_to_pos, step_seed
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.optim import FlatAdamW
    _, m = tds._models()
    opt = FlatAdamW(m.parameters(), lr=5e-4, weight_decay=1e-6)
    L = DeNSLoss(MEAN, STD, NSTD, W_E, W_F, W_D)
    batch = _batch()
    out, losses = [], []
    for epoch in range(epochs):
        L.set_weights(denoising_pos_weight=train.dens_denoising_pos_weight(W_D, epoch, epochs))
        stats = []
        for j in range(steps_per_epoch):
            k = epoch * steps_per_epoch + j
            data = SimpleNamespace(**{n: batch[n] for n in ("pos", "z", "batch", "y", "dy")})
            add_masked_gaussian_noise_to_pos(data, NSTD, PROB, RATIO, seed=step_seed(SEED, k))
            opt.zero_grad(set_to_none=True)
            g = EdgeGraph.from_radius(data.pos, data.batch, tds.R, num_graphs=2)
            E, Y = m(data, graph=g)
            loss = L(E, Y, data)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
            stats.append(L.stats.cpu())
        out.append(_host_meters(stats))
    torch.cuda.synchronize()
    return out, losses


def test_dens_loop_meters_equal_the_host_restatement_and_the_eager_loop():
    b = _loop(PROB, RATIO, epochs=2, steps_per_epoch=4, min_eager=3)
    ts, rec = b["ts"], b["rec"]
    assert (ts.eager_steps, ts.captures, ts.replays) == (3, 1, 5), (ts.eager_steps, ts.captures, ts.replays)
    e, e_losses = _eager(2, 4)
    for epoch in range(2):
        mae, loss = b["out"][epoch]
        want_mae, want_loss = _host_meters(rec["stats"][4 * epoch:4 * epoch + 4])
        eager_mae, eager_loss = e[epoch]
        for kind, got, want, eager in (("mae", mae, want_mae, eager_mae), ("loss", loss, want_loss, eager_loss)):
            for p in PARTS:
                g, w, x = got[p], want[p], eager[p]
                print("epoch %d %s %s: loop %r / %r, host %r / %r, eager avg %.9f" % (epoch, kind, p, g.sum, g.count, float(w.sum),
                                                                                     float(w.count), x.sum / x.count))
                # bit for bit: the device's fp64 additions are the host's
                assert g.sum == float(w.sum) and g.count == float(w.count), (epoch, kind, p)
                assert g.count == float(x.count) and g.count > 0, (epoch, kind, p)
                want_avg = x.sum / x.count
                assert abs(g.avg - want_avg) <= 1e-4 * max(1.0, abs(want_avg)), (epoch, kind, p, g.avg, want_avg)
    for k in range(8):
        assert abs(rec["losses"][k] - e_losses[k]) <= 1e-4 * max(1.0, abs(e_losses[k])), (rec["losses"], e_losses)
        # the loss a replay returns is made of the device weights of that epoch
        w_d = 10.0 if k < 4 else 5.0
        assert rec["w"][k] == w_d
        s = rec["stats"][k]
        made = W_E * s[0].item() + W_F * s[1].item() + w_d * s[2].item()
        assert abs(made - rec["losses"][k]) <= 1e-5 * max(1.0, abs(rec["losses"][k])), (k, made, rec["losses"][k])
    assert any(rec["stats"][k][2].item() > 0 for k in range(4, 8)), "the decayed weight needs corrupted atoms in a replay"
    # one read-back per log line (print_freq 2: steps 0, 2 and the last, 3) and one at the end, per epoch
    assert b["reads"] == [(3, 4), (3, 4)], b["reads"]
    assert b["lines"][3].startswith("Epoch: [1][0/4] \tloss_e: ") and b["lines"][3].endswith("denoising_pos_weight=5.00e+00")


@pytest.mark.parametrize("prob,empty", [(1.0, "force"), (0.0, "denoising_pos")])
def test_dens_loop_empty_atom_sets_leave_their_meters(prob, empty):
    """3 steps, min_eager 1: eager, capture, replay"""
    b = _loop(prob, None, epochs=1, steps_per_epoch=3, min_eager=1, print_freq=100)
    ts = b["ts"]
    assert (ts.eager_steps, ts.captures, ts.replays) == (1, 1, 2), (ts.eager_steps, ts.captures, ts.replays)
    mae, loss = b["out"][0]
    for metrics in (mae, loss):
        assert metrics[empty].count == 0.0 and metrics[empty].sum == 0.0 and metrics[empty].avg != metrics[empty].avg
        for p in PARTS:
            if p != empty:
                assert metrics[p].count == (6.0 if p == "energy" else 3 * 42.0) and metrics[p].avg == metrics[p].avg, p
    assert b["reads"] == [(2, 3)]  # the log lines of step 0 and of the last step, and the end
