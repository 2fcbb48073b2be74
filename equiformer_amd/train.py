"""Training loops on the HIP path for the three recipes bench.py measures: QM9, MD17 and plain IS2RE (no auxiliary head).
[ref: engine.py:30-107 train_one_epoch (QM9), main_md17.py:361-422 train_one_epoch, the energy term of
oc20/trainer/energy_trainer_v2.py:413-459 with base_trainer_v2.py's per-step scheduler]

The reference loops launch a loss written in ATen and stop the GPU for two (QM9) to four (MD17) `.item()` read-backs per step.
Here, per step:
  * the loss is ONE operator (eqf_ef_loss_fwd / _bwd, csrc/trainloss.hip: `ops.ef_loss`), whose forward also folds the batch
    into the ten fp64 running sums of `evaluate.Meter` (`evaluate.SUMS`), so the meters cost no launch and no read-back;
  * the step is a `BucketedTrainStep` (capture.py), exactly as `dens.DeNSTrainStep` wraps one: model + loss + backward +
    AdamW replay as one HIP graph per shape bucket; the energy and force weights are device words (`EFLoss.set_weights`);
  * the loop reads the sums back once per log line and once at the end.  The graph build's own host read-back remains.
What the loops report comes from the sums (`figures`): the reference's AverageMeter averages per-batch means weighted by
the batch size, which is the ratio of two sums.

Schedules: `lr_lambda_cosine` / `lr_lambda_multistep` are the OC20 trainer's per-step factors, `cosine_epoch_lr` the per-epoch
timm cosine schedule of the QM9 and MD17 drivers -- pure host functions.  A captured AdamW reads lr from its device word, so a
`param_group["lr"]` written before a step reaches the replay.  `compute_stats` is engine.compute_stats on the count half of the
GPU graph build."""
import ctypes
import math
import time

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops
from .capture import BucketedTrainStep, _MirrorsBucketed, _refuse_reducer
from .evaluate import Meter, _avg
from .lib import call
from .ops import _c, _p, _stream

CRITERIA = tuple(ops.EF_CRITERIA)


class _EFLoss(Function):
    """ops.ef_loss.  First order only: pred_dy carries the second-order graph of the forces, the loss does not.  The backward
    recomputes the atom count from row_mask: nothing the forward wrote is read (a shared acc is only ever added to)."""

    @staticmethod
    def forward(ctx, pred_y, pred_dy, y, dy, row_mask, weights, acc, n_graphs, crit, mean, std, threshold):
        pred_y, y = _c(pred_y), _c(y)
        pred_dy = None if pred_dy is None else _c(pred_dy)
        dy = None if dy is None else _c(dy)
        N = 0 if pred_dy is None else pred_dy.shape[0]
        loss = torch.empty((), device=pred_y.device, dtype=torch.float32)
        call("eqf_ef_loss_fwd", _p(pred_y), _p(y), n_graphs, _p(pred_dy), _p(dy), _p(row_mask), N, _p(weights), crit, mean, std,
             threshold, _p(loss), None if acc is None else ctypes.c_void_p(acc.data_ptr()), _stream())
        ctx.consts = (n_graphs, N, crit, mean, std)
        ctx.save_for_backward(pred_y, pred_dy, y, dy, row_mask, weights)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, d_loss):
        pred_y, pred_dy, y, dy, row_mask, weights = ctx.saved_tensors
        n_graphs, N, crit, mean, std = ctx.consts
        d_loss = _c(d_loss.to(torch.float32))
        d_pred_y = torch.empty_like(pred_y)
        d_pred_dy = None if pred_dy is None else torch.empty_like(pred_dy)
        call("eqf_ef_loss_bwd", _p(d_loss), _p(pred_y), _p(y), n_graphs, pred_y.numel(), _p(pred_dy), _p(dy), _p(row_mask), N,
             _p(weights), crit, mean, std, _p(d_pred_y), _p(d_pred_dy), _stream())
        return d_pred_y, d_pred_dy, None, None, None, None, None, None, None, None, None, None


class EFLoss:
    """loss = EFLoss(task_mean, task_std, criterion, energy_weight=1, force_weight=0, threshold=0.02)
       l = loss(pred_y, y, n_graphs[, pred_dy, dy, row_mask])      # every step: one launch, nothing read back

    energy_weight C(pred_y[:n_graphs], (y - mean) / std) + force_weight C(pred_dy, dy / std) over the real rows, one criterion
    C in {"l1", "l2" (MSE), "l2mae"} for both terms as the reference applies it (main_md17.py:384-386).  Every call also adds
    the batch to `.meter` (an evaluate.Meter: `.meter.read()` and `Meter.figures` / `figures` below apply); reset it per epoch.
    The weights are two fp32 device words (`set_weights`, the DeNSLoss idiom): a captured step sees a changed weight."""

    def __init__(self, task_mean, task_std, criterion, energy_weight=1.0, force_weight=0.0, threshold=0.02, device=None):
        if criterion not in ops.EF_CRITERIA:
            raise ValueError("EFLoss: criterion %r is not one of %s" % (criterion, sorted(ops.EF_CRITERIA)))
        self.criterion = criterion
        self.meter = Meter(task_mean, task_std, threshold, device=device)
        self.task_mean, self.task_std, self.threshold = self.meter.task_mean, self.meter.task_std, self.meter.threshold
        self.weights = torch.zeros(2, dtype=torch.float32, device=self.meter.acc.device)
        self._w_host = torch.zeros(2, dtype=torch.float32).pin_memory()
        self.set_weights(energy_weight, force_weight)

    def set_weights(self, energy_weight=None, force_weight=None):
        """Write the device words (None keeps a weight): pinned buffer, asynchronous copy, no synchronisation.  (A step's graph
        build reads back on the host, so the copy has landed before the next call here can touch the pinned words.)"""
        for i, w in enumerate((energy_weight, force_weight)):
            if w is not None:
                self._w_host[i] = float(w)
        self.weights.copy_(self._w_host, non_blocking=True)

    def __call__(self, pred_y, y, n_graphs, pred_dy=None, dy=None, row_mask=None):
        """pred_y, y: [rows] or [rows, 1] with rows >= n_graphs (a padded batch carries the phantom molecule's row); pred_dy, dy
        [N, 3]; row_mask [N] fp32, 1 real / 0 phantom (`view.node_mask`)."""
        y = y.detach()
        if y.dtype != torch.float32:
            y = y.to(torch.float32)
        if dy is not None and dy.dtype != torch.float32:
            dy = dy.detach().to(torch.float32)
        return ops.ef_loss(pred_y, y, n_graphs, self.weights, self.task_mean, self.task_std, self.criterion, pred_dy=pred_dy,
                           dy=dy, row_mask=row_mask, acc=self.meter.acc, threshold=self.threshold)


def figures(sums, criterion, task_std):
    """What the reference training loops report, from the ten sums (a pure host function):
      "qm9":  (mae, loss) of engine.train_one_epoch (its return value is the mae);
      "md17": (mae_metrics, loss_metrics) of main_md17.train_one_epoch, each {"energy": Average, "force": Average};
      "oc20": Meter.figures' IS2RE triple, and "oc20_loss" the mean energy loss.
    The loss averages are the criterion's, on the normalised targets, before the weights: "l1" and "l2mae" energies
    abs_norm / n; "l2" energies sq_err / (n std^2) -- the mean training loss under MSE; forces: "l2mae" force_l2 / atoms,
    "l1" force_abs_norm / (3 atoms), "l2" force_sq_err / (3 atoms std^2).  (The "l2" forms are exact in real arithmetic: the
    sums hold the error in the target's units, e = std d.)  With "l2mae" the result equals Meter.figures (evaluate_md17's
    shape).  A count of zero gives NaN averages."""
    if criterion not in ops.EF_CRITERIA:
        raise ValueError("criterion %r is not one of %s" % (criterion, sorted(ops.EF_CRITERIA)))
    base = Meter.figures(sums)
    n, atoms, s2 = sums["graphs"], sums["atoms"], float(task_std) ** 2
    loss_e = _avg(sums["sq_err"] / s2 if criterion == "l2" else sums["abs_norm"], n)
    if criterion == "l2mae":
        loss_f = _avg(sums["force_l2"], atoms)
    else:
        total = sums["force_sq_err"] / s2 if criterion == "l2" else sums["force_abs_norm"]
        loss_f = _avg(total / 3.0, atoms)
    mae_metrics = base["md17"][0]
    return {"qm9": (base["qm9"][0], loss_e.avg), "md17": (mae_metrics, {"energy": loss_e, "force": loss_f}),
            "oc20": base["oc20"], "oc20_loss": loss_e.avg}


# ------------------------------------------------------------------------------------------------------------------------- steps
class EFTrainStep(_MirrorsBucketed):
    """ts = EFTrainStep(kind, model, optimizer, loss, radius, **bucket_kwargs)   (made by qm9_train_step, md17_train_step,
       l = ts.step(batch)                                                         oc20_train_step)

    A `BucketedTrainStep` whose forward_loss is the model on the padded view and `loss(E, view.y, view.B[, forces, view.dy,
    view.node_mask])`: the phantom molecule's energy row and the phantom atoms stay out of the loss and out of the meter.
    `.loss`: the EFLoss (its `.meter` holds the running sums); `.bucketed`: the BucketedTrainStep (its counters are mirrored
    here); `.steps`: steps taken by this instance (the OC20 loop's scheduler step); `.lr_initial`: the optimizer's lr at
    construction."""

    KINDS = ("qm9", "md17", "oc20")

    def __init__(self, kind, model, optimizer, loss, radius, **bucket_kwargs):
        if kind not in self.KINDS:
            raise ValueError("EFTrainStep: kind %r is not one of %s" % (kind, self.KINDS))
        self.kind, self.model, self.optimizer, self.loss = kind, model, optimizer, loss
        self.lr_initial = float(optimizer.param_groups[0]["lr"])
        self.steps = 0
        node_targets = {"qm9": (), "md17": ("dy",), "oc20": ("tags",)}[kind]
        self._predict = getattr(self, "_predict_" + kind)
        if kind == "md17":
            from .nets.equiformer_md17_dens import Equiformer_MD17_DeNS
            self._dens = isinstance(model, Equiformer_MD17_DeNS)
        self.bucketed = BucketedTrainStep(optimizer, self._forward_loss, radius, graph_targets=("y",), node_targets=node_targets,
                                          **bucket_kwargs)

    def _predict_qm9(self, g, v):
        return self.model(None, v.pos, v.batch, v.z, graph=g), None

    def _predict_md17(self, g, v):
        if self._dens:  # (an uncorrupted view: no force / noise_mask, plain energy and forces)
            return self.model(v, graph=g)
        return self.model(node_atom=v.z, pos=v.pos, batch=v.batch, graph=g)

    def _predict_oc20(self, g, v):
        out = self.model(v, graph=g, offsets=v.offsets)
        return (out[0] if isinstance(out, tuple) else out), None

    def _forward_loss(self, g, view):
        energy, forces = self._predict(g, view)
        if forces is None:
            return self.loss(energy, view.y, view.B)
        return self.loss(energy, view.y, view.B, forces, view.dy, view.node_mask)

    def step(self, batch):
        self.steps += 1
        return self.bucketed.step(batch)


def qm9_train_step(model, optimizer, norm_factor, radius, criterion="l1", threshold=0.02, **bucket_kwargs):
    """The EFTrainStep of `train_one_epoch_qm9` (keep it between epochs: its graphs are reused).  norm_factor: (mean, std);
    criterion: the driver's loss (main_qm9.py: L1Loss).  bucket_kwargs: those of BucketedTrainStep."""
    _refuse_reducer(optimizer, "qm9_train_step")
    dev = next(model.parameters()).device
    loss = EFLoss(float(norm_factor[0]), float(norm_factor[1]), criterion, 1.0, 0.0, threshold, device=dev)
    return EFTrainStep("qm9", model, optimizer, loss, radius, **bucket_kwargs)


def md17_train_step(model, optimizer, radius, energy_weight, force_weight, criterion="l2mae", task_mean=None, task_std=None,
                    threshold=0.02, **bucket_kwargs):
    """The EFTrainStep of `train_one_epoch_md17`.  model: GraphAttentionTransformerMD17, or Equiformer_MD17_DeNS on uncorrupted
    batches (called with the padded view as its `data`); task_mean / task_std default to the model's.  energy_weight /
    force_weight: the driver's --energy-weight / --force-weight (EFLoss.set_weights changes them later)."""
    _refuse_reducer(optimizer, "md17_train_step")
    dev = next(model.parameters()).device
    task_mean = getattr(model, "task_mean", None) if task_mean is None else task_mean
    task_std = getattr(model, "task_std", None) if task_std is None else task_std
    if task_mean is None or task_std is None:
        raise ValueError("md17_train_step: the model carries no task_mean / task_std; pass them")
    loss = EFLoss(float(task_mean), float(task_std), criterion, energy_weight, force_weight, threshold, device=dev)
    return EFTrainStep("md17", model, optimizer, loss, radius, **bucket_kwargs)


def oc20_train_step(model, optimizer, radius, task_mean=0.0, task_std=1.0, criterion="l1", energy_weight=1.0, threshold=0.02,
                    **bucket_kwargs):
    """The EFTrainStep of `train_one_epoch_oc20`: periodic batches (`cell`), graph built on the fly -- or, with edges="batch"
    among bucket_kwargs, from the batch's own edge_index / cell_offsets / neighbors.  task_mean / task_std: the trainer's target
    normalizer (0, 1 without normalize_labels); criterion: its loss_energy ("mae" = "l1", "mse" = "l2", "l2mae");
    energy_weight: its energy_coefficient.  A model with the auxiliary IS2RS head is refused: its step is is2rs.IS2RSTrainStep."""
    if getattr(model, "use_auxiliary_task", False):
        raise ValueError("oc20_train_step: the model has the auxiliary IS2RS head (use_auxiliary_task=True); "
                         "train it with equiformer_amd.is2rs.IS2RSTrainStep")
    _refuse_reducer(optimizer, "oc20_train_step")
    dev = next(model.parameters()).device
    loss = EFLoss(task_mean, task_std, criterion, energy_weight, 0.0, threshold, device=dev)
    return EFTrainStep("oc20", model, optimizer, loss, radius, **bucket_kwargs)


# ------------------------------------------------------------------------------------------------------------------------- loops
def _check_step(step, kind):
    if not isinstance(step, EFTrainStep) or step.kind != kind:
        raise ValueError("train_one_epoch_%s needs the step of %s_train_step" % (kind, kind))


def _check_clip(step, clip_grad):
    if clip_grad is not None and clip_grad != getattr(step.optimizer, "clip_grad", None):
        raise ValueError("clip_grad=%r: clipping is the optimizer's (FlatAdamW(clip_grad=...)); the step's optimizer has %r"
                         % (clip_grad, getattr(step.optimizer, "clip_grad", None)))


def _epoch(step, loader, prepare, line, print_freq, log, before=None):
    """the loop all three share: meter reset, one step per batch, no read-back but the log lines' and the final one"""
    step.model.train()
    meter = step.loss.meter
    meter.reset()
    length = len(loader) if hasattr(loader, "__len__") else None
    start = time.perf_counter()
    for k, batch in enumerate(loader):
        if before is not None:
            before()
        step.step(prepare(batch))
        if log is not None and (k % print_freq == 0 or (length is not None and k == length - 1)):
            f = figures(meter.read(), step.loss.criterion, step.loss.task_std)
            ms = 1e3 * (time.perf_counter() - start) / (k + 1)
            log("[%d/%s] \t%s, time/step=%.0fms, lr=%.2e" % (k, length if length is not None else "?", line(f), ms,
                                                             step.optimizer.param_groups[0]["lr"]))
    return figures(meter.read(), step.loss.criterion, step.loss.task_std)


def train_one_epoch_qm9(step, loader, target=None, print_freq=100, log=None, clip_grad=None):
    """The mae of engine.train_one_epoch [ref: engine.py:30-107]: the MAE in the target's units averaged over the molecules.
    step: qm9_train_step(...); loader: batch mappings with pos, z, batch, y ([B], or [B, T] of which column `target` is taken)
    on the model's device.  log: a callable taking one line (logger.info), called every print_freq steps and at the last one.
    clip_grad: the optimizer clips (FlatAdamW(clip_grad=...)); a different value here is refused."""
    _check_step(step, "qm9")
    _check_clip(step, clip_grad)

    def column(batch):
        y = batch["y"]
        return batch if y.dim() < 2 else dict(batch, y=y[:, target])
    f = _epoch(step, loader, column, lambda f: "loss: %.5f, MAE: %.5f" % (f["qm9"][1], f["qm9"][0]), print_freq, log)
    return f["qm9"][0]


def train_one_epoch_md17(step, loader, print_freq=100, log=None):
    """(mae_metrics, loss_metrics) of main_md17.train_one_epoch [ref: main_md17.py:361-422], shaped as evaluate_md17 returns
    them: each {"energy": Average, "force": Average}; the losses are the criterion's on the normalised targets, the MAEs in
    real units (forces averaged over x, y, z).  loader: batch mappings with pos, z, batch, y [B] or [B, 1], dy [N, 3]."""
    _check_step(step, "md17")

    def line(f):
        mae, loss = f["md17"]
        return "loss_e: %.5f, loss_f: %.5f, e_MAE: %.5f, f_MAE: %.5f" % (loss["energy"].avg, loss["force"].avg,
                                                                        mae["energy"].avg, mae["force"].avg)
    return _epoch(step, loader, lambda b: b, line, print_freq, log)["md17"]


def train_one_epoch_oc20(step, loader, lr_lambda=None, print_freq=100, log=None, lr_initial=None):
    """(metrics, loss) of one epoch of the OC20 energy trainer without the auxiliary head [ref: energy_trainer_v2.py:413-459,
    base_trainer_v2.py's per-step `scheduler.step()`]: metrics = {"energy_mae", "energy_mse", "energy_within_threshold"}, each
    {"metric", "total", "numel"}; loss = the mean energy loss (figures).  lr_lambda: k -> factor (lr_lambda_cosine /
    lr_lambda_multistep with their parameters bound); before step k of the instance (`step.steps`, counted over epochs) the
    loop writes param_group["lr"] = lr_initial * lr_lambda(k) (lr_initial: the step's `.lr_initial` by default).  loader: batch
    mappings with pos, atomic_numbers, batch, cell, tags, y (= y_relaxed)[, the given edge fields for edges="batch"]."""
    _check_step(step, "oc20")
    lr0 = step.lr_initial if lr_initial is None else float(lr_initial)

    def set_lr():
        if lr_lambda is not None:
            lr = lr0 * lr_lambda(step.steps)
            for g in step.optimizer.param_groups:
                g["lr"] = lr

    def line(f):
        return "loss: %.5f, energy_mae: %.5f" % (f["oc20_loss"], f["oc20"]["energy_mae"]["metric"])
    f = _epoch(step, loader, lambda b: b, line, print_freq, log, before=set_lr)
    return f["oc20"], f["oc20_loss"]


# --------------------------------------------------------------------------------------------------------------------- schedules
def lr_lambda_cosine(step, warmup, warmup_factor, total, lr_min_factor):
    """The OC20 trainer's per-step cosine factor [ref: oc20/trainer/lr_scheduler.py:20-34 cosine_lr_lambda]: a linear warm-up
    from warmup_factor to 1 over `warmup` steps (step <= warmup), then lr_min_factor + (1 - lr_min_factor) (1 + cos(pi step /
    total)) / 2, and lr_min_factor from `total` on.  (`warmup` and `total` count steps: epochs times iterations per epoch.)"""
    if step <= warmup:
        alpha = step / float(warmup)
        return warmup_factor * (1.0 - alpha) + alpha
    if step >= total:
        return lr_min_factor
    return lr_min_factor + 0.5 * (1 - lr_min_factor) * (1 + math.cos(math.pi * (step / total)))


def lr_lambda_multistep(step, warmup, warmup_factor, decay_steps, decay_rate):
    """The OC20 trainer's per-step multistep factor [ref: oc20/trainer/lr_scheduler.py:57-68 multistep_lr_lambda]: the same
    warm-up, then decay_rate ** (the number of milestones in `decay_steps` (ascending) that are <= step)."""
    if step <= warmup:
        alpha = step / float(warmup)
        return warmup_factor * (1.0 - alpha) + alpha
    return pow(decay_rate, sum(1 for m in decay_steps if m <= step))


def cosine_epoch_lr(epoch, lr, epochs, warmup_epochs=0, warmup_lr=1e-6, min_lr=1e-5):
    """The learning rate of epoch `epoch` (from 0) under the timm cosine schedule the QM9 and MD17 drivers create
    (main_qm9.py:186 / main_md17.py:196 create_scheduler with --sched cosine; the driver calls step(epoch) after each epoch).
    timm is not a dependency here; this restates timm 0.4.12 (the reference's environment), scheduler/cosine_lr.py
    CosineLRScheduler._get_lr with t_mul = 1, decay_rate applied only past the one cycle (cycle_limit = 1), warmup_prefix off:
      epoch < warmup_epochs:   warmup_lr + epoch (lr - warmup_lr) / warmup_epochs
      epoch < epochs:          min_lr + (lr - min_lr) (1 + cos(pi epoch / epochs)) / 2
      otherwise:               min_lr"""
    if epoch < warmup_epochs:
        return warmup_lr + epoch * (lr - warmup_lr) / warmup_epochs
    if epoch < epochs:
        return min_lr + 0.5 * (lr - min_lr) * (1 + math.cos(math.pi * epoch / epochs))
    return min_lr


# ------------------------------------------------------------------------------------------------------------------------- stats
def compute_stats(loader, radius, max_num_neighbors=1000):
    """(avg_node, avg_edge, avg_degree) of engine.compute_stats [ref: engine.py:144-176]: nodes and edges per molecule averaged
    with the molecule count as weight, the degree (edges per node) with the node count.  Runs the COUNT half of the GPU graph
    build only (EdgeGraph.radius_plan: one host read-back per batch, no edge list).  loader: batch mappings with pos, batch on
    the GPU."""
    from .graph import EdgeGraph
    nodes = edges = mols = 0.0
    for batch in loader:
        pos, b = batch["pos"], batch["batch"]
        if not (pos.is_cuda and b.is_cuda):
            raise ops.HipOnlyError("compute_stats runs the GPU graph build; the batch is on %s / %s" % (pos.device, b.device))
        B = int(batch["num_graphs"]) if "num_graphs" in batch else int(b[-1].item()) + 1
        plan = EdgeGraph.radius_plan(pos, b, radius, max_num_neighbors, B)
        nodes += plan.N
        edges += plan.E
        mols += B
    if not mols:
        return float("nan"), float("nan"), float("nan")
    return nodes / mols, edges / mols, edges / nodes
