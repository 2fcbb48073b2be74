"""Training loops on the HIP path for the five recipes: QM9, MD17 and plain IS2RE (no auxiliary head), DeNS and IS2RE + IS2RS.
[ref: engine.py:30-107 train_one_epoch (QM9), main_md17.py:361-422 train_one_epoch, the energy term of
oc20/trainer/energy_trainer_v2.py:413-459 with base_trainer_v2.py's per-step scheduler, main_md17_dens.py:349-450
train_one_epoch (DeNS), energy_trainer_v2.py:240-317 the training loop of the _aux configurations (IS2RE + IS2RS)]

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
GPU graph build.

The DeNS and IS2RE + IS2RS loops run the steps of dens.py / is2rs.py, whose fused losses leave one step's means in an fp32
`stats` buffer.  Their metered losses (`DeNSMeteredLoss`, `IS2RSMeteredLoss`) fold those means into `RunningMeters`, fp64
(sum, count) pairs on the device (eqf_meter_fold, csrc/meters.hip: one launch inside forward_loss, so an eager, captured or
replayed step is counted once), and the loops read the pairs back once per log line and once at the end."""
import ctypes
import math
import time

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import is2rs, ops
from .capture import BucketedTrainStep, _MirrorsBucketed, _refuse_reducer
from .dens import DeNSLoss, DeNSTrainStep
from .evaluate import Meter, _avg
from .is2rs import IS2RSLoss, IS2RSTrainStep
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


# ------------------------------------------------------------------------------------------------------------ running meters
METERS_MAX = 16    # EQF_METERS_MAX
LOSS = "loss"      # a meter's value: the loss scalar the step returns
GRAPHS = "graphs"  # a meter's weight: the step's graph count (view.B: constant within a bucket)
ONE = "one"        # a meter's weight: 1 (one update per step)

# (name, value, weight): value an index into the loss's `stats` or LOSS; weight an index into `stats`, GRAPHS or ONE.
# DeNS [ref: main_md17_dens.py:411-427]: dens.STATS = loss_e, loss_f, loss_d, n_f, n_d, mae_e, mae_f, mae_d
DENS_METERS = (("loss_energy", 0, GRAPHS), ("loss_force", 1, 3), ("loss_denoising_pos", 2, 4),
               ("mae_energy", 5, GRAPHS), ("mae_force", 6, 3), ("mae_denoising_pos", 7, 4))
# IS2RE + IS2RS [ref: energy_trainer_v2.py:247-288, one update per step]: is2rs.STATS = loss_e, loss_aux, n_free, energy_mae,
# energy_mse, energy_within_threshold, pos_mae; pos_mae (weighted by n_free) is no reference figure
IS2RS_METERS = (("loss", LOSS, ONE), ("energy_mae", 3, ONE), ("energy_mse", 4, ONE), ("energy_within_threshold", 5, ONE),
                ("pos_mae", 6, 2))


class RunningMeters:
    """meters = RunningMeters(spec, device)     spec: ((name, value, weight), ...), as DENS_METERS / IS2RS_METERS
       meters.fold(stats, loss, graphs)        # every step: one launch (eqf_meter_fold), nothing read back
       meters.averages()                       # {name: evaluate.Average}: one read-back

    The reference's AverageMeter per name [ref: engine.py:23-27 update(val, n)]: meter i adds value * weight and weight to the
    fp64 pair acc[2i], acc[2i + 1] of ONE device buffer (allocated here, outside any capture: a captured fold writes its
    address), and is left as it is when the weight is 0.  The sums equal a host AverageMeter fed the same fp32 values, bit for
    bit.  `reads` counts the read-backs."""

    def __init__(self, spec, device):
        spec = tuple((str(n), v, w) for n, v, w in spec)
        if not 1 <= len(spec) <= METERS_MAX:
            raise ValueError("RunningMeters: 1 to %d meters, got %d" % (METERS_MAX, len(spec)))
        for n, v, w in spec:
            if not (v == LOSS or (isinstance(v, int) and v >= 0)) or not (w in (GRAPHS, ONE) or (isinstance(w, int) and w >= 0)):
                raise ValueError("RunningMeters: meter %r has value %r, weight %r" % (n, v, w))
        self.spec, self.names = spec, tuple(n for n, _, _ in spec)
        M = len(spec)
        self.acc = torch.zeros(2 * M, dtype=torch.float64, device=device)
        self._value = (ctypes.c_int * M)(*[-1 if v == LOSS else v for _, v, _ in spec])
        self._weight = (ctypes.c_int * M)(*[-1 if w in (GRAPHS, ONE) else w for _, _, w in spec])
        self.reads = 0

    def fold(self, stats, loss, graphs=None):
        """stats: the loss's fp32 stats buffer; loss: its fp32 scalar; graphs: the step's graph count (meters weighted by
        GRAPHS).  Enqueue-only: legal inside a capture, which keeps `graphs` as it was."""
        if not self.acc.is_cuda:
            raise ops.HipOnlyError("RunningMeters.fold runs on MI355X only (the meters are on %s)" % self.acc.device)
        if stats.dtype != torch.float32 or loss.dtype != torch.float32 or loss.numel() != 1 or not stats.is_contiguous():
            raise ValueError("RunningMeters.fold: stats must be a contiguous fp32 buffer and loss an fp32 scalar")
        const = []
        for n, _, w in self.spec:
            if w == GRAPHS and graphs is None:
                raise ValueError("RunningMeters.fold: meter %r is weighted by the graph count; pass graphs" % n)
            const.append(float(graphs) if w == GRAPHS else 1.0)
        M = len(self.spec)
        call("eqf_meter_fold", _p(stats), stats.numel(), _p(loss), M, self._value, self._weight, (ctypes.c_double * M)(*const),
             ctypes.c_void_p(self.acc.data_ptr()), _stream())

    def reset(self):
        """a fill on the stream"""
        self.acc.zero_()

    def read(self):
        """{name: (sum, count)}: the one read-back"""
        self.reads += 1
        a = self.acc.tolist()
        return {n: (a[2 * i], a[2 * i + 1]) for i, n in enumerate(self.names)}

    def averages(self, sums=None):
        """{name: evaluate.Average(avg, sum, count)} of `sums` (default: read()); a count of 0 gives avg NaN (the reference
        prints 0 there)"""
        sums = self.read() if sums is None else sums
        return {n: _avg(*sums[n]) for n in self.names}


class DeNSMeteredLoss(DeNSLoss):
    """A dens.DeNSLoss that folds every call's stats into `.meters` (RunningMeters of DENS_METERS): after the loss launch, in the
    same forward, so the step is counted once whether it runs eager, is captured (recorded, not run) or replayed."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.meters = RunningMeters(DENS_METERS, self.stats.device)

    def __call__(self, pred_y, pred_dy, data, row_mask=None, num_graphs=None):
        loss = super().__call__(pred_y, pred_dy, data, row_mask=row_mask, num_graphs=num_graphs)
        self.meters.fold(self.stats, loss, pred_y.shape[0] if num_graphs is None else num_graphs)
        return loss


class IS2RSMeteredLoss(IS2RSLoss):
    """An is2rs.IS2RSLoss that folds every call's stats and its returned loss into `.meters` (RunningMeters of IS2RS_METERS),
    as DeNSMeteredLoss does."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.meters = RunningMeters(IS2RS_METERS, self.stats.device)

    def __call__(self, pred_y, pred_pos, data, row_mask=None, num_graphs=None):
        loss = super().__call__(pred_y, pred_pos, data, row_mask=row_mask, num_graphs=num_graphs)
        self.meters.fold(self.stats, loss)
        return loss


def dens_train_step(model, optimizer, radius, denoising_pos_std, prob, energy_weight, force_weight, denoising_pos_weight,
                    corrupt_ratio=None, task_mean=None, task_std=None, seed=0, **bucket_kwargs):
    """The dens.DeNSTrainStep of `train_one_epoch_dens`, its loss a DeNSMeteredLoss (keep the step between epochs: its graphs
    are reused).  denoising_pos_std / prob / corrupt_ratio: the driver's --denoising-pos-std / -prob / --denoising-corrupt-ratio
    (the corruption's std is the loss's); the weights: --energy-weight, --force-weight, --denoising-pos-weight (the loop
    writes the decayed denoising weight); task_mean / task_std default to the model's.  bucket_kwargs: those of
    BucketedTrainStep.  A reducer is refused."""
    _refuse_reducer(optimizer, "dens_train_step")
    dev = next(model.parameters()).device
    task_mean = getattr(model, "task_mean", None) if task_mean is None else task_mean
    task_std = getattr(model, "task_std", None) if task_std is None else task_std
    if task_mean is None or task_std is None:
        raise ValueError("dens_train_step: the model carries no task_mean / task_std; pass them")
    loss = DeNSMeteredLoss(task_mean, task_std, denoising_pos_std, energy_weight, force_weight, denoising_pos_weight, device=dev)
    step = DeNSTrainStep(model, optimizer, loss, radius, denoising_pos_std, prob, corrupt_ratio, seed=seed, **bucket_kwargs)
    step.optimizer = optimizer
    return step


def is2rs_train_step(model, optimizer, radius, max_num_neighbors, target_mean, target_std, positions_mean, positions_std,
                     auxiliary_task_weight, energy_weight=1.0, threshold=0.02, interpolate=True, seed=0, **bucket_kwargs):
    """The is2rs.IS2RSTrainStep of `train_one_epoch_is2rs`, its loss an IS2RSMeteredLoss, built with total_steps=None: the loop
    writes the decayed auxiliary weight.  auxiliary_task_weight: the trainer's w0 (`.w0` of the step); `.lr_initial`: the
    optimizer's lr at construction.  bucket_kwargs: those of BucketedTrainStep (edges="batch" among them).  A reducer and a model
    without the auxiliary head (use_auxiliary_task=True) are refused."""
    _refuse_reducer(optimizer, "is2rs_train_step")
    if not getattr(model, "use_auxiliary_task", False):
        raise ValueError("is2rs_train_step: the model has no IS2RS head (use_auxiliary_task=True); train it with oc20_train_step")
    dev = next(model.parameters()).device
    loss = IS2RSMeteredLoss(target_mean, target_std, positions_mean, positions_std, auxiliary_task_weight,
                            energy_weight=energy_weight, threshold=threshold, device=dev)
    step = IS2RSTrainStep(model, optimizer, loss, radius, max_num_neighbors, interpolate=interpolate, seed=seed, total_steps=None,
                          auxiliary_task_weight=float(auxiliary_task_weight), **bucket_kwargs)
    step.optimizer = optimizer
    step.lr_initial = float(optimizer.param_groups[0]["lr"])
    return step


def _check_metered(step, cls, loss_cls, name):
    if not isinstance(step, cls) or not isinstance(getattr(step, "loss", None), loss_cls):
        raise ValueError("train_one_epoch_%s needs the step of %s_train_step" % (name, name))


def _metered_epoch(step, loader, before, due, line, log):
    """reset, one step per batch, a read-back per log line and one at the end; returns the averages"""
    step.model.train()
    meters = step.loss.meters
    meters.reset()
    length = len(loader) if hasattr(loader, "__len__") else None
    start = time.perf_counter()
    for k, batch in enumerate(loader):
        before(k)
        step.step(batch)
        if log is not None and due(k, length):
            log(line(k, length, meters.averages(), 1e3 * (time.perf_counter() - start) / (k + 1)))
    return meters.averages()


def train_one_epoch_dens(step, loader, epoch, epochs, denoising_pos_weight, linear_decay=False, print_freq=100, log=None):
    """(mae_metrics, loss_metrics) of main_md17_dens.train_one_epoch [ref: main_md17_dens.py:349-450], each {"energy", "force",
    "denoising_pos"} of evaluate.Average: the losses (L2MAE on the normalised targets) weighted by the molecules, the
    uncorrupted and the corrupted atoms of each step, the MAEs in real units (forces and noise averaged over x, y, z) likewise.
    A step without uncorrupted (corrupted) atoms leaves the force (denoising) meters as they are; a meter that never moved
    has count 0 and avg NaN.  Before the epoch the denoising weight `dens_denoising_pos_weight(denoising_pos_weight, epoch,
    epochs, linear_decay)` goes to the loss's device word (:372-377).  step: dens_train_step(...); loader: batch mappings with
    pos, z, batch, y, dy[, num_graphs] on the model's device; log: a callable taking one line, called at step k when
    k % print_freq == 0 and at the last step."""
    _check_metered(step, DeNSTrainStep, DeNSMeteredLoss, "dens")
    w = dens_denoising_pos_weight(denoising_pos_weight, epoch, epochs, linear_decay)
    step.loss.set_weights(denoising_pos_weight=w)

    def line(k, length, a, ms):
        return ("Epoch: [%d][%d/%s] \tloss_e: %.5f, loss_f: %.5f, loss_denoising_pos: %.5f, e_MAE: %.5f, f_MAE: %.5f, "
                "denoising_pos_MAE: %.5f, time/step=%.0fms, lr=%.2e, denoising_pos_weight=%.2e"
                % (epoch, k, length if length is not None else "?", a["loss_energy"].avg, a["loss_force"].avg,
                   a["loss_denoising_pos"].avg, a["mae_energy"].avg, a["mae_force"].avg, a["mae_denoising_pos"].avg, ms,
                   step.optimizer.param_groups[0]["lr"], w))
    a = _metered_epoch(step, loader, lambda k: None, lambda k, n: k % print_freq == 0 or (n is not None and k == n - 1),
                       line, log)
    parts = ("energy", "force", "denoising_pos")
    return {p: a["mae_" + p] for p in parts}, {p: a["loss_" + p] for p in parts}


def train_one_epoch_is2rs(step, loader, lr_lambda=None, total_steps=None, auxiliary_task_weight=None, print_freq=100, log=None,
                          lr_initial=None):
    """{name: evaluate.Average} of IS2RS_METERS for one epoch of the IS2RE + IS2RS trainer [ref: energy_trainer_v2.py:240-317]:
    "loss" (the returned total), "energy_mae", "energy_mse", "energy_within_threshold" -- each the plain mean of the steps'
    figures, as avg_metric_dict keeps them -- and "pos_mae", weighted by the free atoms.  Before step k of the instance
    (`step.steps`, counted over epochs) the loop writes param_group["lr"] = lr_initial * lr_lambda(k) (as train_one_epoch_oc20;
    lr_initial: the step's `.lr_initial` by default) and, with total_steps, the auxiliary weight
    is2rs.auxiliary_task_weight(w0, k + 1, total_steps) (the reference's self.step is 1-based, :254, :468; w0: the step's
    `.w0` by default).  step: is2rs_train_step(...) -- a step that schedules the weight itself (total_steps set) is refused.
    log: a callable taking one line, called when the 1-based step is a multiple of print_freq, and at the epoch's first and
    last step (:296-317); the line holds the running averages, not the step's own figures."""
    _check_metered(step, IS2RSTrainStep, IS2RSMeteredLoss, "is2rs")
    if step.total_steps is not None:
        raise ValueError("train_one_epoch_is2rs: the step decays the auxiliary weight itself (total_steps=%d); build it with "
                         "is2rs_train_step (total_steps=None): the loop owns the schedule" % step.total_steps)
    lr0 = float(lr_initial if lr_initial is not None else getattr(step, "lr_initial", step.optimizer.param_groups[0]["lr"]))
    w0 = step.w0 if auxiliary_task_weight is None else auxiliary_task_weight
    if total_steps is not None and w0 is None:
        raise ValueError("train_one_epoch_is2rs: no auxiliary_task_weight to decay")
    aux = [float(step.loss._w_host[1])]

    def before(k):
        if lr_lambda is not None:
            lr = lr0 * lr_lambda(step.steps)
            for g in step.optimizer.param_groups:
                g["lr"] = lr
        if total_steps is not None:
            aux[0] = is2rs.auxiliary_task_weight(w0, step.steps + 1, total_steps)
            step.loss.set_weights(auxiliary_task_weight=aux[0])

    def line(k, length, a, ms):
        parts = ["%s: %.2e" % (n, a[n].avg) for n in ("energy_mae", "energy_mse", "energy_within_threshold", "loss")]
        parts += ["lr: %.2e" % step.optimizer.param_groups[0]["lr"], "step: %d" % step.steps, "aux_weight: %.2e" % aux[0]]
        return ", ".join(parts)
    return _metered_epoch(step, loader, before,
                          lambda k, n: step.steps % print_freq == 0 or k == 0 or (n is not None and k == n - 1), line, log)


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


def dens_denoising_pos_weight(denoising_pos_weight, epoch, epochs, linear_decay=True):
    """The denoising weight of epoch `epoch` (from 0) [ref: main_md17_dens.py:372-377]: with --use-denoising-pos-weight-linear-
    decay w (1 - min(1, epoch / epochs)), a linear decay to 0 over the run; otherwise w."""
    w = float(denoising_pos_weight)
    if not linear_decay:
        return w
    return w * (1 - min(1.0, ((epoch + 0.0) / epochs)))


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
