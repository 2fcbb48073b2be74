"""Evaluation loops on the HIP path: the forward (and, for the MD17 models, the first-order force pass) captured in a HIP graph
per shape bucket, the running metrics kept on the device.
[ref: engine.py:110-141 evaluate (QM9), main_md17.py:425-480 evaluate, oc20/trainer/base_trainer_v2.py:477-524 validate with
energy_trainer_v2.py:445-459 _compute_metrics]

The reference loops launch every kernel from the host and stop the GPU for two (QM9) to four (MD17) `.item()` read-backs per
batch.  Here:
  * `Meter` owns ten fp64 sums on the device; `Meter.update` is one launch (ops.metrics_accumulate) that reads nothing back, and
    `Meter.read` is the one read-back of a whole evaluation pass.  `Meter.figures` turns the sums into what each reference loop
    reports -- the reference's AverageMeter averages per-batch means weighted by the batch size, which is the ratio of the sums.
  * `BucketedEvalStep` pads every batch to its shape bucket as `capture.BucketedTrainStep` does and replays one HIP graph per
    bucket that holds `predict` and the meter update.  What stays outside the graph is the radius graph build (its edge count
    is read back on the host: one read-back per batch, as in training).  No optimizer is involved, and the captured launches
    read the parameters at their addresses: a replay sees the weights as they are then (an optimizer step or an EMA copy made in
    place between two passes is seen; parameters REPLACED by new tensors are not).
  * `evaluate_qm9`, `evaluate_md17`, `evaluate_oc20` are the three loops behind that interface.
OC20 batches with a precomputed edge list (otf_graph=False) are served with `edges="batch"` (BucketedEvalStep, oc20_eval_step and
evaluate_oc20 through their bucket_kwargs): the graph comes from EdgeGraph.edges_pbc_plan / from_edges_pbc_plan, no neighbour
search runs.  Data-parallel evaluation stays eager."""
import collections
import functools

import torch

from . import ops
from .capture import DEFAULT_EDGE_STEP, DEFAULT_NODE_STEP, _BucketedStep

# Meter.acc, in this order (include/equiformer_hip.h eqf_metrics_accumulate)
SUMS = ("graphs", "abs_norm", "abs_err", "sq_err", "within", "atoms", "force_l2", "force_abs_norm", "force_abs_err",
        "force_sq_err")

Average = collections.namedtuple("Average", "avg sum count")  # what the figures keep of the reference's AverageMeter


def _avg(total, count):
    return Average(total / count if count else float("nan"), total, count)


class Meter:
    """meter = Meter(task_mean, task_std, threshold=0.02)
       meter.update(pred_y, y, n_graphs[, pred_dy, dy, node_mask])     # every batch: one launch, nothing read back
       figures = Meter.figures(meter.read())                            # once per pass

    pred_y: the model's (normalised) energies, y: the targets in real units; pred_dy / dy likewise for forces.  `.acc`: the ten
    fp64 sums `SUMS` at one device address -- the same in every captured bucket.  Updates are ordered by the stream they are
    enqueued on; use one stream."""

    def __init__(self, task_mean, task_std, threshold=0.02, device=None):
        self.task_mean, self.task_std, self.threshold = float(task_mean), float(task_std), float(threshold)
        if not self.task_std > 0.0:
            raise ValueError("task_std must be positive, got %r" % (task_std,))
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ops.HipOnlyError("the evaluation metrics run on MI355X only (got device %s); there is no CPU fallback" % dev)
        self.acc = torch.zeros(len(SUMS), dtype=torch.float64, device=dev)

    @staticmethod
    def _f32(t):
        # (`.to` of another dtype and `.contiguous()` are enqueue-only: legal inside a capture)
        t = t.detach()
        if t.dtype != torch.float32:
            t = t.to(torch.float32)
        return t.contiguous()

    def update(self, pred_y, y, n_graphs, pred_dy=None, dy=None, node_mask=None):
        """pred_y, y: [rows] or [rows, 1] with rows >= n_graphs (a padded batch carries the phantom molecule's row); only the
        first n_graphs count.  pred_dy, dy: [N, 3]; node_mask [N]: 1.0 real, 0.0 phantom (None: all real)."""
        pred_y, y = self._f32(pred_y).reshape(-1), self._f32(y).reshape(-1)
        if pred_dy is not None:
            if dy is None:
                raise ValueError("Meter.update: pred_dy without dy")
            pred_dy, dy = self._f32(pred_dy), self._f32(dy)
            if node_mask is not None:
                node_mask = self._f32(node_mask)
        ops.metrics_accumulate(self.acc, pred_y, y, n_graphs, self.task_mean, self.task_std, self.threshold, pred_dy,
                               dy if pred_dy is not None else None, node_mask if pred_dy is not None else None)

    def reset(self):
        self.acc.zero_()  # (a fill on the current stream: ordered with the updates, no synchronisation)

    def read(self):
        """The one host read-back: {name: float} over `SUMS`."""
        return dict(zip(SUMS, self.acc.cpu().tolist()))

    @staticmethod
    def figures(sums):
        """What the reference loops report, from the raw sums (a pure host function):
          "qm9":  (mae, loss) of engine.evaluate;
          "md17": (mae_metrics, loss_metrics) of main_md17.evaluate, each {"energy": Average, "force": Average} (`.avg` as the
                  reference's AverageMeter; the force loss is the L2MAE loss, the force MAE averages over x, y, z);
          "oc20": the IS2RE evaluator's energy_mae, energy_mse, energy_within_threshold, each {"metric", "total", "numel"}.
        A count of zero gives NaN averages."""
        n, atoms = sums["graphs"], sums["atoms"]
        mae_e, loss_e = _avg(sums["abs_err"], n), _avg(sums["abs_norm"], n)
        md17 = ({"energy": mae_e, "force": Average(sums["force_abs_err"] / (3.0 * atoms) if atoms else float("nan"),
                                                   sums["force_abs_err"] / 3.0, atoms)},
                {"energy": loss_e, "force": _avg(sums["force_l2"], atoms)})
        oc20 = {k: {"metric": sums[s] / n if n else float("nan"), "total": sums[s], "numel": n}
                for k, s in (("energy_mae", "abs_err"), ("energy_mse", "sq_err"), ("energy_within_threshold", "within"))}
        return {"qm9": (mae_e.avg, loss_e.avg), "md17": md17, "oc20": oc20}


def _modules_of(fn, depth=0):
    """The torch modules a `predict` callable visibly holds: itself, the object of a bound method, the arguments of a
    functools.partial, the cells of a closure (best effort: it is what the training-mode check looks at)."""
    found = []
    if isinstance(fn, torch.nn.Module):
        return [fn]
    if depth > 2:
        return found
    if isinstance(fn, functools.partial):
        for a in (fn.func,) + tuple(fn.args) + tuple((fn.keywords or {}).values()):
            found += _modules_of(a, depth + 1)
        return found
    owner = getattr(fn, "__self__", None)
    if isinstance(owner, torch.nn.Module):
        found.append(owner)
    for cell in getattr(fn, "__closure__", None) or ():
        try:
            v = cell.cell_contents
        except ValueError:  # (an empty cell)
            continue
        if isinstance(v, torch.nn.Module):
            found.append(v)
    return found


class BucketedEvalStep(_BucketedStep):
    """es = BucketedEvalStep(predict, radius, meter=None, graph_targets=("y",), node_targets=())
       energy, forces = es.step(batch)     # batch: the mapping of BucketedTrainStep.step -- periodic (`cell`) or not

    predict(graph, view) -> (energy [B + 1(, 1)], forces [N_cap, 3] or None) on the padded batch (capture.PaddedBatch).  After
    it the step folds the batch into `meter` -- meter.update(energy, view.y, view.B, forces, view.dy, view.node_mask) -- when a
    meter is given and "y" is among the graph targets (forces: when predict returns them and "dy" is among the node targets).
    Per bucket one HIP graph holds predict + the update; buckets, `min_eager`, `max_graphs` (least recently used evicted) and
    the counters are those of BucketedTrainStep.  predict runs under no_grad; a model that needs its own autograd pass (the
    MD17 and DeNS models take a first-order force pass in eval mode) enables grad itself.  The outputs are detached inside the
    recorded region, so no autograd graph is alive when the capture ends (see capture._TrainStep._run).

    `step` returns the REAL rows (energy[:B], forces[:n_real] or None) as views of the bucket's static buffers: valid until the
    next step of that bucket.  model: the module(s) predict calls; a step with one of them (or of the modules found on
    predict itself: a bound method's object, closure cells) in training mode raises -- dropout and the second-order force pass
    are not what an evaluation captures."""

    def __init__(self, predict, radius, meter=None, graph_targets=("y",), node_targets=(), min_eager=3, max_graphs=16,
                 node_step=DEFAULT_NODE_STEP, edge_step=DEFAULT_EDGE_STEP, max_num_neighbors=1000, device=None, model=None,
                 edges="search"):
        self.predict, self.meter = predict, meter
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise ops.HipOnlyError("the evaluation step runs on MI355X only (got device %s); there is no CPU fallback" % self.device)
        mods = [] if model is None else ([model] if isinstance(model, torch.nn.Module) else list(model))
        self._models = mods + [m for m in _modules_of(predict) if all(m is not k for k in mods)]
        self._init_buckets(radius, graph_targets, node_targets, min_eager, max_graphs, node_step, edge_step, max_num_neighbors,
                           edges)

    def _check_eval(self):
        for m in self._models:
            if m.training:
                raise ValueError("BucketedEvalStep: %s is in training mode; call .eval() first" % type(m).__name__)

    def _run(self, g, view):
        with torch.no_grad():
            energy, forces = self.predict(g, view)
            # detached: nothing of an autograd graph (the force pass builds one) outlives the recorded region
            energy = energy.detach()
            forces = None if forces is None else forces.detach()
            if self.meter is not None and "y" in self.graph_targets:
                with_forces = forces is not None and "dy" in self.node_targets
                self.meter.update(energy, view.y, view.B, forces if with_forces else None,
                                  view.dy if with_forces else None, view.node_mask if with_forces else None)
        return energy, forces

    def _check(self, batch):
        self._check_eval()
        self._check_periodic(batch)
        if self.device is not None and batch["pos"].device != self.device:
            raise ValueError("BucketedEvalStep: the batch is on %s, the step on %s" % (batch["pos"].device, self.device))

    def _returned(self, out, B, n_real):
        """the real rows (a capture also holds the addresses of the parameters and of the meter's sums; its first replay is
        what shows this batch to the outputs and the meter)"""
        energy, forces = out
        return energy[:B], None if forces is None else forces[:n_real]


# ------------------------------------------------------------------------------------------------------------------ the three loops
def _loop(step, loader):
    if step.meter is None:
        raise ValueError("the evaluation drivers need a BucketedEvalStep with a meter")
    step.meter.reset()
    for batch in loader:
        step.step(batch)
    return Meter.figures(step.meter.read())


def qm9_eval_step(model, norm_factor, radius, threshold=0.02, **bucket_kwargs):
    """The BucketedEvalStep of `evaluate_qm9` (keep it between epochs: its graphs are reused).  norm_factor: (mean, std)."""
    dev = next(model.parameters()).device
    meter = Meter(float(norm_factor[0]), float(norm_factor[1]), threshold, device=dev)

    def predict(g, v):
        return model(None, v.pos, v.batch, v.z, graph=g), None
    return BucketedEvalStep(predict, radius, meter, graph_targets=("y",), model=model, **bucket_kwargs)


def evaluate_qm9(model, norm_factor, target, loader, radius, step=None, **bucket_kwargs):
    """(mae, loss) of engine.evaluate [ref: engine.py:110-141]: the MAE in the target's units and the L1 loss on the normalised
    target, both averaged over the molecules.  loader: batch mappings with pos, z, batch, y ([B], or [B, T] of which column
    `target` is taken) on the model's device.  One read-back at the end (plus the graph build's own per batch)."""
    model.eval()
    if step is None:
        step = qm9_eval_step(model, norm_factor, radius, **bucket_kwargs)

    def column(batch):
        y = batch["y"]
        return batch if y.dim() < 2 else dict(batch, y=y[:, target])
    return _loop(step, (column(b) for b in loader))["qm9"]


def md17_eval_step(model, radius, task_mean=None, task_std=None, threshold=0.02, **bucket_kwargs):
    """The BucketedEvalStep of `evaluate_md17`.  model: GraphAttentionTransformerMD17 (called with node_atom, pos, batch) or
    Equiformer_MD17_DeNS (called with the padded view as its `data`); task_mean / task_std default to the model's."""
    dev = next(model.parameters()).device
    task_mean = getattr(model, "task_mean", None) if task_mean is None else task_mean
    task_std = getattr(model, "task_std", None) if task_std is None else task_std
    if task_mean is None or task_std is None:
        raise ValueError("md17_eval_step: the model carries no task_mean / task_std; pass them")
    meter = Meter(float(task_mean), float(task_std), threshold, device=dev)
    from .nets.equiformer_md17_dens import Equiformer_MD17_DeNS
    if isinstance(model, Equiformer_MD17_DeNS):
        def predict(g, v):
            return model(v, graph=g)
    else:
        def predict(g, v):
            return model(node_atom=v.z, pos=v.pos, batch=v.batch, graph=g)
    return BucketedEvalStep(predict, radius, meter, graph_targets=("y",), node_targets=("dy",), model=model, **bucket_kwargs)


def evaluate_md17(model, loader, radius, step=None, **bucket_kwargs):
    """(mae_metrics, loss_metrics) of main_md17.evaluate [ref: main_md17.py:425-480], each {"energy": Average, "force": Average}
    with the reference's `.avg`: L2MAE losses on the normalised targets, MAEs in real units (forces averaged over x, y, z).
    loader: batch mappings with pos, z, batch, y [B] or [B, 1], dy [N, 3].  The force pass is the model's first-order one."""
    model.eval()
    if step is None:
        step = md17_eval_step(model, radius, **bucket_kwargs)
    return _loop(step, loader)["md17"]


def oc20_eval_step(model, radius, task_mean=0.0, task_std=1.0, threshold=0.02, node_targets=("tags",), **bucket_kwargs):
    """The BucketedEvalStep of `evaluate_oc20`: periodic batches (`cell`), graph built on the fly -- or, with edges="batch" among
    bucket_kwargs, from the batch's own edge_index / cell_offsets / neighbors.  task_mean / task_std: the trainer's target
    normalizer (0, 1 without normalize_labels)."""
    dev = next(model.parameters()).device
    meter = Meter(task_mean, task_std, threshold, device=dev)

    def predict(g, v):
        out = model(v, graph=g, offsets=v.offsets)
        return (out[0] if isinstance(out, tuple) else out), None  # (the auxiliary IS2RS head has no validation metric)
    return BucketedEvalStep(predict, radius, meter, graph_targets=("y",), node_targets=node_targets, model=model, **bucket_kwargs)


def evaluate_oc20(model, loader, radius, step=None, **bucket_kwargs):
    """The IS2RE metrics of the OC20 trainer's validate [ref: base_trainer_v2.py:477-524, energy_trainer_v2.py:445-459]:
    {"energy_mae", "energy_mse", "energy_within_threshold"}, each {"metric", "total", "numel"}.  loader: batch mappings with pos,
    atomic_numbers, batch, cell, tags, y (= y_relaxed) and max_num_neighbors among bucket_kwargs (the model's max_neighbors).
    For the EMA weights copy them into the model in place before the call, as the trainer does."""
    model.eval()
    if step is None:
        step = oc20_eval_step(model, radius, **bucket_kwargs)
    return _loop(step, loader)["oc20"]
