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
search runs.  Data-parallel evaluation stays eager.

The OC20 PREDICTION pass [ref: oc20/trainer/energy_trainer_v2.py:134-225 predict, base_trainer_oc20.py:707-756 save_results] is
the same step with another tail: instead of folding a batch into a meter, one launch (eqf_predict_append, csrc/predict.hip)
appends its denormalised energies, its ids and -- write_pos -- the predicted relaxed positions to a `PredictionSink` on the
device.  The launch finds the sink through a descriptor in device memory that holds the cursors, the capacities and the
buffers' addresses, so a replayed graph appends behind the previous batch and keeps working after the host has grown the
buffers.  `predict_oc20` is the loop (one read-back per pass), `save_results` writes the reference's npz."""
import collections
import ctypes
import functools

import torch

from . import ops
from .capture import DEFAULT_EDGE_STEP, DEFAULT_NODE_STEP, _BucketedStep
from .lib import call

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


# ------------------------------------------------------------------------------------------------------------------ prediction
# PredictionSink.desc, in this order (include/equiformer_hip.h eqf_predict_append)
DESC = ("graph_cursor", "atom_cursor", "graph_capacity", "atom_capacity", "dropped_graphs", "dropped_atoms", "energy_out",
        "sid_out", "natoms_out", "pos_out")
_GRAPH_BUFFERS = (("energy", torch.float32), ("sid", torch.int64), ("natoms", torch.int32))


def grown_capacity(capacity, needed):
    """The capacity a sink buffer of `capacity` rows has after `needed` rows were asked of it: unchanged while they fit, else
    max(2 x capacity, needed).  A pure host function."""
    capacity, needed = int(capacity), int(needed)
    return capacity if needed <= capacity else max(2 * capacity, needed)


def _three(v, default):
    """a per-component normalisation constant: None (the default), a number (all three) or three numbers"""
    if v is None:
        return (float(default),) * 3
    if torch.is_tensor(v):
        v = v.detach().cpu().reshape(-1).tolist()
    if isinstance(v, (int, float)):
        return (float(v),) * 3
    v = tuple(float(x) for x in v)
    if len(v) == 1:
        return v * 3
    if len(v) != 3:
        raise ValueError("a positions normalizer has one or three components, got %d" % len(v))
    return v


class PredictionSink:
    """sink = PredictionSink(device, graphs=4096, atoms=262144, write_pos=False)
       sink.reserve(B, n_atoms)                      # every batch, on the host, from shapes: grows the buffers when needed
       sink.append(energy, sid, mol_ptr, B[, pos, delta, tags], ...)   # every batch: one launch, nothing read back
       out = sink.read()                             # once per pass: {"energy", "sid", "natoms", "pos"} on the host

    The results of a prediction pass on the device: `energy` fp32 / `sid` int64 / `natoms` int32 per structure, `pos` fp32
    [atoms, 3] (write_pos only), and `.desc`, the `DESC` int64 words the launches read: the two cursors, the capacities, two
    counters of dropped rows and the ADDRESSES of the four buffers.  A launch appends at the cursors and advances them on the
    device, so a captured launch needs no host write to land behind its predecessor.  `reserve` is the host's share: it counts
    the rows it is told about (no synchronisation) and, when they would not fit, allocates max(2 x, needed), copies the prefix
    on the stream and rewrites addresses and capacities in `.desc` through a pinned buffer -- graphs captured before see the
    new buffers, because they read the addresses when they run.  (The pinned buffer is reused as capture._DeviceWord's is:
    inside a step the graph build's read-back follows the write; an event makes a second growth wait for the first copy
    where no read-back stands between them.)  A batch appended without `reserve` that does not fit is dropped whole by the
    launch, and `read` raises.  Appends are ordered by the stream they are enqueued on; use one stream."""

    def __init__(self, device=None, graphs=4096, atoms=262144, write_pos=False):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ops.HipOnlyError("the prediction sink lives on MI355X only (got device %s); there is no CPU fallback" % dev)
        self.device, self.write_pos = dev, bool(write_pos)
        self.graph_capacity, self.atom_capacity = max(0, int(graphs)), max(0, int(atoms)) if write_pos else 0
        for name, dtype in _GRAPH_BUFFERS:
            setattr(self, name, torch.empty(self.graph_capacity, dtype=dtype, device=dev))
        self.pos = torch.empty((self.atom_capacity, 3), dtype=torch.float32, device=dev) if write_pos else None
        self.graphs = self.atoms = 0  # what reserve() has been told since the last reset: the cursors, known without a read-back
        self._host = torch.zeros(len(DESC), dtype=torch.int64).pin_memory()
        self._sent = None
        # (a pageable copy: the host waits for it, nothing of `words` is reused)
        self.desc = torch.tensor(self._words(), dtype=torch.int64, device=dev)

    def _words(self):
        """the host's share of the descriptor (the cursors and counters, zero here, belong to the device)"""
        return [0, 0, self.graph_capacity, self.atom_capacity, 0, 0, self.energy.data_ptr(), self.sid.data_ptr(),
                self.natoms.data_ptr(), 0 if self.pos is None else self.pos.data_ptr()]

    def reset(self):
        """an empty sink (two fills on the current stream: ordered with the appends, no synchronisation)"""
        self.desc[0:2].zero_()
        self.desc[4:6].zero_()
        self.graphs = self.atoms = 0

    def reserve(self, n_graphs, n_atoms=0):
        """Room for one more batch of n_graphs structures and n_atoms atoms (counted only by a write_pos sink), before its
        launch is enqueued or its graph replayed.  Host arithmetic on shapes; growth enqueues copies, it does not wait."""
        g = self.graphs + int(n_graphs)
        a = self.atoms + (int(n_atoms) if self.write_pos else 0)
        gcap, acap = grown_capacity(self.graph_capacity, g), grown_capacity(self.atom_capacity, a)
        if (gcap, acap) != (self.graph_capacity, self.atom_capacity):
            self._grow(gcap, acap)
        self.graphs, self.atoms = g, a

    def _grow(self, gcap, acap):
        with torch.no_grad():
            if gcap != self.graph_capacity:
                used = min(self.graphs, self.graph_capacity)
                for name, dtype in _GRAPH_BUFFERS:
                    old, new = getattr(self, name), torch.empty(gcap, dtype=dtype, device=self.device)
                    new[:used].copy_(old[:used])
                    setattr(self, name, new)
                self.graph_capacity = gcap
            if acap != self.atom_capacity:
                used = min(self.atoms, self.atom_capacity)
                new = torch.empty((acap, 3), dtype=torch.float32, device=self.device)
                new[:used].copy_(self.pos[:used])
                self.pos, self.atom_capacity = new, acap
            if self._sent is not None:
                self._sent.synchronize()  # (the previous growth's copy has read the pinned buffer)
            self._host.copy_(torch.tensor(self._words(), dtype=torch.int64))
            # capacities and addresses only: the cursors and the counters are the device's
            self.desc[2:4].copy_(self._host[2:4], non_blocking=True)
            self.desc[6:10].copy_(self._host[6:10], non_blocking=True)
            self._sent = torch.cuda.Event()
            self._sent.record()

    def append(self, energy, sid, mol_ptr, n_graphs, pos=None, delta=None, tags=None, target_mean=0.0, target_std=1.0,
               positions_mean=None, positions_std=None):
        """One launch (include/equiformer_hip.h eqf_predict_append): the first n_graphs rows of energy ([rows] or [rows, 1]
        fp32, normalised) denormalised with target_mean / target_std, sid [>= n_graphs] int64 and the atom counts from mol_ptr
        [>= n_graphs + 1] int32; with pos / delta [N, 3] fp32 and tags [N] int32 / int64 also the rows mol_ptr[0] <=
        i < mol_ptr[n_graphs] of pos, moved by delta * positions_std + positions_mean where tags > 0.  Enqueue-only."""
        B = int(n_graphs)
        energy = Meter._f32(energy).reshape(-1)
        sid, mol_ptr = sid.detach(), mol_ptr.detach()
        for t in (energy, sid, mol_ptr, pos, delta):
            if t is not None and not t.is_cuda:
                raise ops.HipOnlyError("the prediction pass runs on MI355X only (got a %s tensor); there is no CPU fallback" % t.device)
        if sid.dtype != torch.int64 or mol_ptr.dtype != torch.int32 or not sid.is_contiguous() or not mol_ptr.is_contiguous():
            raise ValueError("predict_append: sid is contiguous int64 and mol_ptr contiguous int32, got %s / %s" % (sid.dtype, mol_ptr.dtype))
        if B < 0 or energy.numel() < B or sid.numel() < B or mol_ptr.numel() < B + 1:
            raise ValueError("predict_append: energy %s, sid %s, mol_ptr %s, n_graphs %d"
                             % (tuple(energy.shape), tuple(sid.shape), tuple(mol_ptr.shape), B))
        is64 = 0
        if pos is not None:
            if not self.write_pos:
                raise ValueError("predict_append: positions handed to a sink built without write_pos")
            if delta is None or tags is None:
                raise ValueError("predict_append: pos needs delta and tags")
            pos, delta = Meter._f32(pos), Meter._f32(delta)
            N = pos.shape[0]
            if tuple(pos.shape) != (N, 3) or tuple(delta.shape) != (N, 3):
                raise ValueError("predict_append: pos %s, delta %s" % (tuple(pos.shape), tuple(delta.shape)))
            tags, is64 = ops._tags_arg(tags, N, "predict_append")
        elif delta is not None or tags is not None:
            raise ValueError("predict_append: delta / tags without pos")
        pm, ps = _three(positions_mean, 0.0), _three(positions_std, 1.0)
        addr = lambda t: None if t is None else ctypes.c_void_p(ops._nonnull(t))  # noqa: E731
        call("eqf_predict_append", addr(energy), addr(sid), addr(mol_ptr), B, addr(pos), addr(delta), addr(tags), is64,
             float(target_mean), float(target_std), pm[0], pm[1], pm[2], ps[0], ps[1], ps[2],
             ctypes.c_void_p(self.desc.data_ptr()), ops._stream())

    def read(self):
        """The one host read-back of a pass: {"energy" fp32 [G], "sid" int64 [G], "natoms" int32 [G], "pos" fp32 [A, 3] or
        None}, G structures and A atoms as the device cursors count them.  Raises when a launch dropped a batch (naming the
        capacity that was needed) or appended rows `reserve` was not told about."""
        def pinned(shape, dtype):
            return torch.empty(shape, dtype=dtype, pin_memory=bool(shape[0]))
        n_g, n_a = min(self.graphs, self.graph_capacity), min(self.atoms, self.atom_capacity)
        desc = pinned((len(DESC),), torch.int64)
        desc.copy_(self.desc, non_blocking=True)
        host = {}
        for name, dtype in _GRAPH_BUFFERS:
            host[name] = pinned((n_g,), dtype)
            host[name].copy_(getattr(self, name)[:n_g], non_blocking=True)
        if self.write_pos:
            host["pos"] = pinned((n_a, 3), torch.float32)
            host["pos"].copy_(self.pos[:n_a], non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        d = dict(zip(DESC, desc.tolist()))
        if d["dropped_graphs"] or d["dropped_atoms"]:
            raise RuntimeError("the prediction sink dropped %d structures / %d atoms: it needed a capacity of %d structures and %d "
                               "atoms and has %d and %d (call reserve() before every append, or build it larger)"
                               % (d["dropped_graphs"], d["dropped_atoms"], d["graph_cursor"] + d["dropped_graphs"],
                                  d["atom_cursor"] + d["dropped_atoms"], d["graph_capacity"], d["atom_capacity"]))
        G, A = d["graph_cursor"], d["atom_cursor"]
        if G > n_g or A > n_a:
            raise RuntimeError("the prediction sink holds %d structures / %d atoms, reserve() was told of %d / %d"
                               % (G, A, self.graphs, self.atoms))
        out = {name: host[name][:G] for name, _ in _GRAPH_BUFFERS}
        out["pos"] = host["pos"][:A] if self.write_pos else None
        return out


class OC20PredictStep(BucketedEvalStep):
    """The BucketedEvalStep of the prediction pass: `sid` travels as a per-structure target and `tags` as a per-node one, the
    pre-check refuses a batch without `sid` and tells the sink the batch's sizes (from shapes: no synchronisation) before the
    graph build, and `predict` ends in the sink's append -- inside the captured region."""

    def __init__(self, predict, radius, sink, write_pos=False, **bucket_kwargs):
        super().__init__(predict, radius, None, graph_targets=("sid",), node_targets=("tags",), **bucket_kwargs)
        self.sink, self.write_pos = sink, bool(write_pos)

    def _check(self, batch):
        super()._check(batch)
        if "sid" not in batch or batch["sid"] is None:
            raise ValueError("the prediction pass needs every batch's `sid` (the ids the predictions are filed under): sid missing")
        self.sink.reserve(batch["sid"].shape[0], batch["pos"].shape[0])


def oc20_predict_step(model, radius, target_mean=0.0, target_std=1.0, positions_mean=None, positions_std=None, write_pos=False,
                      sink=None, **bucket_kwargs):
    """The step of `predict_oc20` (keep it between passes: its graphs are reused).  target_mean / target_std: the trainer's
    target normalizer (0, 1 without normalize_labels); positions_mean / positions_std: its positions normalizer, a number or
    three (None: 0 / 1, normalize_positions unset).  write_pos needs a model with the IS2RS head (use_auxiliary_task).  sink: a
    PredictionSink of one's own (its write_pos must cover the step's).  bucket_kwargs as oc20_eval_step, edges="batch" included."""
    aux = bool(getattr(model, "use_auxiliary_task", False))
    if write_pos and not aux:
        raise ValueError("write_pos needs the IS2RS head: %s was built without use_auxiliary_task" % type(model).__name__)
    write_pos = bool(write_pos)
    if sink is None:
        sink = PredictionSink(next(model.parameters()).device, write_pos=write_pos)
    norm = dict(target_mean=float(target_mean), target_std=float(target_std), positions_mean=_three(positions_mean, 0.0),
                positions_std=_three(positions_std, 1.0))

    def predict(g, v):
        out = model(v, graph=g, offsets=v.offsets)
        energy, delta = out if isinstance(out, tuple) else (out, None)
        sid = v.sid if v.sid.dtype == torch.int64 else v.sid.to(torch.int64)
        if write_pos:
            sink.append(energy, sid, g.mol_ptr, v.B, v.pos, delta, v.tags, **norm)
        else:
            sink.append(energy, sid, g.mol_ptr, v.B, **norm)
        return energy, delta if write_pos else None
    return OC20PredictStep(predict, radius, sink, write_pos, model=model, **bucket_kwargs)


def split_positions(pos, natoms, sids):
    """{str(sid): pos rows [natoms, 3]} of the concatenated positions [ref: energy_trainer_v2.py:200-204]; an id met twice
    keeps its last rows, as the reference's dict does.  A pure host function."""
    natoms = [int(n) for n in natoms]
    if len(natoms) != len(sids) or sum(natoms) != pos.shape[0]:
        raise ValueError("split_positions: %d ids, %d atom counts that sum to %d, %d rows"
                         % (len(sids), len(natoms), sum(natoms), pos.shape[0]))
    return {str(int(s)): p for s, p in zip(sids, torch.split(pos, natoms))}


def predictions_of(read, write_pos=False):
    """What the reference's predict returns, from PredictionSink.read(): {"id": [str], "energy": [float]} in loader order,
    plus "pos": {str(sid): tensor [natoms, 3]} with write_pos.  A pure host function."""
    sids = read["sid"].tolist()
    out = {"id": [str(s) for s in sids], "energy": read["energy"].tolist()}
    if write_pos:
        if read.get("pos") is None:
            raise ValueError("write_pos: the sink holds no positions")
        out["pos"] = split_positions(read["pos"], read["natoms"].tolist(), sids)
    return out


def predict_oc20(model, loader, radius, step=None, write_pos=False, **kw):
    """The OC20 trainer's predict [ref: energy_trainer_v2.py:134-225], per_image=True, one process: {"id": [str(sid)],
    "energy": [float]} in loader order (denormalised: fp32 `energy * target_std + target_mean`), and with write_pos also "pos":
    {str(sid): [natoms, 3]}, the batch's own `pos` with `delta * positions_std + positions_mean` added on the free atoms (tags
    > 0).  loader: batch mappings with pos, atomic_numbers, batch, cell, tags, sid [B] (and the edge fields with edges="batch").
    kw: the normalizers and bucket arguments of `oc20_predict_step`.  One read-back at the end (plus the graph build's own per
    batch).  For the EMA weights pass the EMA module (`opt.ema_module(model)`) as the model: nothing is stored or restored."""
    model.eval()
    if step is None:
        step = oc20_predict_step(model, radius, write_pos=write_pos, **kw)
    elif write_pos and not step.write_pos:
        raise ValueError("predict_oc20: write_pos with a step that was built without it")
    step.sink.reset()
    for batch in loader:
        step.step(batch)
    return predictions_of(step.sink.read(), write_pos)


def save_results(predictions, path):
    """The results file of the reference for one process [ref: base_trainer_oc20.py:707-756, keys=["energy"]]: an npz with
    `ids` and `energy`, ids made unique with `np.unique(ids, return_index=True)` (sorted as strings, the first occurrence
    kept) and the energies reordered alike.  Returns what was written."""
    import numpy as np
    _, idx = np.unique(predictions["id"], return_index=True)
    results = {"ids": np.array(predictions["id"])[idx], "energy": np.array(predictions["energy"])[idx]}
    np.savez_compressed(path, **results)
    return results
