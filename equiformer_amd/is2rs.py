"""The IS2RE + IS2RS training step around `GraphAttentionTransformerOC20(use_auxiliary_task=True)`: the relaxed energy plus,
through the auxiliary head, every free atom's displacement to its relaxed position -- device-side perturbation, one fused loss,
and the step captured in a HIP graph per shape bucket.
[ref: oc20/trainer/base_trainer_v2.py:81-126 interpolate_init_relaxed_pos, oc20/trainer/energy_trainer_v2.py:413-442
_compute_loss, :445-459 _compute_metrics, :462-470 _compute_auxiliary_task_weight]

What runs where in a step of `IS2RSTrainStep`:
  * OUTSIDE the capture: the perturbation (ops.is2rs_perturb, one launch, seed by value).  It moves atoms, so it has to precede
    the periodic radius graph, whose size is read back on the host (capture.py).  The noise differs every step, so the edge
    count does too: the step is the case `BucketedTrainStep` was built for.  The decayed auxiliary weight of the step goes out
    here as well (pinned buffer, asynchronous copy into the loss's device word).
  * INSIDE the capture: the model, the loss (ops.is2rs_loss: one launch forward, one backward, no boolean indexing, no
    `.item()`), the backward and the fused AdamW.  The two loss weights are device words: a by-value weight would be frozen
    into the graph.  The metrics land in `IS2RSLoss.stats`, a device buffer at one address for every bucket; read it when a log
    line is due, not every step.
Not here: data-parallel steps (a reducer is refused, as everywhere in capture.py), the `mse` / `l2mae` losses (no shipped _aux
configuration uses them), and the OCP trainer around the step (loaders, EMA, evaluation, checkpoints)."""
import torch

from . import ops
from .capture import BucketedTrainStep, _MirrorsBucketed, _refuse_reducer, given_edge_fields
from .droppath import step_seed  # noqa: F401  (re-exported: the seed of step k)

STATS = ("loss_e", "loss_aux", "n_free", "energy_mae", "energy_mse", "energy_within_threshold", "pos_mae", "unused")


def auxiliary_task_weight(w0, step, total_steps):
    """The auxiliary weight of `step` (energy_trainer_v2.py:462-470): linear decay from w0 to 1 over total_steps, constant from
    there on; a w0 <= 1 stays as it is.  A pure host function."""
    w0 = float(w0)
    return w0 - max(0.0, w0 - 1.0) * min(1.0, (step + 0.0) / total_steps)


def interpolate_init_relaxed_pos(data, seed=None, p_perturb=0.5, f_min=0.0, noise_std=0.3):
    """The reference's function of this name (base_trainer_v2.py:81-126), one launch: with probability p_perturb per structure,
    its free atoms (tags > 0) move to `pos * f + (1 - f) * pos_relaxed + noise`, f uniform in [f_min, 1) per atom, noise
    N(0, noise_std^2) per component.  Sets `pos` (a new tensor: the caller's is not written), `interpolate_factor` [N],
    `noise_vec` [N, 3] (both filled on every row) and `perturbed` [N] bool (the structure's draw, per atom: the atoms that moved
    are `perturbed & (tags > 0)`) on `data` (which has pos, pos_relaxed, tags, batch on the GPU) and returns it.  seed: the
    64-bit seed of this call's draws -- the same seed gives the same bits; None draws one from torch's CPU generator (the
    reference's behaviour: a fresh perturbation per call)."""
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    batch = data.batch
    if batch.is_cuda and batch.dtype == torch.int64:
        batch = batch.to(torch.int32)
    pos, factor, noise_vec, selected = ops.is2rs_perturb(
        data.pos.detach().to(torch.float32), data.pos_relaxed.to(torch.float32), data.tags, batch, p_perturb, f_min, noise_std,
        seed)
    data.pos, data.interpolate_factor, data.noise_vec, data.perturbed = pos, factor, noise_vec, selected
    return data


class IS2RSLoss:
    """loss = IS2RSLoss(target_mean, target_std, positions_mean, positions_std, auxiliary_task_weight)
       l = loss(pred_y, pred_pos, data)       # data: y (relaxed energy), pos (as the model saw it), pos_relaxed, tags

    energy_weight * MAE(pred_y, (y - target_mean) / target_std) + auxiliary_task_weight * MAE over the free atoms (tags > 0) of
    (pred_pos, ((pos_relaxed - pos) - positions_mean) / positions_std); positions_mean / positions_std: a number or three (per
    component).  Without a free atom the auxiliary term adds an exact 0.  `.stats`: 8 floats on the device, `STATS` names them
    -- the two losses, the free atoms, the evaluator's three energy figures in the target's units (threshold: that of
    energy_within_threshold) and the position MAE in Angstrom of the last call.  `.weights`: {energy, auxiliary} on the device."""

    def __init__(self, target_mean, target_std, positions_mean, positions_std, auxiliary_task_weight, energy_weight=1.0,
                 threshold=0.02, device=None):
        self.target_mean, self.target_std, self.threshold = float(target_mean), float(target_std), float(threshold)
        self.positions_mean, self.positions_std = ops._three(positions_mean), ops._three(positions_std)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ops.HipOnlyError("the IS2RS loss runs on MI355X only (got device %s); there is no CPU fallback" % dev)
        self.stats = torch.zeros(8, dtype=torch.float32, device=dev)
        self.weights = torch.zeros(2, dtype=torch.float32, device=dev)
        self._w_host = torch.zeros(2, dtype=torch.float32).pin_memory()
        self.set_weights(energy_weight, auxiliary_task_weight)

    def set_weights(self, energy_weight=None, auxiliary_task_weight=None):
        """Write the device words (None keeps a weight): pinned buffer, asynchronous copy, no synchronisation -- every later
        call and every later replay of a captured step sees the new values.  (A step's graph build reads back on the host,
        so the copy has landed before the next call here can touch the pinned words.)"""
        for i, w in enumerate((energy_weight, auxiliary_task_weight)):
            if w is not None:
                self._w_host[i] = float(w)
        self.weights.copy_(self._w_host, non_blocking=True)

    def __call__(self, pred_y, pred_pos, data, row_mask=None, num_graphs=None):
        """row_mask: [N] fp32, 1 real / 0 phantom (`view.node_mask` of a padded batch); num_graphs: the real structures when
        `data.y` carries the phantom structure's row as well (`view.B`)."""
        y = data.y if num_graphs is None else data.y[:num_graphs]
        return ops.is2rs_loss(pred_y, pred_pos, y, data.pos, data.pos_relaxed, data.tags, self.weights, self.target_mean,
                              self.target_std, self.positions_mean, self.positions_std, threshold=self.threshold,
                              row_mask=row_mask, stats_out=self.stats)


class IS2RSTrainStep(_MirrorsBucketed):
    """ts = IS2RSTrainStep(model, optimizer, loss, radius, max_num_neighbors, interpolate=True, seed=0, total_steps=None,
                           auxiliary_task_weight=None, **bucket_kwargs)
       l = ts.step(batch)   # batch: mapping with pos, pos_relaxed [N, 3], atomic_numbers, tags [N], batch [N] (ascending),
                            # cell [B, 3, 3], y [B] (the relaxed energy), num_graphs

    Step k perturbs the batch with the seed `step_seed(seed, k)` (interpolate=True: the `_aux_interpolation` configurations;
    probability 0.5, factor from 0, noise 0.3 A: the reference's constants) -- an eager loop that calls
    interpolate_init_relaxed_pos(..., seed=step_seed(seed, k)) sees the same atoms move to the same places; torch's global
    generator is not touched, the caller's `pos` is not written.  With `total_steps` the loss's auxiliary device word is set to
    `auxiliary_task_weight(w0, k, total_steps)` before the step, w0 = the constructor's `auxiliary_task_weight` (default: the
    weight `loss` holds at construction).  The perturbed pos, y and the node targets tags, pos_relaxed then go to a periodic
    `BucketedTrainStep` (bucket_kwargs: min_eager, max_graphs, node_step, edge_step, edges -- "batch": the batch's own edge_index,
    cell_offsets, neighbors travel with it and the perturbation still comes first --, drop_path_seed -- default `seed`: step k of
    a model with drop_path_rate > 0, out_drop > 0 (the 100k recipe) or proj_drop > 0 drops what an eager step under
    `droppath.device_draws(step_seed(seed, k))` drops) whose
    forward_loss is
    `model(view, graph=g, offsets=view.offsets)` and `loss(E[:view.B], vectors, view, row_mask=view.node_mask,
    num_graphs=view.B)`.  The phantom rows of a padded batch have tag 0 and stay out of the loss through the row mask as well.
    model: an OC20 model with use_auxiliary_task=True (either head); optimizer: a FlatAdamW without a reducer.  `.last`: the
    perturbed batch of the latest step; `.bucketed`: the BucketedTrainStep (its counters are mirrored here)."""

    NODE_TARGETS = ("tags", "pos_relaxed")

    def __init__(self, model, optimizer, loss, radius, max_num_neighbors, interpolate=True, seed=0, total_steps=None,
                 auxiliary_task_weight=None, **bucket_kwargs):
        _refuse_reducer(optimizer, "IS2RSTrainStep")
        if not getattr(model, "use_auxiliary_task", False):
            raise ValueError("IS2RSTrainStep: the model has no IS2RS head (use_auxiliary_task=True)")
        self.model, self.loss = model, loss
        self.interpolate, self.seed = bool(interpolate), int(seed)
        self.total_steps = None if total_steps is None else int(total_steps)
        if auxiliary_task_weight is None and self.total_steps is not None:
            auxiliary_task_weight = float(loss._w_host[1])
        self.w0 = auxiliary_task_weight
        self.steps = 0
        self.last = None
        bucket_kwargs.setdefault("drop_path_seed", self.seed)  # (its own stream of the seed: the kernels separate them by tag)
        self.bucketed = BucketedTrainStep(optimizer, self._forward_loss, radius, graph_targets=("y",),
                                          node_targets=self.NODE_TARGETS, max_num_neighbors=max_num_neighbors, **bucket_kwargs)

    def _forward_loss(self, g, view):
        out = self.model(view, graph=g, offsets=view.offsets)
        return self.loss(out[0][:view.B], out[1], view, row_mask=view.node_mask, num_graphs=view.B)

    def step(self, batch):
        k = self.steps
        self.steps += 1
        d = {n: batch[n] for n in ("pos", "pos_relaxed", "atomic_numbers", "tags", "batch", "cell", "y")}
        if self.interpolate:
            b = batch["batch"]
            b32 = b.to(torch.int32) if b.dtype != torch.int32 else b
            d["pos"], d["interpolate_factor"], d["noise_vec"], d["perturbed"] = ops.is2rs_perturb(
                batch["pos"].to(torch.float32), batch["pos_relaxed"].to(torch.float32), batch["tags"], b32,
                seed=step_seed(self.seed, k))
        if self.total_steps is not None:
            self.loss.set_weights(auxiliary_task_weight=auxiliary_task_weight(self.w0, k, self.total_steps))
        if "num_graphs" in batch:
            d["num_graphs"] = batch["num_graphs"]
        if self.bucketed.edges == "batch":  # (the zero-length test of the given edges then sees the moved atoms, as the reference's)
            for n in given_edge_fields(batch):
                d[n] = batch[n]
        self.last = d
        return self.bucketed.step(d)
