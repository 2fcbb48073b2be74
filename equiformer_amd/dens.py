"""The DeNS training step (denoising non-equilibrium structures) around `Equiformer_MD17_DeNS`: device-side corruption, one
fused loss, and the step captured in a HIP graph per shape bucket.
[ref: main_md17_dens.py:379-409 the loop body of train_one_epoch, :417-427 its MAE meters, :514-548
add_masked_gaussian_noise_to_pos]

What runs where in a step of `DeNSTrainStep`:
  * OUTSIDE the capture: the corruption (ops.dens_corrupt, one launch, seed by value).  It moves atoms, so it has to precede
    the radius graph, and the radius graph is the one part of a step whose size is read back on the host (capture.py).
    The noise differs every step, so the edge count does too: the step is the case `BucketedTrainStep` was built for.
  * INSIDE the capture: the model (forces by a create_graph backward), the loss (ops.dens_loss: one launch forward, one
    backward, no boolean indexing, no `isnan` test, no `.item()`), the second-order backward and the fused AdamW.  The three
    loss weights are device words: `DeNSLoss.set_weights` changes what the next replay multiplies by (the linear decay of
    --use-denoising-pos-weight-linear-decay), a by-value weight would be frozen into the graph.  The metrics land in
    `DeNSLoss.stats`, a device buffer at one address for every bucket; read it when a log line is due, not every step.
"""
import torch

from . import ops
from .capture import BucketedTrainStep, _MirrorsBucketed, _refuse_reducer
from .droppath import step_seed  # noqa: F401  (re-exported: the corruption seed of step k)

STATS = ("loss_e", "loss_f", "loss_d", "n_f", "n_d", "mae_e", "mae_f", "mae_d")  # DeNSLoss.stats, in this order


def add_masked_gaussian_noise_to_pos(data, std, prob, corrupt_ratio=None, seed=None):
    """The reference's function of this name (main_md17_dens.py:514-548), one launch: sets `pos` (corrupted), `force` (dy on
    the corrupted atoms, 0 elsewhere), `noise_vec`, `noise_mask` and `denoising_pos_mask` on `data` (which has pos, dy, batch
    on the GPU) and returns it.  seed: the 64-bit seed of this call's draws -- the same seed gives the same bits; None draws
    one from torch's CPU generator (the reference's behaviour: a fresh corruption per call)."""
    if seed is None:
        seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    batch = data.batch
    if batch.is_cuda and batch.dtype == torch.int64:
        batch = batch.to(torch.int32)
    pos, force, noise_vec, noise_mask, denoising_pos_mask = ops.dens_corrupt(
        data.pos.detach().to(torch.float32), data.dy.to(torch.float32), batch, std, prob, corrupt_ratio, seed)
    data.pos, data.force, data.noise_vec = pos, force, noise_vec
    data.noise_mask, data.denoising_pos_mask = noise_mask, denoising_pos_mask
    return data


class DeNSLoss:
    """loss = DeNSLoss(task_mean, task_std, denoising_pos_std, energy_weight, force_weight, denoising_pos_weight)
       l = loss(pred_y, pred_dy, data)       # data: y, dy, noise_vec, noise_mask

    energy_weight * L2MAE(pred_y, (y - mean) / std) + force_weight * L2MAE over the uncorrupted atoms of (pred_dy, dy / std)
    + denoising_pos_weight * L2MAE over the corrupted atoms of (pred_dy, noise_vec / denoising_pos_std); a term without atoms
    adds an exact 0 (the reference skips it after an `isnan` test).  `.stats`: 8 floats on the device, `STATS` names them --
    the losses, the two atom counts and the three MAEs of the last call."""

    def __init__(self, task_mean, task_std, denoising_pos_std, energy_weight, force_weight, denoising_pos_weight, device=None):
        self.task_mean, self.task_std, self.denoising_pos_std = float(task_mean), float(task_std), float(denoising_pos_std)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        dev = torch.device(device)
        if dev.type != "cuda":
            raise ops.HipOnlyError("the DeNS loss runs on MI355X only (got device %s); there is no CPU fallback" % dev)
        self.stats = torch.zeros(8, dtype=torch.float32, device=dev)
        self.weights = torch.zeros(3, dtype=torch.float32, device=dev)
        self._w_host = torch.zeros(3, dtype=torch.float32).pin_memory()
        self.set_weights(energy_weight, force_weight, denoising_pos_weight)

    def set_weights(self, energy_weight=None, force_weight=None, denoising_pos_weight=None):
        """Write the device words (None keeps a weight): pinned buffer, asynchronous copy, no synchronisation -- every later
        call and every later replay of a captured step sees the new values.  (A step's graph build reads back on the host,
        so the copy has landed before the next call here can touch the pinned words.)"""
        for i, w in enumerate((energy_weight, force_weight, denoising_pos_weight)):
            if w is not None:
                self._w_host[i] = float(w)
        self.weights.copy_(self._w_host, non_blocking=True)

    def __call__(self, pred_y, pred_dy, data, row_mask=None, num_graphs=None):
        """row_mask: [N] fp32, 1 real / 0 phantom (`view.node_mask` of a padded batch); num_graphs: the real molecules when
        `data.y` carries the phantom molecule's row as well (`view.B`)."""
        y = data.y if num_graphs is None else data.y[:num_graphs]
        return ops.dens_loss(pred_y, pred_dy, y, data.dy, data.noise_vec, data.noise_mask, self.weights, self.task_mean,
                             self.task_std, self.denoising_pos_std, row_mask=row_mask, stats_out=self.stats)


class DeNSTrainStep(_MirrorsBucketed):
    """ts = DeNSTrainStep(model, optimizer, loss, radius, std, prob, corrupt_ratio=None, seed=0, **bucket_kwargs)
       l = ts.step(batch)       # batch: mapping with pos [N, 3], z [N], batch [N] (ascending), y [B], dy [N, 3][, num_graphs]

    Step k corrupts the batch with the seed `step_seed(seed, k)` -- an eager loop that calls
    add_masked_gaussian_noise_to_pos(..., seed=step_seed(seed, k)) sees the same atoms move by the same amounts; torch's
    global generator is not touched -- and hands pos (corrupted), y and the node targets dy, force, noise_vec, noise_mask to
    a `BucketedTrainStep` (bucket_kwargs: min_eager, max_graphs, node_step, edge_step, max_num_neighbors, drop_path_seed) whose forward_loss is
    `model(view, graph=g)` and `loss(E[:view.B], dy_pred, view, row_mask=view.node_mask, num_graphs=view.B)`.  The phantom rows
    of a padded batch have noise_mask 0 and a zero force (nothing encoded) and stay out of the loss through the row mask.
    optimizer: a FlatAdamW without a reducer.  `.last`: the corrupted batch of the latest step; `.bucketed`: the
    BucketedTrainStep (its counters are mirrored here)."""

    NODE_TARGETS = ("dy", "force", "noise_vec", "noise_mask")

    def __init__(self, model, optimizer, loss, radius, std, prob, corrupt_ratio=None, seed=0, **bucket_kwargs):
        _refuse_reducer(optimizer, "DeNSTrainStep")
        self.model, self.loss = model, loss
        self.std, self.prob, self.corrupt_ratio, self.seed = float(std), float(prob), corrupt_ratio, int(seed)
        self.steps = 0
        self.last = None
        self.bucketed = BucketedTrainStep(optimizer, self._forward_loss, radius, graph_targets=("y",),
                                          node_targets=self.NODE_TARGETS, **bucket_kwargs)

    def _forward_loss(self, g, view):
        E, dy_pred = self.model(view, graph=g)
        return self.loss(E[:view.B], dy_pred, view, row_mask=view.node_mask, num_graphs=view.B)

    def step(self, batch):
        b = batch["batch"]
        b32 = b.to(torch.int32) if b.dtype != torch.int32 else b
        pos, force, noise_vec, noise_mask, denoising_pos_mask = ops.dens_corrupt(
            batch["pos"].to(torch.float32), batch["dy"].to(torch.float32), b32, self.std, self.prob, self.corrupt_ratio,
            step_seed(self.seed, self.steps))
        self.steps += 1
        d = dict(pos=pos, z=batch["z"], batch=b, y=batch["y"], dy=batch["dy"], force=force, noise_vec=noise_vec,
                 noise_mask=noise_mask, denoising_pos_mask=denoising_pos_mask)
        if "num_graphs" in batch:
            d["num_graphs"] = batch["num_graphs"]
        self.last = d
        return self.bucketed.step(d)
