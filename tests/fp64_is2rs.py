"""Plain float64 restatement of the IS2RE + IS2RS step's loss, metrics and perturbation invariants (TEST INFRASTRUCTURE, not
product code), written the way the reference's trainer is [ref: oc20/trainer/energy_trainer_v2.py:413-442 _compute_loss with the
`mae` losses, :445-459 the evaluator's energy figures, oc20/trainer/base_trainer_v2.py:81-126]: boolean indexing and
`abs().mean()`.  Nothing here imports `equiformer_amd.ops`; gradients come from autograd.  tests/test_is2rs_host.py pins it to a
second, literal statement on a hand-made case.
"""
import torch

STATS = ("loss_e", "loss_aux", "n_free", "energy_mae", "energy_mse", "energy_within_threshold", "pos_mae", "unused")


def _three(v):
    t = torch.as_tensor(v, dtype=torch.float64).reshape(-1)
    return t.expand(3) if t.numel() == 1 else t


def is2rs_loss(pred_y, pred_pos, y, pos, pos_relaxed, tags, weights, target_mean, target_std, positions_mean, positions_std,
               threshold=0.02, row_mask=None):
    """(loss, stats[8]) in float64.  row_mask (bool, True = real row) drops the phantom rows of a padded batch first: what the
    reference computes on the unpadded batch.  An empty free set adds 0 (the reference's empty mean would be NaN)."""
    pred_y, pred_pos = pred_y.double().reshape(-1), pred_pos.double()
    y, pos, pos_relaxed = y.double().reshape(-1), pos.double(), pos_relaxed.double()
    if row_mask is not None:
        keep = row_mask.bool()
        pred_pos, pos, pos_relaxed, tags = pred_pos[keep], pos[keep], pos_relaxed[keep], tags[keep]
    p_mean, p_std = _three(positions_mean), _three(positions_std)
    w_e, w_a = (float(w) for w in weights)
    zero = torch.zeros((), dtype=torch.float64)
    loss_e = (pred_y - (y - target_mean) / target_std).abs().mean()
    delta_pos = pos_relaxed - pos
    tag_mask = tags > 0
    n_free = int(tag_mask.sum())
    loss = w_e * loss_e
    loss_aux = pos_mae = zero
    if n_free:
        loss_aux = (pred_pos[tag_mask] - ((delta_pos - p_mean) / p_std)[tag_mask]).abs().mean()
        loss = loss + w_a * loss_aux
        pos_mae = (pred_pos.detach() * p_std + p_mean - delta_pos)[tag_mask].abs().mean()
    err = (pred_y.detach() * target_std + target_mean - y).abs()
    stats = torch.stack([loss_e.detach(), loss_aux.detach(), torch.tensor(float(n_free), dtype=torch.float64), err.mean(),
                         (err * err).mean(), (err < threshold).double().mean(), pos_mae, zero])
    return loss, stats


def check_perturbation(pos, pos_relaxed, tags, batch, outputs, f_min):
    """The exact invariants of interpolate_init_relaxed_pos on CPU copies: outputs = (pos_out, factor, noise_vec, selected).
    Raises AssertionError naming the broken one."""
    pos_out, factor, noise_vec, selected = outputs
    N = pos.shape[0]
    assert selected.dtype == torch.bool and pos_out.dtype == factor.dtype == noise_vec.dtype == torch.float32
    assert pos_out.shape == (N, 3) and factor.shape == (N,) and noise_vec.shape == (N, 3) and selected.shape == (N,)
    for g in batch.unique().tolist():
        vals = selected[batch == g]
        assert bool((vals == vals[0]).all()), "selected varies inside structure %d" % g
    m = selected & (tags > 0)
    assert torch.equal(pos_out[~m].view(torch.int32), pos[~m].view(torch.int32)), "pos changed on a fixed or unselected row"
    f = factor.view(-1, 1)
    want = (pos * f + (1 - f) * pos_relaxed) + noise_vec  # eager fp32 on the CPU: every operation rounded separately
    assert torch.equal(pos_out[m].view(torch.int32), want[m].view(torch.int32)), "moved rows != pos f + (1 - f) pos_relaxed + noise"
    assert bool((factor >= f_min).all()) and bool((factor < 1).all()), "factor outside [f_min, 1)"
    assert torch.isfinite(noise_vec).all() and torch.isfinite(pos_out).all()
    return m
