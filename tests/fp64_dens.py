"""Plain float64 restatement of the DeNS step's loss, metrics and corruption invariants (TEST INFRASTRUCTURE, not product
code), written the way the reference's loop is [ref: main_md17_dens.py:389-427, :514-548]: boolean indexing, `mean`, a term
skipped when its mean over an empty set is NaN.  Nothing here imports `equiformer_amd.ops`; gradients come from autograd.
tests/test_dens_host.py pins it to a vectorised masked form.
"""
import torch

STATS = ("loss_e", "loss_f", "loss_d", "n_f", "n_d", "mae_e", "mae_f", "mae_d")


def l2mae(a, b):
    """The reference's criterion (L2MAELoss): mean over the rows of the L2 norm of the row's difference."""
    return torch.norm(a - b, p=2, dim=-1).mean()


def dens_loss(pred_y, pred_dy, y, dy, noise_vec, noise_mask, weights, task_mean, task_std, noise_std, row_mask=None):
    """(loss, stats[8]) in float64.  row_mask (bool, True = real row) drops the phantom rows of a padded batch first: what the
    reference computes on the unpadded batch."""
    pred_y, pred_dy = pred_y.double().reshape(-1, 1), pred_dy.double()
    y, dy, noise_vec = y.double().reshape(-1, 1), dy.double(), noise_vec.double()
    noise_mask = noise_mask.bool()
    if row_mask is not None:
        keep = row_mask.bool()
        pred_dy, dy, noise_vec, noise_mask = pred_dy[keep], dy[keep], noise_vec[keep], noise_mask[keep]
    w_e, w_f, w_d = (float(w) for w in weights)
    loss_e = l2mae(pred_y, (y - task_mean) / task_std)
    loss_f = l2mae(pred_dy[~noise_mask], dy[~noise_mask] / task_std)
    loss_d = l2mae(pred_dy[noise_mask], noise_vec[noise_mask] / noise_std)
    loss = w_e * loss_e
    if not loss_f.isnan():
        loss = loss + w_f * loss_f
    if not loss_d.isnan():
        loss = loss + w_d * loss_d
    zero = torch.zeros((), dtype=torch.float64)
    n_f, n_d = int((~noise_mask).sum()), int(noise_mask.sum())
    mae_e = (pred_y.detach() * task_std + task_mean - y).abs().mean()
    mae_f = mae_d = zero
    if not loss_f.isnan():
        mae_f = (pred_dy.detach() * task_std - dy)[~noise_mask].abs().mean()
    if not loss_d.isnan():
        mae_d = (pred_dy.detach() * noise_std - noise_vec)[noise_mask].abs().mean()
    stats = torch.stack([loss_e.detach(), zero if loss_f.isnan() else loss_f.detach(), zero if loss_d.isnan() else loss_d.detach(),
                         torch.tensor(float(n_f), dtype=torch.float64), torch.tensor(float(n_d), dtype=torch.float64),
                         mae_e, mae_f, mae_d])
    return loss, stats


def dens_loss_masked(pred_y, pred_dy, y, dy, noise_vec, noise_mask, weights, task_mean, task_std, noise_std, row_mask=None):
    """The same quantities without boolean indexing: per-row norms for both targets, selected with `where` and divided by the
    set's count; an empty set gives 0."""
    pred_y, pred_dy = pred_y.double().reshape(-1, 1), pred_dy.double()
    y, dy, noise_vec = y.double().reshape(-1, 1), dy.double(), noise_vec.double()
    m = noise_mask.bool()
    real = torch.ones_like(m) if row_mask is None else row_mask.bool()
    sel_f, sel_d = real & ~m, real & m
    zero = torch.zeros((), dtype=torch.float64)

    def mean_over(rows, sel, per_row):
        n = int(sel.sum())
        return (torch.where(sel, rows, torch.zeros_like(rows)).sum() / (n * per_row)) if n else zero

    w_e, w_f, w_d = (float(w) for w in weights)
    loss_e = (pred_y - (y - task_mean) / task_std).abs().mean()
    # (rows outside a set may hold anything: they are replaced BEFORE the norm, so that neither their value nor the
    # gradient of a norm at a garbage point reaches the result)
    df = torch.where(sel_f.view(-1, 1), pred_dy - dy / task_std, torch.zeros_like(dy))
    dd = torch.where(sel_d.view(-1, 1), pred_dy - noise_vec / noise_std, torch.zeros_like(dy))
    loss_f = mean_over(torch.linalg.vector_norm(df, dim=1), sel_f, 1)
    loss_d = mean_over(torch.linalg.vector_norm(dd, dim=1), sel_d, 1)
    loss = w_e * loss_e + w_f * loss_f + w_d * loss_d
    pd = pred_dy.detach()
    ef = torch.where(sel_f.view(-1, 1), pd * task_std - dy, torch.zeros_like(dy)).abs().sum(dim=1)
    ed = torch.where(sel_d.view(-1, 1), pd * noise_std - noise_vec, torch.zeros_like(dy)).abs().sum(dim=1)
    stats = torch.stack([loss_e.detach(), loss_f.detach(), loss_d.detach(),
                         torch.tensor(float(sel_f.sum()), dtype=torch.float64), torch.tensor(float(sel_d.sum()), dtype=torch.float64),
                         (pred_y.detach() * task_std + task_mean - y).abs().mean(), mean_over(ef, sel_f, 3), mean_over(ed, sel_d, 3)])
    return loss, stats


def check_corruption(pos, dy, batch, out, corrupt_ratio):
    """The exact invariants of add_masked_gaussian_noise_to_pos on CPU copies: out = (pos_out, force, noise_vec, noise_mask,
    denoising_pos_mask).  Raises AssertionError naming the broken one."""
    pos_out, force, noise_vec, noise_mask, dpm = out
    m = noise_mask.bool()
    assert noise_mask.dtype == torch.bool and dpm.dtype == torch.bool
    assert torch.equal(pos_out[m], (pos + noise_vec)[m]), "pos_out != pos + noise_vec on masked rows"
    assert torch.equal(pos_out[~m].view(torch.int32), pos[~m].view(torch.int32)), "pos changed on an unmasked row"
    assert torch.equal(force[m], dy[m]), "force != dy on masked rows"
    assert force[~m].abs().sum().item() == 0, "force != 0 on unmasked rows"
    for g in batch.unique().tolist():
        vals = dpm[batch == g]
        assert bool((vals == vals[0]).all()), "denoising_pos_mask varies inside molecule %d" % g
    if corrupt_ratio is None:
        assert torch.equal(noise_mask, dpm), "noise_mask != denoising_pos_mask without a corrupt ratio"
    else:
        assert bool((dpm | ~m).all()), "noise_mask is not a subset of denoising_pos_mask"
    assert torch.isfinite(noise_vec).all()
