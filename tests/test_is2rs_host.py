"""CPU-side checks of the IS2RE + IS2RS training step: the decay of the auxiliary weight, the public interface of
equiformer_amd.is2rs without a GPU, and the float64 restatement of tests/fp64_is2rs.py against a second, literal statement of the
reference's loss on a hand-made case whose answer is worked out here."""
import inspect
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_is2rs as fi  # noqa: E402


@pytest.mark.parametrize("w0,want", [(15.0, (15.0, 8.0, 1.0, 1.0)), (1.0, (1.0, 1.0, 1.0, 1.0)), (0.5, (0.5, 0.5, 0.5, 0.5))])
def test_auxiliary_task_weight_decays_linearly_to_one(w0, want):
    from equiformer_amd.is2rs import auxiliary_task_weight
    total = 1000
    got = tuple(auxiliary_task_weight(w0, s, total) for s in (0, total // 2, total, 3 * total))
    assert got == want, (got, want)
    assert auxiliary_task_weight(15.0, 250, 1000) == 11.5


def test_is2rs_imports_without_a_gpu_and_refuses_cpu_tensors():
    from equiformer_amd import dens, is2rs, ops
    assert is2rs.STATS == fi.STATS
    assert is2rs.step_seed is dens.step_seed
    with pytest.raises(ops.HipOnlyError):
        is2rs.IS2RSLoss(0.0, 1.0, 0.0, 1.0, 15.0, device="cpu")
    data = SimpleNamespace(pos=torch.zeros(4, 3), pos_relaxed=torch.zeros(4, 3), tags=torch.ones(4, dtype=torch.int64),
                           batch=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ops.HipOnlyError):
        is2rs.interpolate_init_relaxed_pos(data, seed=1)
    with pytest.raises(ops.HipOnlyError):
        ops.is2rs_loss(torch.zeros(1, 1), torch.zeros(4, 3), torch.zeros(1), torch.zeros(4, 3), torch.zeros(4, 3),
                       torch.ones(4, dtype=torch.int64), torch.ones(2), 0.0, 1.0, 0.0, 1.0)
    assert list(inspect.signature(is2rs.interpolate_init_relaxed_pos).parameters) == ["data", "seed", "p_perturb", "f_min", "noise_std"]
    assert list(inspect.signature(is2rs.IS2RSLoss.__init__).parameters)[1:] == [
        "target_mean", "target_std", "positions_mean", "positions_std", "auxiliary_task_weight", "energy_weight", "threshold",
        "device"]
    assert list(inspect.signature(is2rs.IS2RSTrainStep.__init__).parameters)[1:10] == [
        "model", "optimizer", "loss", "radius", "max_num_neighbors", "interpolate", "seed", "total_steps", "auxiliary_task_weight"]


def test_train_step_refuses_a_model_without_the_head_and_a_reducer():
    from equiformer_amd import is2rs
    with_head, without = SimpleNamespace(use_auxiliary_task=True), SimpleNamespace(use_auxiliary_task=False)
    with pytest.raises(ValueError, match="use_auxiliary_task"):
        is2rs.IS2RSTrainStep(without, SimpleNamespace(), None, 5.0, 50)
    with pytest.raises(ValueError, match="data-parallel steps stay eager"):
        is2rs.IS2RSTrainStep(with_head, SimpleNamespace(_reducer=object()), None, 5.0, 50)


def _literal_compute_loss(out, batch, target_norm, positions_norm, weight):
    """The steps of energy_trainer_v2.py:423-440 in their order, restated: L1 (`mean`) on the normalised energy target; the
    displacement to the relaxed positions, normalised ((x - mean) / std); the mask of the free atoms; L1 over the masked rows of
    prediction and target; the weighted sum."""
    l1 = torch.nn.L1Loss()
    energy_term = l1(out["energy"], target_norm(batch.y_relaxed))
    displacement = positions_norm(batch.pos_relaxed - batch.pos)
    free = batch.tags > 0
    aux_term = l1(out["pos"][free], displacement[free])
    return energy_term + aux_term * weight, aux_term


def test_restatement_agrees_with_a_literal_statement_on_a_worked_case():
    """3 structures, 5 atoms of which 2 are fixed.  Energies: mean 1, std 2, y = (3, 1, -1) -> targets (1, 0, -1); predictions
    (1.5, -0.5, -1) -> differences (0.5, 0.5, 0): loss_e = 1/3; in the target's units the errors are (1, 1, 0): MAE 2/3, MSE 2/3,
    one of three within 0.02.  Positions: pos = 0, positions mean (0.5, 0, 0), std (0.5, 0.5, 0.25); the free atoms' relaxed
    positions (1, 0, 0.5), (0, -1, 0), (0.5, 0.5, 0.25) -> targets (1, 0, 2), (-1, -2, 0), (0, 1, 1); predictions (2, 0, 2),
    (-1, 0, 1), (0, 1, 1) -> absolute differences sum to 1 + 3 + 0 = 4 over 9 components: loss_aux = 4/9; in Angstrom
    0.5 + 1.25 + 0 = 1.75 over 9.  With weights (1, 15): loss = 1/3 + 15 * 4/9 = 7."""
    d64 = torch.float64
    y = torch.tensor([3.0, 1.0, -1.0], dtype=d64)
    pred_y = torch.tensor([1.5, -0.5, -1.0], dtype=d64, requires_grad=True)
    tags = torch.tensor([1, 0, 2, 0, 1])
    pos = torch.zeros(5, 3, dtype=d64)
    pos_relaxed = torch.tensor([[1, 0, 0.5], [9, 9, 9], [0, -1, 0], [7, 7, 7], [0.5, 0.5, 0.25]], dtype=d64)
    pred_pos = torch.tensor([[2, 0, 2], [100, 100, 100], [-1, 0, 1], [-100, 3, 5], [0, 1, 1]], dtype=d64, requires_grad=True)
    p_mean, p_std = (0.5, 0.0, 0.0), (0.5, 0.5, 0.25)
    loss, stats = fi.is2rs_loss(pred_y, pred_pos, y, pos, pos_relaxed, tags, (1.0, 15.0), 1.0, 2.0, p_mean, p_std, threshold=0.02)
    gy, gp = torch.autograd.grad(loss, [pred_y, pred_pos])
    want = [1 / 3, 4 / 9, 3.0, 2 / 3, 2 / 3, 1 / 3, 1.75 / 9, 0.0]
    assert abs(loss.item() - 7.0) < 1e-14
    for name, got, w in zip(fi.STATS, stats.tolist(), want):
        assert abs(got - w) < 1e-15, (name, got, w)
    batch = SimpleNamespace(y_relaxed=y, pos=pos, pos_relaxed=pos_relaxed, tags=tags)
    py2, pp2 = pred_y.detach().clone().requires_grad_(True), pred_pos.detach().clone().requires_grad_(True)
    lit, lit_aux = _literal_compute_loss({"energy": py2, "pos": pp2}, batch, lambda t: (t - 1.0) / 2.0,
                                         lambda t: (t - torch.tensor(p_mean, dtype=d64)) / torch.tensor(p_std, dtype=d64), 15.0)
    gy2, gp2 = torch.autograd.grad(lit, [py2, pp2])
    assert abs(lit.item() - loss.item()) < 1e-14 and abs(lit_aux.item() - stats[1].item()) < 1e-15
    assert torch.allclose(gy, gy2, rtol=1e-15, atol=0) and torch.allclose(gp, gp2, rtol=1e-15, atol=0)
    # the gradient by hand: sign(d) w / count; fixed atoms and vanishing differences get 0
    assert torch.allclose(gy, torch.tensor([1 / 3, -1 / 3, 0.0], dtype=d64), rtol=1e-15, atol=0)
    c = 15.0 / 9
    assert torch.allclose(gp, torch.tensor([[c, 0, 0], [0, 0, 0], [0, c, c], [0, 0, 0], [0, 0, 0]], dtype=d64), rtol=1e-15, atol=0)
    # phantom rows behind a row mask and the empty free set
    rm = torch.tensor([True, True, True, True, True, False, False])
    pad = lambda t, v: torch.cat([t.detach(), torch.full((2,) + tuple(t.shape[1:]), v, dtype=t.dtype)])  # noqa: E731
    loss_p, stats_p = fi.is2rs_loss(pred_y, pad(pred_pos, 3e37), y, pad(pos, 0), pad(pos_relaxed, 1), pad(tags, 2), (1.0, 15.0), 1.0, 2.0,
                                    p_mean, p_std, row_mask=rm)
    assert abs(loss_p.item() - 7.0) < 1e-14 and torch.equal(stats_p, stats)
    loss_0, stats_0 = fi.is2rs_loss(pred_y, pred_pos, y, pos, pos_relaxed, torch.zeros(5, dtype=torch.int64), (1.0, 15.0), 1.0, 2.0,
                                    p_mean, p_std)
    assert abs(loss_0.item() - 1 / 3) < 1e-15 and stats_0[1].item() == 0 and stats_0[2].item() == 0 and stats_0[6].item() == 0


def test_check_perturbation_accepts_a_hand_made_case_and_rejects_a_broken_one():
    pos = torch.arange(12, dtype=torch.float32).view(4, 3)
    pos_relaxed = pos + 1.0
    tags = torch.tensor([1, 0, 2, 1])
    batch = torch.tensor([0, 0, 1, 1])
    factor = torch.tensor([0.25, 0.5, 0.75, 0.0])
    nv = torch.full((4, 3), 0.125)
    selected = torch.tensor([True, True, False, False])
    moved = pos * factor.view(-1, 1) + (1 - factor.view(-1, 1)) * pos_relaxed + nv
    pos_out = torch.where((selected & (tags > 0)).view(-1, 1), moved, pos)
    m = fi.check_perturbation(pos, pos_relaxed, tags, batch, (pos_out, factor, nv, selected), 0.0)
    assert m.tolist() == [True, False, False, False]
    with pytest.raises(AssertionError):  # a fixed atom moved
        fi.check_perturbation(pos, pos_relaxed, tags, batch, (moved, factor, nv, selected), 0.0)
    with pytest.raises(AssertionError):  # the draw varies inside a structure
        fi.check_perturbation(pos, pos_relaxed, tags, batch, (pos_out, factor, nv, torch.tensor([True, False, False, False])), 0.0)
    with pytest.raises(AssertionError):  # factor below f_min
        fi.check_perturbation(pos, pos_relaxed, tags, batch, (pos_out, factor, nv, selected), 0.1)
