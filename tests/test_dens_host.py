"""CPU-side checks of the DeNS training step: the float64 restatement of tests/fp64_dens.py against a vectorised masked form,
the public interface of equiformer_amd.dens without a GPU, and the new C-ABI entry points in header and binding table."""
import inspect
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_dens as fd  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("eqf_dens_corrupt", "eqf_dens_loss_fwd", "eqf_dens_loss_bwd")


def _inputs(N, nB, mask, seed):
    g = torch.Generator().manual_seed(seed)
    d = dict(pred_y=torch.randn(nB, 1, generator=g, dtype=torch.float64, requires_grad=True),
             pred_dy=torch.randn(N, 3, generator=g, dtype=torch.float64, requires_grad=True),
             y=torch.randn(nB, generator=g, dtype=torch.float64) * 3 + 5, dy=torch.randn(N, 3, generator=g, dtype=torch.float64) * 2,
             noise_vec=torch.randn(N, 3, generator=g, dtype=torch.float64) * 0.05)
    d["noise_mask"] = {"mixed": torch.rand(N, generator=g) < 0.4, "all": torch.ones(N, dtype=torch.bool),
                       "none": torch.zeros(N, dtype=torch.bool)}[mask]
    return d


@pytest.mark.parametrize("mask", ["mixed", "all", "none"])
@pytest.mark.parametrize("N,nB,phantoms", [(1, 1, 0), (37, 3, 0), (65, 2, 9)])
def test_restatement_agrees_with_masked_form(N, nB, phantoms, mask):
    d = _inputs(N, nB, mask, seed=N + nB)
    row_mask = None
    if phantoms:
        row_mask = torch.ones(N, dtype=torch.bool)
        row_mask[-phantoms:] = False
        with torch.no_grad():
            d["pred_dy"][-phantoms:] = 1e30  # garbage on the phantom rows reaches neither form
    if N > 3:
        with torch.no_grad():  # one row whose difference is exactly zero: both forms take the zero subgradient
            d["pred_dy"][2] = (d["noise_vec"][2] / 0.05) if d["noise_mask"][2] else (d["dy"][2] / 1.7)
    args = (d["pred_y"], d["pred_dy"], d["y"], d["dy"], d["noise_vec"], d["noise_mask"], (1.0, 80.0, 0.25), 5.0, 1.7, 0.05)
    la, sa = fd.dens_loss(*args, row_mask=row_mask)
    ga = torch.autograd.grad(la, [d["pred_y"], d["pred_dy"]])
    lb, sb = fd.dens_loss_masked(*args, row_mask=row_mask)
    gb = torch.autograd.grad(lb, [d["pred_y"], d["pred_dy"]])
    assert torch.isfinite(la) and abs(la.item() - lb.item()) <= 1e-13 * max(1.0, abs(la.item()))
    assert torch.allclose(sa, sb, rtol=1e-13, atol=0)
    n_real = N - phantoms
    want_f = {"mixed": None, "all": 0, "none": n_real}[mask]
    if want_f is not None:
        assert sa[3].item() == want_f and sa[4].item() == n_real - want_f
        empty = (1, 6) if mask == "all" else (2, 7)
        assert sa[empty[0]].item() == 0 and sa[empty[1]].item() == 0
    assert sa[3].item() + sa[4].item() == n_real
    for x, r in zip(gb, ga):
        assert torch.isfinite(r).all() and torch.allclose(x, r, rtol=1e-12, atol=1e-300)
    if phantoms:
        assert ga[1][-phantoms:].abs().sum().item() == 0
    if N > 3:
        assert ga[1][2].abs().sum().item() == 0


def test_check_corruption_accepts_a_hand_made_case_and_rejects_a_broken_one():
    pos = torch.arange(12, dtype=torch.float32).view(4, 3)
    dy = torch.ones(4, 3)
    batch = torch.tensor([0, 0, 1, 1])
    nv = torch.full((4, 3), 0.5)
    dpm = torch.tensor([True, True, False, False])
    m = torch.tensor([True, False, False, False])
    pos_out = torch.where(m.view(-1, 1), pos + nv, pos)
    force = torch.where(m.view(-1, 1), dy, torch.zeros_like(dy))
    fd.check_corruption(pos, dy, batch, (pos_out, force, nv, m, dpm), corrupt_ratio=0.5)
    with pytest.raises(AssertionError):
        fd.check_corruption(pos, dy, batch, (pos_out, force, nv, m, dpm), corrupt_ratio=None)
    with pytest.raises(AssertionError):
        fd.check_corruption(pos, dy, batch, (pos_out, force, nv, m, torch.tensor([True, False, False, False])), corrupt_ratio=0.5)


def test_dens_imports_without_a_gpu_and_refuses_cpu_tensors():
    from equiformer_amd import dens, ops
    assert dens.STATS == fd.STATS
    assert dens.step_seed(5, 0) == 5 and dens.step_seed(5, 2) == (5 + 2 * 0x9E3779B97F4A7C15) % 2 ** 64
    assert dens.step_seed(2 ** 64 - 1, 1) < 2 ** 64
    data = SimpleNamespace(pos=torch.zeros(4, 3), dy=torch.zeros(4, 3), batch=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ops.HipOnlyError):
        dens.add_masked_gaussian_noise_to_pos(data, 0.05, 0.5, seed=1)
    with pytest.raises(ops.HipOnlyError):
        ops.dens_loss(torch.zeros(1, 1), torch.zeros(4, 3), torch.zeros(1), torch.zeros(4, 3), torch.zeros(4, 3),
                      torch.zeros(4, dtype=torch.bool), torch.ones(3), 0.0, 1.0, 0.05)
    with pytest.raises(ops.HipOnlyError):
        dens.DeNSLoss(0.0, 1.0, 0.05, 1.0, 80.0, 10.0, device="cpu")
    names = list(inspect.signature(dens.add_masked_gaussian_noise_to_pos).parameters)
    assert names == ["data", "std", "prob", "corrupt_ratio", "seed"]
    assert list(inspect.signature(dens.DeNSLoss.__init__).parameters)[1:7] == [
        "task_mean", "task_std", "denoising_pos_std", "energy_weight", "force_weight", "denoising_pos_weight"]
    assert list(inspect.signature(dens.DeNSTrainStep.__init__).parameters)[1:9] == [
        "model", "optimizer", "loss", "radius", "std", "prob", "corrupt_ratio", "seed"]


def test_train_step_refuses_a_reducer():
    from equiformer_amd import dens
    opt = SimpleNamespace(_reducer=object())
    with pytest.raises(ValueError):
        dens.DeNSTrainStep(None, opt, None, 5.0, 0.05, 0.5)


def test_dens_forward_takes_a_graph():
    from equiformer_amd.nets.equiformer_md17_dens import Equiformer_MD17_DeNS
    p = inspect.signature(Equiformer_MD17_DeNS.forward).parameters
    assert list(p) == ["self", "data", "graph"] and p["graph"].default is None


def test_new_entry_points_are_declared_and_bound():
    from equiformer_amd import build, lib
    header = open(os.path.join(ROOT, "include", "equiformer_hip.h")).read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in lib.SIGNATURES, name
    assert "dens.hip" in build.SOURCES
    # the weights and the upstream gradient are device pointers, the seed of the corruption is a 64-bit value
    assert lib.SIGNATURES["eqf_dens_corrupt"][7] is lib._u64
    assert lib.SIGNATURES["eqf_dens_loss_fwd"][7] is lib.c_fp and lib.SIGNATURES["eqf_dens_loss_bwd"][0] is lib.c_fp
    # every entry cites the reference lines it replaces
    for name in NEW:
        before = header[:header.index("int %s(" % name)]
        assert "main_md17_dens.py:" in before[before.rindex("/*"):], name


def test_argument_errors_are_return_codes(hip_lib):
    import ctypes
    p = ctypes.c_void_p(8)
    assert hip_lib.eqf_dens_corrupt(None, None, None, 4, 0.1, 0.5, -1.0, 1, None, None, None, None, None, None) == -1
    assert hip_lib.eqf_dens_corrupt(None, None, None, 0, 0.1, 0.5, -1.0, 1, None, None, None, None, None, None) == 0
    assert hip_lib.eqf_dens_corrupt(p, p, p, -1, 0.1, 0.5, -1.0, 1, p, p, p, p, p, None) == -1
    assert hip_lib.eqf_dens_loss_fwd(p, p, p, p, p, p, None, p, 4, 0, 0.0, 1.0, 0.05, p, p, None) == -1
    assert hip_lib.eqf_dens_loss_fwd(p, p, p, p, p, p, None, None, 4, 1, 0.0, 1.0, 0.05, p, p, None) == -1
    assert hip_lib.eqf_dens_loss_fwd(p, p, p, p, p, p, None, p, 4, 1, 0.0, 0.0, 0.05, p, p, None) == -1
    assert hip_lib.eqf_dens_loss_bwd(None, p, p, p, p, p, p, None, p, p, 4, 1, 0.0, 1.0, 0.05, p, p, None) == -1
