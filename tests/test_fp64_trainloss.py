"""The float64 restatement of tests/fp64_trainloss.py against the reference's own formulas (CPU only): the loss of its loops
[ref: main_md17.py:384-386 with L2MAELoss :126-129, torch.nn.L1Loss, torch.nn.MSELoss; engine.py:71] -- taken from the
reference checkout where it exists, from tests/golden/trainloss/criteria.npz (recorded from it) otherwise --, and the running
figures of equiformer_amd.train.figures against the reference's AverageMeter arithmetic.  Negative controls: a force target
not divided by std, the l1 force mean over N instead of 3N, a phantom row counted -- each misses the GPU bound of
tests/test_gpu_trainloss.py (1e-6 relative) by more than 1000 x."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_trainloss as ft  # noqa: E402

GPU_BOUND = 1e-6  # tests/test_gpu_trainloss.py
CRITERIA = ("l1", "l2", "l2mae")


def _l2mae():
    return ft.reference_l2mae() if ft.reference_available() else None


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-300)


@pytest.mark.parametrize("crit", CRITERIA)
@pytest.mark.parametrize("case", range(len(ft.FIXTURE_CASES)))
def test_restatement_equals_the_reference_loop(case, crit):
    """the padded form (row_mask, rows past n_graphs) equals the reference's loop expression on the unpadded batch"""
    d, nB = ft.fixture_inputs(case)
    a = ft.FIXTURE_ARGS
    got = ft.ef_loss(d["pred_y"], d["y"], nB, a["weights"], a["task_mean"], a["task_std"], crit, d["pred_dy"], d["dy"],
                     d["row_mask"])
    recorded = ft.load_fixture()["%d::%s" % (case, crit)]
    ref = _l2mae()
    if ref is not None:
        live = float(ft.fixture_loop_loss(case, crit, ref))
        print("case %d %s: restatement %.17g, reference %.17g, fixture %.17g" % (case, crit, float(got), live, recorded))
        assert _rel(recorded, live) <= 1e-14  # the fixture is what the reference computes
        assert _rel(got, live) <= 1e-13
    assert _rel(got, recorded) <= 1e-13


def test_reference_l2mae_is_the_restated_one_on_random_rows():
    ref = _l2mae()
    g = torch.Generator().manual_seed(3)
    for shape in ((5, 3), (1, 3), (7, 1), (64, 3)):
        a, b = torch.randn(*shape, generator=g, dtype=torch.float64), torch.randn(*shape, generator=g, dtype=torch.float64)
        a[0] = b[0]  # a zero row
        want = ft.L2MAELoss()(a, b)
        if ref is not None:
            assert float(ref()(a, b)) == float(want)
        assert _rel(want, torch.linalg.vector_norm(a - b, dim=1).mean()) <= 1e-15


def _case():
    d, nB = ft.fixture_inputs(2)
    return d, nB, ft.FIXTURE_ARGS


def test_negative_controls_miss_the_gpu_bound_by_far():
    d, nB, a = _case()
    w, mean, std = a["weights"], a["task_mean"], a["task_std"]
    keep = d["row_mask"].bool()
    for crit in CRITERIA:
        right = ft.ef_loss(d["pred_y"], d["y"], nB, w, mean, std, crit, d["pred_dy"], d["dy"], d["row_mask"])
        # (1) the force target not divided by std
        wrong = ft.ef_loss(d["pred_y"], d["y"], nB, w, mean, std, crit, d["pred_dy"], d["dy"] * std, d["row_mask"])
        # (3) a phantom row counted: the mask loses one zero
        m = d["row_mask"].clone()
        m[int((~keep).nonzero()[0])] = 1.0
        counted = ft.ef_loss(d["pred_y"], d["y"], nB, w, mean, std, crit, d["pred_dy"], d["dy"], m)
        for name, x in (("dy not / std", wrong), ("phantom row counted", counted)):
            print("%s %s: %.3e" % (crit, name, _rel(x, right)))
            assert _rel(x, right) > 1000 * GPU_BOUND, (crit, name)
    # (2) l1 forces averaged over N instead of 3N
    right = ft.ef_loss(d["pred_y"], d["y"], nB, w, mean, std, "l1", d["pred_dy"], d["dy"], d["row_mask"])
    e_only = ft.ef_loss(d["pred_y"], d["y"], nB, w, mean, std, "l1")
    diff = d["pred_dy"][keep] - d["dy"][keep] / std
    over_n = e_only + w[1] * diff.abs().sum() / keep.sum()
    print("l1 mean over N: %.3e" % _rel(over_n, right))
    assert _rel(over_n, right) > 1000 * GPU_BOUND


class _AverageMeter:
    """engine.py:12-27"""

    def __init__(self):
        self.sum, self.count = 0, 0

    def update(self, val, n=1):
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


@pytest.mark.parametrize("crit", CRITERIA)
def test_figures_are_the_reference_meters(crit):
    """three unpadded batches through main_md17.py:392-400's meters (engine.py:85-87 for the QM9 pair) against
    train.figures of the summed ten sums"""
    from equiformer_amd import train
    mean, std, thr = 0.3, 1.7, 0.5
    C = ft.criterion_module(crit, _l2mae() or ft.L2MAELoss)
    loss_m = {"energy": _AverageMeter(), "force": _AverageMeter()}
    mae_m = {"energy": _AverageMeter(), "force": _AverageMeter()}
    tot = [0.0] * 10
    g = torch.Generator().manual_seed(11)
    for B, N in ((3, 20), (5, 41), (1, 7)):
        py, y = torch.randn(B, 1, generator=g, dtype=torch.float64), torch.randn(B, 1, generator=g, dtype=torch.float64) + 1
        pdy, dy = torch.randn(N, 3, generator=g, dtype=torch.float64), torch.randn(N, 3, generator=g, dtype=torch.float64)
        loss_e, loss_f = C(py, (y - mean) / std), C(pdy, dy / std)
        loss_m["energy"].update(loss_e.item(), n=B)
        loss_m["force"].update(loss_f.item(), n=N)
        mae_m["energy"].update(torch.mean(torch.abs(py * std + mean - y)).item(), n=B)
        mae_m["force"].update(torch.mean(torch.abs(pdy * std - dy)).item(), n=N)
        tot = [a + b for a, b in zip(tot, ft.sums(py, y, B, mean, std, thr, pdy, dy))]
    f = train.figures(dict(zip(ft.SUMS, tot)), crit, std)
    mae, loss = f["md17"]
    for k in ("energy", "force"):
        assert _rel(mae[k].avg, mae_m[k].avg) <= 1e-12 and _rel(loss[k].avg, loss_m[k].avg) <= 1e-12, (k, crit)
    assert _rel(f["qm9"][0], mae_m["energy"].avg) <= 1e-12 and _rel(f["qm9"][1], loss_m["energy"].avg) <= 1e-12
    assert _rel(f["oc20_loss"], loss_m["energy"].avg) <= 1e-12
    if crit == "l2mae":  # evaluate_md17's shape and values
        from equiformer_amd.evaluate import Meter
        assert f["md17"] == Meter.figures(dict(zip(ft.SUMS, tot)))["md17"]
