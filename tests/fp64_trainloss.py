"""Plain float64 restatement of the energy / force training loss and of the ten running sums (TEST INFRASTRUCTURE, not product
code), written the way the reference's loops are [ref: engine.py:71 and :85-87, main_md17.py:384-400 with L2MAELoss
:126-129, energy_trainer_v2.py:413-459]: boolean indexing first (the unpadded batch), then the criterion as a torch module.
Nothing here imports `equiformer_amd`; gradients come from autograd.  tests/test_fp64_trainloss.py pins it to the
reference's own criteria (or to tests/golden/trainloss/criteria.npz where there is no reference checkout).
"""
import ast
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = "/root/reference"  # the reference checkout, where tests/golden/make_reference_golden.py expects it
FIXTURE = os.path.join(HERE, "golden", "trainloss", "criteria.npz")
SCHEDULES = os.path.join(HERE, "golden", "trainloss", "schedules.json")
SUMS = ("graphs", "abs_norm", "abs_err", "sq_err", "within", "atoms", "force_l2", "force_abs_norm", "force_abs_err",
        "force_sq_err")


class L2MAELoss(torch.nn.Module):
    """main_md17.py:120-131, restated: mean over the rows of the L2 norm of the row's difference."""

    def forward(self, input, target):
        return torch.mean(torch.norm(input - target, p=2, dim=-1))


def criterion_module(name, l2mae=L2MAELoss):
    return {"l1": torch.nn.L1Loss(), "l2": torch.nn.MSELoss(), "l2mae": l2mae()}[name]


def ef_loss(pred_y, y, n_graphs, weights, task_mean, task_std, criterion, pred_dy=None, dy=None, row_mask=None, l2mae=L2MAELoss):
    """float64 loss: w_e C(pred_y[:n], (y[:n] - mean) / std) + w_f C(pred_dy[real], dy[real] / std); C applied to [n, 1] energies
    and [n_real, 3] forces as the reference applies it; an empty atom set adds 0 (the reference would get NaN)."""
    C = criterion_module(criterion, l2mae)
    py = pred_y.double().reshape(-1, 1)[:n_graphs]
    t = (y.double().reshape(-1, 1)[:n_graphs] - task_mean) / task_std
    w_e, w_f = (float(w) for w in weights)
    loss = w_e * C(py, t)
    if pred_dy is not None:
        pdy, tdy = pred_dy.double(), dy.double()
        if row_mask is not None:
            keep = row_mask.bool()
            pdy, tdy = pdy[keep], tdy[keep]
        if pdy.shape[0]:
            loss = loss + w_f * C(pdy, tdy / task_std)
    return loss


def sums(pred_y, y, n_graphs, task_mean, task_std, threshold, pred_dy=None, dy=None, row_mask=None):
    """the ten sums of evaluate.SUMS that one batch adds, float64"""
    p = pred_y.double().reshape(-1)[:n_graphs]
    t = y.double().reshape(-1)[:n_graphs]
    e = p * task_std + task_mean - t
    out = [float(n_graphs), (p - (t - task_mean) / task_std).abs().sum().item(), e.abs().sum().item(), (e * e).sum().item(),
           float((e.abs() < threshold).sum())]
    if pred_dy is None:
        return out + [0.0] * 5
    pdy, tdy = pred_dy.double(), dy.double()
    if row_mask is not None:
        keep = row_mask.bool()
        pdy, tdy = pdy[keep], tdy[keep]
    d, r = pdy - tdy / task_std, pdy * task_std - tdy
    return out + [float(pdy.shape[0]), d.norm(dim=1).sum().item(), d.abs().sum().item(), r.abs().sum().item(),
                  (r * r).sum().item()]


# ------------------------------------------------------------------------------------------------------------- the reference
def reference_available():
    return os.path.isfile(os.path.join(REFERENCE, "main_md17.py"))


def reference_l2mae():
    """The reference's own L2MAELoss class: its source cut out of main_md17.py (whose imports -- timm among them -- are not
    needed by the class) and compiled with torch in scope."""
    path = os.path.join(REFERENCE, "main_md17.py")
    tree = ast.parse(open(path).read(), path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "L2MAELoss"]
    assert len(cls) == 1
    ns = {"torch": torch}
    exec(compile(ast.Module(body=cls, type_ignores=[]), path, "exec"), ns)
    return ns["L2MAELoss"]


def reference_schedules():
    """(cosine_lr_lambda, multistep_lr_lambda) of the reference's oc20/trainer/lr_scheduler.py, loaded from the file"""
    import importlib.util
    path = os.path.join(REFERENCE, "oc20", "trainer", "lr_scheduler.py")
    spec = importlib.util.spec_from_file_location("_reference_lr_scheduler", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.cosine_lr_lambda, mod.multistep_lr_lambda


FIXTURE_CASES = (  # (N, n_graphs, rows of y, phantom atoms)
    (7, 3, 4, 2), (1, 1, 1, 0), (40, 5, 6, 9))
COSINE = dict(warmup_epochs=10, warmup_factor=0.2, epochs=100, lr_min_factor=0.01)
MULTISTEP = dict(warmup_epochs=5, warmup_factor=0.2, decay_epochs=[20, 40, 60], decay_rate=0.3)
COSINE_STEPS = (0, 1, 5, 9, 10, 11, 50, 99, 100, 101, 150)
MULTISTEP_STEPS = (0, 3, 5, 6, 19, 20, 21, 39, 40, 41, 60, 61, 1000)


def fixture_inputs(case):
    N, nB, rows, k = FIXTURE_CASES[case]
    g = torch.Generator().manual_seed(100 + case)
    d = dict(pred_y=torch.randn(rows, 1, generator=g, dtype=torch.float64),
             y=torch.randn(rows, generator=g, dtype=torch.float64) * 3 + 5,
             pred_dy=torch.randn(N, 3, generator=g, dtype=torch.float64),
             dy=torch.randn(N, 3, generator=g, dtype=torch.float64) * 2)
    m = torch.ones(N, dtype=torch.float64)
    if k:
        m[-k:] = 0
    d["row_mask"] = m
    return d, nB


FIXTURE_ARGS = dict(weights=(1.3, 40.0), task_mean=0.7, task_std=1.9)


def loop_loss(criterion, pred_y, y, pred_dy, dy, energy_weight, force_weight, task_mean, task_std):
    """main_md17.py:384-386 as written, on an UNPADDED batch (pred_y [B, 1], y [B, 1], pred_dy / dy [N, 3])"""
    loss_e = criterion(pred_y, ((y - task_mean) / task_std))
    loss_f = criterion(pred_dy, (dy / task_std))
    return energy_weight * loss_e + force_weight * loss_f


def fixture_loop_loss(case, crit, l2mae):
    d, nB = fixture_inputs(case)
    keep = d["row_mask"].bool()
    a = FIXTURE_ARGS
    return loop_loss(criterion_module(crit, l2mae), d["pred_y"][:nB], d["y"][:nB].reshape(-1, 1), d["pred_dy"][keep],
                     d["dy"][keep], a["weights"][0], a["weights"][1], a["task_mean"], a["task_std"])


def write_fixture():
    """Record the reference's criteria in its loop's expression, and its schedules, on the fixture cases (needs the reference
    checkout)."""
    import json
    C = reference_l2mae()
    out = {}
    for case in range(len(FIXTURE_CASES)):
        for crit in ("l1", "l2", "l2mae"):
            out["%d::%s" % (case, crit)] = fixture_loop_loss(case, crit, C).numpy()
    np.savez(FIXTURE, **out)
    cos, ms = reference_schedules()
    sched = {"cosine": [cos(s, COSINE) for s in COSINE_STEPS], "multistep": [ms(s, MULTISTEP) for s in MULTISTEP_STEPS]}
    with open(SCHEDULES, "w") as f:
        json.dump(sched, f, indent=1)


def load_fixture():
    z = np.load(FIXTURE)
    return {k: float(z[k]) for k in z.files}


if __name__ == "__main__":
    write_fixture()
    print("wrote", FIXTURE, SCHEDULES)
