"""CPU-side checks of the evaluation path (equiformer_amd/evaluate.py): the C-ABI entry eqf_metrics_accumulate in header and
binding table, its argument errors without a GPU, `Meter.figures` against a plain-torch fp64 restatement of the three reference
loops (engine.evaluate, main_md17.evaluate, the IS2RE evaluator) and the bucket / LRU bookkeeping of BucketedEvalStep."""
import ctypes
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "eqf_metrics_accumulate"


# ------------------------------------------------------------------------------------------------------------------ the entry point
def test_entry_point_is_declared_bound_and_cites_the_reference():
    from equiformer_amd import build, lib, ops
    header = open(os.path.join(ROOT, "include", "equiformer_hip.h")).read()
    assert "metrics.hip" in build.SOURCES
    before = header[:header.index("int %s(" % NAME)]
    comment = before[before.rindex("/*"):]
    for cite in ("engine.py:136-139", "main_md17.py:451-462", "_compute_metrics"):
        assert cite in comment, cite
    assert "stream" in comment and "capture" in comment  # the concurrency it supports is stated
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % NAME, text, flags=re.S)
    assert m, "%s is not declared in include/equiformer_hip.h" % NAME
    args = [a.strip() for a in m.group(1).split(",")]
    sig = lib.SIGNATURES[NAME]
    assert len(args) == len(sig) == 12
    for a, t in zip(args, sig):
        if "*" in a:
            assert t is ctypes.c_void_p, (a, t)
        elif a.startswith("int "):
            assert t is ctypes.c_int, (a, t)
        else:
            assert a.startswith("double ") and t is ctypes.c_double, (a, t)
    assert args[-1] == "void* stream" and args[-2] == "double* acc"
    assert [a.split()[-1].lstrip("*") for a in args[7:10]] == ["task_mean", "task_std", "threshold"]
    # the constants the Python side mirrors
    assert int(re.search(r"#define\s+EQF_METRICS_SUMS\s+(\d+)", header).group(1)) == ops.METRICS_SUMS
    assert int(re.search(r"#define\s+EQF_METRICS_THREADS\s+(\d+)", header).group(1)) == ops.METRICS_THREADS
    from equiformer_amd import evaluate
    assert len(evaluate.SUMS) == ops.METRICS_SUMS


def test_argument_errors_are_return_codes(hip_lib):
    p = ctypes.c_void_p(8)
    f = hip_lib.eqf_metrics_accumulate
    assert f(None, p, 4, None, None, None, 0, 0.0, 1.0, 0.02, p, None) == -1      # pred_y missing
    assert f(p, None, 4, None, None, None, 0, 0.0, 1.0, 0.02, p, None) == -1      # y missing
    assert f(p, p, 4, None, None, None, 0, 0.0, 1.0, 0.02, None, None) == -1      # acc missing
    assert f(p, p, 4, None, None, None, 0, 0.0, 0.0, 0.02, p, None) == -1         # std == 0
    assert f(p, p, 4, None, None, None, 0, 0.0, -1.0, 0.02, p, None) == -1        # std < 0
    assert f(p, p, 4, None, None, None, 0, 0.0, float("nan"), 0.02, p, None) == -1
    assert f(p, p, -1, None, None, None, 0, 0.0, 1.0, 0.02, p, None) == -1        # negative counts
    assert f(p, p, 4, p, p, None, -1, 0.0, 1.0, 0.02, p, None) == -1
    assert f(p, p, 4, p, None, None, 5, 0.0, 1.0, 0.02, p, None) == -1            # pred_dy without dy
    assert f(p, p, 0, None, None, None, 0, 0.0, 1.0, 0.02, p, None) == 0          # nothing to add: no launch
    assert f(p, p, 0, p, p, None, 0, 0.0, 1.0, 0.02, p, None) == 0


def test_meter_and_ops_refuse_the_cpu():
    from equiformer_amd import evaluate, ops
    with pytest.raises(ops.HipOnlyError):
        evaluate.Meter(0.0, 1.0, device="cpu")
    with pytest.raises(ops.HipOnlyError):
        ops.metrics_accumulate(torch.zeros(10, dtype=torch.float64), torch.zeros(3), torch.zeros(3), 3, 0.0, 1.0, 0.02)
    with pytest.raises(ops.HipOnlyError):
        evaluate.BucketedEvalStep(lambda g, v: None, 5.0, device="cpu")
    assert list(inspect.signature(evaluate.Meter.__init__).parameters)[1:] == ["task_mean", "task_std", "threshold", "device"]
    assert list(inspect.signature(evaluate.Meter.update).parameters)[1:] == ["pred_y", "y", "n_graphs", "pred_dy", "dy", "node_mask"]
    p = inspect.signature(evaluate.BucketedEvalStep.__init__).parameters
    assert list(p)[1:4] == ["predict", "radius", "meter"] and "optimizer" not in p
    assert p["min_eager"].default == 3 and p["max_graphs"].default == 16 and p["graph_targets"].default == ("y",)
    for fn, head in ((evaluate.evaluate_qm9, ["model", "norm_factor", "target", "loader", "radius"]),
                     (evaluate.evaluate_md17, ["model", "loader", "radius"]), (evaluate.evaluate_oc20, ["model", "loader", "radius"])):
        assert list(inspect.signature(fn).parameters)[:len(head)] == head


# ------------------------------------------------------------------------------------------------------------------ the figures
class AverageMeter:
    """the reference's (engine.py): a running average of per-batch means weighted by n"""

    def __init__(self):
        self.sum, self.count, self.avg = 0.0, 0, 0.0

    def update(self, val, n=1):
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


def _batches():
    """5 unequal batches of random fp64 predictions and targets: (pred_y [B], y [B], pred_dy [N, 3], dy [N, 3])"""
    g = torch.Generator().manual_seed(3)
    out = []
    for B, N in ((1, 21), (7, 150), (3, 40), (16, 333), (5, 111)):
        out.append((torch.randn(B, generator=g, dtype=torch.float64), torch.randn(B, generator=g, dtype=torch.float64) * 3 + 5,
                    torch.randn(N, 3, generator=g, dtype=torch.float64), torch.randn(N, 3, generator=g, dtype=torch.float64) * 2))
    return out


def _sums(batches, mean, std, thr):
    """the raw sums the kernel documents, in plain torch fp64"""
    from equiformer_amd.evaluate import SUMS
    s = dict.fromkeys(SUMS, 0.0)
    for p, y, pd, dy in batches:
        e = p * std + mean - y
        s["graphs"] += p.shape[0]
        s["abs_norm"] += float((p - (y - mean) / std).abs().sum())
        s["abs_err"] += float(e.abs().sum())
        s["sq_err"] += float((e * e).sum())
        s["within"] += float((e.abs() < thr).sum())
        s["atoms"] += pd.shape[0]
        s["force_l2"] += float((pd - dy / std).norm(dim=1).sum())
        s["force_abs_norm"] += float((pd - dy / std).abs().sum())
        s["force_abs_err"] += float((pd * std - dy).abs().sum())
        s["force_sq_err"] += float(((pd * std - dy) ** 2).sum())
    return s


def _close(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


def test_figures_are_the_three_reference_loops():
    from equiformer_amd.evaluate import Meter
    mean, std, thr = 5.0, 1.7, 0.5
    batches = _batches()
    fig = Meter.figures(_sums(batches, mean, std, thr))
    # engine.evaluate (engine.py:136-141)
    loss_m, mae_m = AverageMeter(), AverageMeter()
    for p, y, _, _ in batches:
        loss_m.update(torch.nn.functional.l1_loss(p, (y - mean) / std).item(), n=p.shape[0])
        mae_m.update(torch.mean(torch.abs(p * std + mean - y)).item(), n=p.shape[0])
    mae, loss = fig["qm9"]
    assert _close(mae, mae_m.avg) and _close(loss, loss_m.avg)
    # main_md17.evaluate (main_md17.py:451-462) with its criterion L2MAELoss (mean over rows of the row's L2 norm)
    def l2mae(a, b):
        return torch.mean(torch.norm(a - b, p=2, dim=-1))
    lm = {"energy": AverageMeter(), "force": AverageMeter()}
    mm = {"energy": AverageMeter(), "force": AverageMeter()}
    for p, y, pd, dy in batches:
        py, yy = p.view(-1, 1), y.view(-1, 1)
        lm["energy"].update(l2mae(py, (yy - mean) / std).item(), n=py.shape[0])
        lm["force"].update(l2mae(pd, dy / std).item(), n=pd.shape[0])
        mm["energy"].update(torch.mean(torch.abs(py * std + mean - yy)).item(), n=py.shape[0])
        mm["force"].update(torch.mean(torch.abs(pd * std - dy)).item(), n=pd.shape[0])
    mae_metrics, loss_metrics = fig["md17"]
    for k in ("energy", "force"):
        assert _close(mae_metrics[k].avg, mm[k].avg), k
        assert _close(loss_metrics[k].avg, lm[k].avg), k
        assert mae_metrics[k].count == mm[k].count and loss_metrics[k].count == lm[k].count
        assert _close(mae_metrics[k].sum, mm[k].sum) and _close(loss_metrics[k].sum, lm[k].sum)
    # the IS2RE evaluator: running total / numel over the denormalised predictions, threshold on |error|
    tot = {"energy_mae": 0.0, "energy_mse": 0.0, "energy_within_threshold": 0.0}
    numel = 0
    for p, y, _, _ in batches:
        e = p * std + mean - y
        tot["energy_mae"] += torch.abs(e).sum().item()
        tot["energy_mse"] += (e ** 2).sum().item()
        tot["energy_within_threshold"] += (torch.abs(e) < thr).sum().item()
        numel += e.numel()
    assert 0 < tot["energy_within_threshold"] < numel
    for k in tot:
        assert set(fig["oc20"][k]) == {"metric", "total", "numel"}
        assert fig["oc20"][k]["numel"] == numel and _close(fig["oc20"][k]["total"], tot[k])
        assert _close(fig["oc20"][k]["metric"], tot[k] / numel)
    assert fig["oc20"]["energy_within_threshold"]["total"] == tot["energy_within_threshold"]
    # nothing counted: NaN averages, not a division error
    empty = Meter.figures(_sums([], mean, std, thr))
    assert empty["qm9"][0] != empty["qm9"][0] and empty["md17"][0]["force"].count == 0


# ------------------------------------------------------------------------------------------------------------------ bookkeeping
def test_eval_step_shares_the_bucket_bookkeeping_of_the_train_step():
    from equiformer_amd import capture, evaluate
    assert issubclass(evaluate.BucketedEvalStep, capture._BucketedStep) and issubclass(capture.BucketedTrainStep, capture._BucketedStep)
    es = evaluate.BucketedEvalStep(lambda g, v: None, 5.0, min_eager=2, max_graphs=2, node_step=16, edge_step=128)
    assert (es.replays, es.eager_steps, es.captures, es.evictions, es.live_graphs()) == (0, 0, 0, 0, [])
    assert (es.node_step, es.edge_step, es.max_num_neighbors, es.graph_targets, es.node_targets) == (16, 128, 1000, ("y",), ())
    assert evaluate.BucketedEvalStep(lambda g, v: None, 5.0, max_graphs=0).max_graphs == 1
    # a bucket runs eagerly min_eager times, then earns a graph
    a, b, c = (6, 96, 640), (6, 112, 768), (6, 112, 896)
    assert es._count_eager(a) and es._count_eager(a) and not es._count_eager(a) and es.eager_steps == 2
    es._captured(a, "A")
    assert es._count_eager(b) and es._count_eager(b) and not es._count_eager(b)
    es._make_room()
    es._captured(b, "B")
    assert es.live_graphs() == [a, b] and es.evictions == 0
    # least recently used out, and its bucket has to be seen min_eager times again
    es._graphs.move_to_end(a)
    es._make_room()
    es._captured(c, "C")
    assert es.live_graphs() == [a, c] and es.evictions == 1 and es.captures == 3
    assert es._count_eager(b) and es.captures_of == {a: 1, b: 1, c: 1}
    # periodic or not, never both
    es._check_periodic({"pos": None})
    with pytest.raises(ValueError):
        es._check_periodic({"pos": None, "cell": None})


def test_eval_step_refuses_a_model_in_training_mode_before_it_touches_the_batch():
    from equiformer_amd import evaluate
    m = torch.nn.Linear(2, 2)

    def predict(g, v):
        return m(v.pos), None
    for es in (evaluate.BucketedEvalStep(predict, 5.0), evaluate.BucketedEvalStep(lambda g, v: None, 5.0, model=m),
               evaluate.BucketedEvalStep(m.forward, 5.0)):
        m.train()
        with pytest.raises(ValueError, match="training mode"):
            es.step({})
        m.eval()
        with pytest.raises(KeyError):  # past the check: the empty batch is what fails now
            es.step({})
