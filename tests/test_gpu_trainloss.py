"""The fused energy / force training loss (csrc/trainloss.hip: eqf_ef_loss_fwd / _bwd) through the C ABI, every buffer between
NaN guard rows, against the float64 restatement of tests/fp64_trainloss.py: loss, both gradients and the ten running sums.

Grid: criterion l1 / l2 / l2mae, with and without forces; n_graphs 1, 255, 256, 257 (one, and around the 256 lanes of the
workgroup); N 0, 1, 3, 256, 257, 1000; row masks none / a phantom tail / all phantom; a real row and a real energy whose
difference is exactly zero; NaN in every phantom row and in the energy row past n_graphs.

Bound: 1e-6 relative to the largest magnitude of the quantity -- the bound at which tests/test_gpu_dens_step.py holds
eqf_dens_loss_* to tests/fp64_dens.py; the summation scheme is the same (fp64 lane partials, wave shuffles, waves in order),
so the error is the final fp32 store (2^-24) plus fp64 rounding.  The worst measured figure is printed; on an MI355X: loss
5.4e-8, d_pred_y 5.7e-8, d_pred_dy 4.8e-8, the ten sums 3.3e-16.
Wall time of this file on an MI355X, one run each (pytest's figure): 3.5 s at the parent commit, 3.9 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py)."""
import ctypes
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_trainloss as ft  # noqa: E402
from poison import guard_input, poisoned_ops  # noqa: E402,F401  (the fixture of the tests that run on poisoned, guarded allocations)

DEV = torch.device("cuda:0")
BOUND = 1e-6
G = 64  # guard elements on each side of every buffer
MEAN, STD, THR = 5.0, 1.7, 0.5
W = (1.0, 80.0)
UP = float(torch.tensor(0.37, dtype=torch.float32))  # the upstream gradient, an fp32 word
CRIT = {"l1": 0, "l2": 1, "l2mae": 2}
N_GRAPHS = (1, 255, 256, 257)
NS = (0, 1, 3, 256, 257, 1000)
MASKS = ("none", "tail", "all")
WORST = {}


class Buf:
    """a flat device buffer [G | data | G]; the guards hold NaN (fp32 / fp64) and must keep their bits"""

    def __init__(self, data, dtype=torch.float32):
        flat = data.reshape(-1).to(dtype)
        self.shape, self.n, self.dtype = tuple(data.shape), flat.numel(), dtype
        buf = torch.full((2 * G + self.n,), float("nan"), dtype=dtype)
        buf[G:G + self.n] = flat
        self.buf = guard_input(buf.to(DEV))  # (and the whole of it between the bands of tests/poison.py: a store further out than G)
        self.guards = self._guard_bits().clone()

    def _guard_bits(self):
        it = torch.int32 if self.dtype == torch.float32 else torch.int64
        return torch.cat([self.buf[:G], self.buf[G + self.n:]]).view(it).cpu()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf[G:].data_ptr())

    def mid(self):
        return self.buf[G:G + self.n].cpu().reshape(self.shape)

    def check(self, what):
        assert torch.equal(self._guard_bits(), self.guards), "%s: a guard element changed" % what
        return self.mid()


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inputs(n_graphs, N, mask, seed):
    g = torch.Generator().manual_seed(seed)
    d = dict(pred_y=torch.randn(n_graphs + 1, generator=g), y=torch.randn(n_graphs + 1, generator=g) * 3 + MEAN,
             pred_dy=torch.randn(N, 3, generator=g), dy=torch.randn(N, 3, generator=g) * 2)
    d["pred_y"][0], d["y"][0] = 0.0, MEAN  # an energy whose difference is exactly zero
    d["pred_y"][-1] = d["y"][-1] = float("nan")  # the row past n_graphs
    m = torch.ones(N)
    if mask == "tail":
        m[N - max(1, N // 4):] = 0.0
    elif mask == "all":
        m[:] = 0.0
    if N:
        d["pred_dy"][0] = 0.0  # a force row whose difference is exactly zero (a real row unless all are phantom)
        d["dy"][0] = 0.0
    d["pred_dy"][m == 0] = float("nan")
    d["dy"][m == 0] = float("nan")
    d["row_mask"] = None if mask == "none" else m
    return d


def _reference(d, n_graphs, crit, forces):
    py = d["pred_y"].double().requires_grad_(True)
    pdy = d["pred_dy"].double().requires_grad_(True)
    rm = d["row_mask"]
    loss = ft.ef_loss(py, d["y"], n_graphs, W, MEAN, STD, crit, pdy if forces else None, d["dy"] if forces else None,
                      rm if forces else None)
    gy, gdy = torch.autograd.grad(loss * UP, [py, pdy], allow_unused=True)
    gy = torch.zeros_like(py) if gy is None else gy
    gy[n_graphs:] = 0.0  # (slicing gives the row past n_graphs no gradient; autograd leaves it 0)
    gdy = torch.zeros_like(pdy) if gdy is None else gdy
    if rm is not None:
        gdy[rm == 0] = 0.0
    sums = ft.sums(d["pred_y"], d["y"], n_graphs, MEAN, STD, THR, d["pred_dy"] if forces else None,
                   d["dy"] if forces else None, rm if forces else None)
    return float(loss.detach()), gy.detach(), gdy.detach(), torch.tensor(sums, dtype=torch.float64)


def _launch(d, n_graphs, crit, forces, acc_fill=None):
    """one forward and one backward through the C ABI -> (loss, d_pred_y, d_pred_dy, acc after the forward) as CPU tensors"""
    from equiformer_amd import lib
    N = d["pred_dy"].shape[0]
    b = {k: Buf(d[k]) for k in ("pred_y", "y", "pred_dy", "dy")}
    rm = None if d["row_mask"] is None else Buf(d["row_mask"])
    w = Buf(torch.tensor(W))
    loss = Buf(torch.full((1,), float("nan")))
    acc = Buf(torch.zeros(10) if acc_fill is None else acc_fill, torch.float64)
    f = forces
    lib.call("eqf_ef_loss_fwd", b["pred_y"].ptr, b["y"].ptr, n_graphs, b["pred_dy"].ptr if f else None,
             b["dy"].ptr if f else None, rm.ptr if (rm is not None and f) else None, N if f else 0, w.ptr, CRIT[crit], MEAN, STD,
             THR, loss.ptr, acc.ptr, _st())
    up = Buf(torch.tensor([UP]))
    gy = Buf(torch.full((n_graphs + 1,), float("nan")))
    gdy = Buf(torch.full((N, 3), float("nan")))
    lib.call("eqf_ef_loss_bwd", up.ptr, b["pred_y"].ptr, b["y"].ptr, n_graphs, n_graphs + 1, b["pred_dy"].ptr if f else None,
             b["dy"].ptr if f else None, rm.ptr if (rm is not None and f) else None, N if f else 0, w.ptr, CRIT[crit], MEAN, STD,
             gy.ptr, gdy.ptr if f else None, _st())
    torch.cuda.synchronize()
    for k, v in b.items():
        v.check(k)
    if rm is not None:
        rm.check("row_mask")
    w.check("weights"), up.check("d_loss")
    out = (loss.check("loss"), gy.check("d_pred_y"), gdy.check("d_pred_dy"), acc.check("acc"))
    assert torch.isfinite(out[0]).all() and torch.isfinite(out[1]).all() and torch.isfinite(out[3]).all()
    if f:
        assert torch.isfinite(out[2]).all()
    else:
        assert torch.isnan(out[2]).all(), "without forces d_pred_dy is not written"
    return out


def _close(got, want, what, key):
    # (dtype at construction: a Python float would otherwise become a float32 tensor, rounding the fp64 reference)
    got = torch.as_tensor(got).double().reshape(-1)
    want = torch.as_tensor(want, dtype=torch.float64).reshape(-1)
    if not want.numel():
        return
    err = (got - want).abs().max().item()
    scale = want.abs().max().item()
    rel = err / scale if scale > 0 else (0.0 if err == 0 else math.inf)
    if what not in WORST or rel > WORST[what][0]:
        WORST[what] = (rel, key)
    assert err <= BOUND * scale, (what, key, err, scale)


@pytest.mark.usefixtures("poisoned_ops")
@pytest.mark.parametrize("forces", [True, False])
@pytest.mark.parametrize("crit", ["l1", "l2", "l2mae"])
def test_grid_against_fp64(crit, forces):
    WORST.clear()
    for n_graphs in N_GRAPHS:
        for N in NS:
            for mask in MASKS:
                key = (crit, forces, n_graphs, N, mask)
                d = _inputs(n_graphs, N, mask, seed=1000 * N_GRAPHS.index(n_graphs) + 10 * NS.index(N) + MASKS.index(mask))
                real = torch.ones(N, dtype=torch.bool) if d["row_mask"] is None else d["row_mask"] > 0
                want = _reference(d, n_graphs, crit, forces)
                got = _launch(d, n_graphs, crit, forces)
                again = _launch(d, n_graphs, crit, forces)
                for a, b in zip(got, again):
                    assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), ("two launches differ", key)
                _close(got[0], want[0], "loss", key)
                _close(got[1], want[1], "d_pred_y", key)
                assert got[1][-1].item() == 0.0 and got[1][0].item() == 0.0, "phantom energy row / zero difference: exact 0"
                if forces:
                    _close(got[2], want[2], "d_pred_dy", key)
                    assert got[2][~real].abs().sum().item() == 0, "phantom rows: exact zeros"
                    if N and bool(real[0]):
                        assert got[2][0].abs().sum().item() == 0, "zero difference: exact zero gradient"
                    if not bool(real.any()):
                        assert got[2].abs().sum().item() == 0
                for q, name in enumerate(ft.SUMS):
                    _close(got[3][q], want[3][q], "sum " + name, key)
                assert got[3][0].item() == n_graphs and got[3][5].item() == (int(real.sum()) if forces else 0)
    for what, (rel, key) in sorted(WORST.items()):
        print("%-20s worst %.3e at %s (bound %.0e)" % (what, rel, key, BOUND))


@pytest.mark.usefixtures("poisoned_ops")
def test_sums_accumulate_over_three_batches():
    prefill = torch.randn(10, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    acc, want = prefill, prefill.clone()
    for i, (n_graphs, N, mask) in enumerate(((255, 257, "tail"), (1, 3, "none"), (257, 1000, "tail"))):
        d = _inputs(n_graphs, N, mask, seed=900 + i)
        acc = _launch(d, n_graphs, "l2mae", True, acc_fill=acc)[3]
        want = want + _reference(d, n_graphs, "l2mae", True)[3]
    for q, name in enumerate(ft.SUMS):
        _close(acc[q], want[q], "accumulated " + name, "three batches")
    print("accumulated sums: worst %.3e" % max(v[0] for k, v in WORST.items() if k.startswith("accumulated")))


@pytest.mark.usefixtures("poisoned_ops")
def test_operator_autograd_and_device_weights():
    """ops.ef_loss / EFLoss: the autograd path, the meter's sums, a weight changed between two calls"""
    from equiformer_amd.train import EFLoss
    d = _inputs(5, 257, "tail", seed=77)
    L = EFLoss(MEAN, STD, "l2mae", W[0], W[1], threshold=THR)

    def run():
        py = d["pred_y"].to(DEV).requires_grad_(True)
        pdy = d["pred_dy"].to(DEV).requires_grad_(True)
        loss = L(py, d["y"].to(DEV), 5, pdy, d["dy"].to(DEV), d["row_mask"].to(DEV))
        (loss * UP).backward()
        return loss.detach().cpu(), py.grad.cpu(), pdy.grad.cpu()
    want = _reference(d, 5, "l2mae", True)
    got = run()
    for i, what in enumerate(("loss", "d_pred_y", "d_pred_dy")):
        _close(got[i], want[i], "ops " + what, "autograd")
    _close(L.meter.acc.cpu(), want[3], "ops sums", "autograd")
    L.set_weights(force_weight=10.0)
    W2 = (W[0], 10.0)
    loss2 = float(ft.ef_loss(d["pred_y"], d["y"], 5, W2, MEAN, STD, "l2mae", d["pred_dy"], d["dy"], d["row_mask"]))
    _close(run()[0], loss2, "ops loss after set_weights", "autograd")
    _close(L.meter.acc.cpu(), 2 * want[3], "ops sums after two calls", "autograd")


def test_refusals_raise_before_a_launch():
    from equiformer_amd import lib, ops
    acc = torch.zeros(10, dtype=torch.float64, device=DEV)
    w = torch.tensor(W, device=DEV)
    py, y = torch.randn(4, 1, device=DEV), torch.randn(4, device=DEV)
    pdy, dy, rm = torch.randn(9, 3, device=DEV), torch.randn(9, 3, device=DEV), torch.ones(9, device=DEV)

    def ok(**kw):
        a = dict(pred_y=py, y=y, n_graphs=3, weights=w, task_mean=MEAN, task_std=STD, criterion="l1", pred_dy=pdy, dy=dy,
                 row_mask=rm, acc=acc)
        a.update(kw)
        return a
    bad = [dict(pred_y=py.double()), dict(y=y.cpu()), dict(pred_dy=pdy.cpu()), dict(dy=dy[:, :2].contiguous()),
           dict(pred_dy=torch.randn(8, 3, device=DEV)), dict(row_mask=rm[:8]), dict(row_mask=rm.double()),
           dict(weights=torch.ones(3, device=DEV)), dict(weights=w.cpu()), dict(acc=acc.float()), dict(acc=acc[:9]),
           dict(acc=acc.cpu()), dict(n_graphs=0), dict(n_graphs=5), dict(criterion="mse"), dict(task_std=0.0),
           dict(dy=None), dict(pred_dy=None), dict(pred_dy=pdy[::2].contiguous()), dict(pred_dy=pdy.t()),
           dict(pred_dy=None, dy=None)]
    for kw in bad:
        with pytest.raises((ValueError, ops.HipOnlyError, RuntimeError)):
            ops.ef_loss(**ok(**kw))
    torch.cuda.synchronize()
    assert acc.abs().sum().item() == 0, "a refused call launched"
    # the C ABI refuses what ops.ef_loss would not hand it: nothing is launched either
    loss = torch.full((1,), float("nan"), device=DEV)
    for n_graphs, crit, std, with_dy in ((0, 0, 1.0, True), (3, 3, 1.0, True), (3, -1, 1.0, True), (3, 0, 0.0, True),
                                         (3, 0, -1.0, True), (3, 0, 1.0, False)):
        with pytest.raises(lib.HipLibraryError):
            lib.call("eqf_ef_loss_fwd", ctypes.c_void_p(py.data_ptr()), ctypes.c_void_p(y.data_ptr()), n_graphs,
                     ctypes.c_void_p(pdy.data_ptr()), ctypes.c_void_p(dy.data_ptr()) if with_dy else None, None, 9,
                     ctypes.c_void_p(w.data_ptr()), crit, 0.0, std, 0.02, ctypes.c_void_p(loss.data_ptr()),
                     ctypes.c_void_p(acc.data_ptr()), _st())
    with pytest.raises(lib.HipLibraryError):  # n_rows_y < n_graphs
        lib.call("eqf_ef_loss_bwd", ctypes.c_void_p(loss.data_ptr()), ctypes.c_void_p(py.data_ptr()),
                 ctypes.c_void_p(y.data_ptr()), 3, 2, None, None, None, 0, ctypes.c_void_p(w.data_ptr()), 0, 0.0, 1.0,
                 ctypes.c_void_p(loss.data_ptr()), None, _st())
    torch.cuda.synchronize()
    assert acc.abs().sum().item() == 0 and torch.isnan(loss).all(), "a refused call launched"
