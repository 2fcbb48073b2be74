"""Identities between the linear operators that share one autograd Function triple (ops._Linear) or one set of descriptor
builders, on the shapes of tests/linear_trace.py (5 rows), in the matrix modes split and fp32:

  * irreps_linear_pair == two irreps_linear calls (forward, weight and bias gradients; its dx == the sum of theirs);
  * dense_linear(x, W, b) == grouped_linear(x, K, [W], [b], wide=True), for a contiguous x and for a column block read in place;
  * columns of an output (of dx) that no degree pair of the plan covers are exactly 0.0, whatever the allocator hands out.

Everything is compared with torch.equal: the descriptors on both sides are the same, and the weight / bias gradients are ONE
atomic add onto zero each -- with at most 25 reduction rows (5 rows x 5 components) both back ends take a single K split
(gemm.hip / gemmx.hip: ksplit <= ceil(steps / 8), and 25 rows are at most 2 steps).
Wall time of this file on an MI355X, one run each (pytest's figure): 3.1 s at the parent commit, 3.3 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py)."""
import pytest
import torch

from equiformer_amd import ops
from equiformer_amd.layout import RowLayout
from poison import poisoned_ops  # noqa: E402,F401  (every launch of this file runs on poisoned, guarded allocations)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_ops")]
MODES = ["split", "fp32"]
ROWS = 5
FULL = "8x0e+4x1e+4x2e"


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rand(g, *shape):
    return torch.randn(*shape, generator=g).to(_dev()).requires_grad_(True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("bias_second", [True, False])
def test_pair_equals_two_linears(mode, bias_second):
    g = torch.Generator().manual_seed(1)
    li = RowLayout(FULL)
    s1, s2 = ops.LinearSpec(li, RowLayout(FULL)), ops.LinearSpec(li, RowLayout("8x0e+4x1e"))
    x = _rand(g, ROWS, li.dim)
    w1, w2, b1 = _rand(g, s1.weight_numel), _rand(g, s2.weight_numel), _rand(g, s1.bias_dim)
    b2 = _rand(g, s2.bias_dim) if bias_second else None
    c1, c2 = _rand(g, ROWS, s1.out_layout.dim).detach(), _rand(g, ROWS, s2.out_layout.dim).detach()
    params = [p for p in (w1, b1, w2, b2) if p is not None]
    with ops.matrix_mode(mode):
        y1, y2 = ops.irreps_linear_pair(x, w1, b1, s1, w2, b2, s2)
        got = torch.autograd.grad([y1, y2], [x] + params, [c1, c2])
        z1, z2 = ops.irreps_linear(x, w1, b1, s1), ops.irreps_linear(x, w2, b2, s2)
        dx1, dw1, db1 = torch.autograd.grad(z1, [x, w1, b1], c1)
        ref2 = torch.autograd.grad(z2, [x, w2] + ([b2] if bias_second else []), c2)
    assert torch.equal(y1, z1) and torch.equal(y2, z2)
    assert torch.equal(got[0], dx1.clone().add_(ref2[0]))
    for a, b in zip(got[1:], (dw1, db1) + tuple(ref2[1:])):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("block", [None, 16])
def test_dense_equals_a_grouped_linear_with_one_group(mode, block):
    g = torch.Generator().manual_seed(2)
    K, N = 8, 12
    W, b, c = _rand(g, N, K), _rand(g, N), _rand(g, ROWS, N).detach()
    res = []
    for op in ("dense", "grouped"):
        if block is None:
            leaf = _rand(torch.Generator().manual_seed(3), ROWS, K)
            x = leaf
        else:  # a column block with row stride and offset multiples of 4: dense_linear reads it in place
            leaf = _rand(torch.Generator().manual_seed(3), ROWS, block)
            x = leaf[:, 4:4 + K]
        with ops.matrix_mode(mode):
            y = ops.dense_linear(x, W, b) if op == "dense" else ops.grouped_linear(x, K, [W], [b], wide=True)
            res.append((y,) + torch.autograd.grad(y, [leaf, W, b], c))
    for a, r in zip(*res):
        assert a.shape == r.shape and torch.equal(a, r)
    xd = (res[0][1] if block is None else res[0][1][:, 4:4 + K]).double()
    assert torch.allclose(xd, c.double() @ W.detach().double(), rtol=0, atol=1e-3)  # (the block's dx landed in its columns)
    if block is not None:
        assert float(res[0][1][:, :4].abs().max()) == 0.0 and float(res[0][1][:, 4 + K:].abs().max()) == 0.0


def _dirty(shape):
    """leave a freed block of this size full of NaN at the head of the allocator's free list"""
    t = torch.full(shape, float("nan"), device=_dev())
    torch.cuda.synchronize()
    del t


@pytest.mark.parametrize("mode", MODES)
def test_uncovered_columns_are_exactly_zero(mode):
    g = torch.Generator().manual_seed(4)
    small, full = RowLayout("8x0e+4x1e"), RowLayout(FULL)
    up, down = ops.LinearSpec(small, full), ops.LinearSpec(full, small)
    assert not up.out_covered and up.in_covered and down.out_covered and not down.in_covered
    with ops.matrix_mode(mode):
        x, w = _rand(g, ROWS, small.dim), _rand(g, up.weight_numel)
        _dirty((ROWS, full.dim))
        y = ops.irreps_linear(x, w, None, up).detach()
        assert torch.equal(y[:, small.dim:], torch.zeros(ROWS, full.dim - small.dim, device=_dev()))
        assert bool(torch.isfinite(y).all()) and float(y[:, :small.dim].abs().max()) > 0
        x, w = _rand(g, ROWS, full.dim), _rand(g, down.weight_numel)
        z = ops.irreps_linear(x, w, None, down)
        c = torch.randn(ROWS, small.dim, generator=g).to(_dev())
        _dirty((ROWS, full.dim))
        (dx,) = torch.autograd.grad(z, [x], c)
        assert torch.equal(dx[:, small.dim:], torch.zeros(ROWS, full.dim - small.dim, device=_dev()))
        assert bool(torch.isfinite(dx).all()) and float(dx[:, :small.dim].abs().max()) > 0
