"""The float64 restatements of tests/fp64_norms.py (graph norm, instance norm) pinned three ways on the CPU:
hand-computed answers that depend on no code, the reference's own EquivariantGraphNorm / EquivariantInstanceNorm /
EquivariantLayerNormFast classes run through oracle/refshim (values and every gradient, 1e-12, ragged batches; skipped
where there is no reference checkout), and the model fixtures of tests/golden/norms/ against a fresh run of the
reference's model classes (1e-9)."""
import math
import os
import sys
import warnings

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import fp64_norms as fn  # noqa: E402
import fp64_ops as fo  # noqa: E402
from oracle.refshim import reference_available  # noqa: E402

warnings.filterwarnings("ignore", category=FutureWarning)
needs_reference = pytest.mark.skipif(not reference_available(), reason="no reference checkout on this machine")
EPS = 1e-5
D = torch.float64


def _t(v):
    return torch.tensor(v, dtype=D)


# ------------------------------------------------------------------------------------------------- hand known answers
def test_scalar_pair_mean_shift_one():
    """1x0e, one graph, x = [1, 3], mean_shift 1: mu = 2, c = [-1, 1], v = 1, y = -+w / sqrt(1 + eps) + b"""
    w, b = 1.7, 0.3
    y = fn.graph_norm(_t([[1.0], [3.0]]), _t([1.0]), _t([w]), _t([b]), "1x0e", [0, 2], EPS)
    r = w / math.sqrt(1.0 + EPS)
    assert torch.allclose(y, _t([[-r + b], [r + b]]), rtol=0, atol=1e-15)
    yi = fn.instance_norm(_t([[1.0], [3.0]]), _t([w]), _t([b]), "1x0e", [0, 2], EPS)
    assert torch.equal(y, yi)


def test_scalar_pair_mean_shift_half():
    """the same input with mean_shift 0.5: c = x - 0.5 * 2 = [0, 2], v = (0 + 4) / 2 = 2"""
    w, b = 1.7, 0.3
    y = fn.graph_norm(_t([[1.0], [3.0]]), _t([0.5]), _t([w]), _t([b]), "1x0e", [0, 2], EPS)
    assert torch.allclose(y, _t([[b], [2.0 * w / math.sqrt(2.0 + EPS) + b]]), rtol=0, atol=1e-15)


def test_vector_segment_is_scaled_not_centred():
    """1x1e, one graph of two nodes (1, 2, 2) and (0, 0, 0): v = 9 / (2 * 3) = 1.5; no mean, no bias"""
    w = 0.8
    x = _t([[1.0, 2.0, 2.0], [0.0, 0.0, 0.0]])
    y = fn.graph_norm(x, _t([]), _t([w]), _t([]), "1x1e", [0, 2], EPS)
    assert torch.allclose(y, x * w / math.sqrt(1.5 + EPS), rtol=0, atol=1e-15)
    # a pseudo-scalar is treated the same way: x = [1, 3] -> v = 5, not centred
    y = fn.graph_norm(_t([[1.0], [3.0]]), _t([]), _t([w]), _t([]), "1x0o", [0, 2], EPS)
    assert torch.allclose(y, _t([[1.0], [3.0]]) * w / math.sqrt(5.0 + EPS), rtol=0, atol=1e-15)


def test_statistics_do_not_mix_between_graphs():
    """1x0e, graphs [1, 3] and [10, 10, 16] (and an empty one between them): the second has mu = 12, c = (-2, -2, 4),
    v = 8; the first keeps the answer it has alone"""
    x = _t([[1.0], [3.0], [10.0], [10.0], [16.0]])
    y = fn.instance_norm(x, _t([1.0]), _t([0.0]), "1x0e", [0, 2, 2, 5], EPS)
    r1, r2 = 1.0 / math.sqrt(1.0 + EPS), 1.0 / math.sqrt(8.0 + EPS)
    assert torch.allclose(y, _t([[-r1], [r1], [-2 * r2], [-2 * r2], [4 * r2]]), rtol=0, atol=1e-15)
    # one graph of all five nodes is something else: mu = 8
    y1 = fn.instance_norm(x, _t([1.0]), _t([0.0]), "1x0e", [0, 5], EPS)
    assert float((y1 - y).abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------- the reference's classes
IRREPS = ["8x0e+4x1e+2x2e", "8x0e+2x0o+4x1e+4x1o", "5x0e", "3x1e+2x2e"]
SIZES = [1, 2, 7, 3, 1, 12]


def _case(irr, seed):
    seg = fo.Segs(irr)
    g = torch.Generator().manual_seed(seed)
    n = sum(SIZES)
    nw = sum(mul for mul, _ in seg.segs)
    nb = sum(mul for s, (mul, _) in enumerate(seg.segs) if seg.scalar(s))
    x = torch.randn(n, seg.dim, generator=g, dtype=D) + 3.0
    ms = torch.rand(nb, generator=g, dtype=D) + 0.5
    w = 1.0 + 0.5 * torch.randn(nw, generator=g, dtype=D)
    b = torch.randn(nb, generator=g, dtype=D)
    go = torch.randn(n, seg.dim, generator=g, dtype=D)
    ptr = [0]
    for s in SIZES:
        ptr.append(ptr[-1] + s)
    batch = torch.repeat_interleave(torch.arange(len(SIZES)), torch.tensor(SIZES))
    return seg, x, ms, w, b, go, ptr, batch


def _close(a, b, what):
    err = float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30) if b.numel() else 0.0
    assert err < 1e-12, (what, err)


@needs_reference
@pytest.mark.parametrize("irr", IRREPS)
@pytest.mark.parametrize("kind", ["graph", "instance", "fast_layer"])
def test_restatement_equals_the_reference_class(irr, kind):
    from oracle.refshim import load_reference_nets
    load_reference_nets()
    from nets.fast_layer_norm import EquivariantLayerNormFast
    from nets.graph_norm import EquivariantGraphNorm
    from nets.instance_norm import EquivariantInstanceNorm
    seg, x, ms, w, b, go, ptr, batch = _case(irr, 5)
    perm = seg.perm_from_e3nn()  # x_rows = x_e3nn[:, perm]
    inv = torch.argsort(perm)
    cls = dict(graph=EquivariantGraphNorm, instance=EquivariantInstanceNorm, fast_layer=EquivariantLayerNormFast)[kind]
    ref = cls(irr).double()
    with torch.no_grad():
        ref.affine_weight.copy_(w)
        ref.affine_bias.copy_(b)
        if kind == "graph":
            ref.mean_shift.copy_(ms)
    xe = x[:, inv].clone().requires_grad_(True)
    ye = ref(xe, batch=batch)
    ye.backward(go[:, inv])
    leaves = [t.clone().requires_grad_(True) for t in (x, ms, w, b)]
    if kind == "graph":
        y = fn.graph_norm(leaves[0], leaves[1], leaves[2], leaves[3], seg, ptr, EPS)
    elif kind == "instance":
        y = fn.instance_norm(leaves[0], leaves[2], leaves[3], seg, ptr, EPS)
    else:
        y = fo.layer_norm(leaves[0], leaves[2], leaves[3], seg, EPS)
    y.backward(go)
    _close(y.detach(), ye.detach()[:, perm], "y")
    _close(leaves[0].grad, xe.grad[:, perm], "dx")
    _close(leaves[2].grad, ref.affine_weight.grad, "d_weight")
    if b.numel():
        _close(leaves[3].grad, ref.affine_bias.grad, "d_bias")
    if kind == "graph" and b.numel():
        _close(leaves[1].grad, ref.mean_shift.grad, "d_mean_shift")


def test_add_variants_are_the_norm_of_the_sum():
    seg, x, ms, w, b, go, ptr, _ = _case("8x0e+4x1e+2x2e", 6)
    a = 0.25 * x
    y, s = fn.add_graph_norm(a, x - a, ms, w, b, seg, ptr, EPS)
    assert torch.equal(s, a + (x - a)) and torch.equal(y, fn.graph_norm(s, ms, w, b, seg, ptr, EPS))
    y, s = fn.add_instance_norm(a, x - a, w, b, seg, ptr, EPS)
    assert torch.equal(y, fn.instance_norm(s, w, b, seg, ptr, EPS))


# ------------------------------------------------------------------------------------------------- the model fixtures
@needs_reference
def test_model_fixtures_equal_a_fresh_reference_run():
    import make_norm_golden as mng
    errs = mng.check(log=lambda *a: None)
    assert {t for t, _ in errs} == {"qm9_graph", "qm9_instance", "md17_graph"}
    bad = {k: v for k, v in errs.items() if v > 1e-9}
    assert not bad, bad
