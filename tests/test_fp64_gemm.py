"""tests/fp64_gemm.py pinned on the CPU: `ref_group` against torch.nn.functional.linear and the oracle's LinearRS (forward and
autograd, 1e-12), `ref_split(split6)` against `ref_group` at the float32 class, `planes` exactly."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_gemm as fg  # noqa: E402
import fp64_ops as fo  # noqa: E402

from oracle import e3 as oe3  # noqa: E402
from oracle import nets as onets  # noqa: E402


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _flat(ar, name, t, pad=8):
    """tensor t as a buffer of the arena (values rounded to float32); returns (name, offset)"""
    off = ar.alloc(name, t.numel(), pad)
    ar.bufs[name][off:off + t.numel()] = t.reshape(-1).float()
    return (name, off)


def test_ref_group_is_nn_linear_and_its_autograd():
    """forward = kind 1 (weight [N,K]) with bias, data gradient = kind 0, weight + bias gradient = kind 3 with column sums"""
    g = torch.Generator().manual_seed(0)
    M, K, N = 37, 29, 13
    x, W, b, dy = (fo.f32r(torch.randn(s, generator=g, dtype=torch.float64)) for s in ((M, K), (N, K), (N,), (M, N)))
    xr, Wr, br = (t.clone().requires_grad_(True) for t in (x, W, b))
    y = torch.nn.functional.linear(xr, Wr, br)
    dx, dW, db = torch.autograd.grad(y, [xr, Wr, br], dy)
    ar = fg.Arena(1)
    X, Wb, Bb, DY = _flat(ar, "x", x), _flat(ar, "W", W), _flat(ar, "b", b), _flat(ar, "dy", dy)
    Y = ("y", ar.alloc("y", M * N))
    DX = ("dx", ar.alloc("dx", M * K))
    DW = ("dW", ar.alloc("dW", N * K))
    DB = ("db", ar.alloc("db", N))
    dW0 = ar.bufs["dW"][DW[1]:DW[1] + N * K].double().view(N, K)
    db0 = ar.bufs["db"][DB[1]:DB[1] + N].double()
    probs = [fg.Prob(1, X, (1, K, 0), Wb, K, Y, (1, N, 0), Bb, M, N, K),
             fg.Prob(0, DY, (1, N, 0), Wb, K, DX, (1, K, 0), None, M, K, N),
             fg.Prob(3, DY, (1, N, 0), X, K, DW, (1, K, 0), DB, N, K, M)]
    r = fg.ref_group(probs, ar.bufs)
    assert _rel(r.exp["y"][Y[1]:Y[1] + M * N].view(M, N), y.detach()) < 1e-12
    assert _rel(r.exp["dx"][DX[1]:DX[1] + M * K].view(M, K), dx) < 1e-12
    assert _rel(r.exp["dW"][DW[1]:DW[1] + N * K].view(N, K) - dW0, dW) < 1e-12   # the tn kinds add to what is there
    assert _rel(r.exp["db"][DB[1]:DB[1] + N] - db0, db) < 1e-12
    for name in ("y", "dx", "dW", "db"):  # nothing outside the outputs is marked or changed
        w = r.written[name]
        assert int(w.sum()) == {"y": M * N, "dx": M * K, "dW": N * K, "db": N}[name]
        assert torch.equal(r.exp[name][~w], ar.bufs[name].double()[~w])


def _pairs(si, so):
    """(l, in_off, K, out_off, N, w_off) of a LinearRS between two row layouts: equal degree AND parity, weights in the
    order of the input segments, each [K, N] (e3nn's flat tp.weight)"""
    pairs, w_off = [], 0
    for (K, l), par, in_off in zip(si.segs, si.par, si.offsets):
        for (N, lo), paro, out_off in zip(so.segs, so.par, so.offsets):
            if (lo, paro) == (l, par):
                pairs.append((l, in_off, K, out_off, N, w_off))
                w_off += K * N
    return pairs, w_off


@pytest.mark.parametrize("irr_in,irr_out", [("16x0e+8x1e+4x2e", "12x0e+6x1e+5x2e"),
                                             ("8x0e+4x0o+6x1o+3x2e", "5x0e+7x0o+2x1o+3x2e"),
                                             ("6x0e+5x1e+4x2e+3x3e", "9x0e+2x2e")])
def test_ref_group_is_linear_rs_and_its_autograd(irr_in, irr_out):
    """the per-degree problems of a LinearRS in the row layout ([2l+1][mul] segments, two-level rows) against the oracle
    module in the e3nn layout: forward (kind 0, bias on 0e only), data gradient (kind 1), weight gradient (kind 2 with the
    column sums of the 0e pair as the bias gradient)"""
    torch.manual_seed(4)
    ref = onets.LinearRS(oe3.Irreps(irr_in), oe3.Irreps(irr_out)).double()
    for b in ref.bias:
        b.data.normal_()
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(fo.f32r(p))
    si, so = fo.Segs(irr_in), fo.Segs(irr_out)
    n = 11
    g = torch.Generator().manual_seed(5)
    x = fo.f32r(torch.randn(n, si.dim, generator=g, dtype=torch.float64)).requires_grad_(True)
    dy = fo.f32r(torch.randn(n, so.dim, generator=g, dtype=torch.float64))
    y = ref(x)
    params = list(ref.parameters())
    grads = torch.autograd.grad(y, [x] + params, dy)
    weight = ref.tp.weight.detach()
    pairs, wn = _pairs(si, so)
    assert wn == weight.numel()
    ar = fg.Arena(6)
    X = _flat(ar, "x", x.detach()[:, si.perm_from_e3nn()])
    DY = _flat(ar, "dy", dy[:, so.perm_from_e3nn()])
    Wb = _flat(ar, "w", weight)
    Bb = _flat(ar, "b", ref.bias[0].detach()) if len(ref.bias) else None
    Y, DX, DW = ("y", ar.alloc("y", n * so.dim)), ("dx", ar.alloc("dx", n * si.dim)), ("dw", ar.alloc("dw", wn))
    DB = ("db", ar.alloc("db", ref.bias[0].numel())) if len(ref.bias) else None
    init = {k: v.double().clone() for k, v in ar.bufs.items()}
    probs = []
    for (l, in_off, K, out_off, N, w_off) in pairs:
        d = 2 * l + 1
        ra, rc = (d, si.dim, K), (d, so.dim, N)
        j = [s for s in range(len(so.segs)) if so.offsets[s] == out_off][0]
        has_b = Bb is not None and so.scalar(j)
        A, Bw, C = (X[0], X[1] + in_off), (Wb[0], Wb[1] + w_off), (Y[0], Y[1] + out_off)
        probs.append(fg.Prob(0, A, ra, Bw, N, C, rc, Bb if has_b else None, n * d, N, K))
        probs.append(fg.Prob(1, (DY[0], DY[1] + out_off), rc, Bw, N, (DX[0], DX[1] + in_off), ra, None, n * d, K, N))
        probs.append(fg.Prob(2, A, ra, (DY[0], DY[1] + out_off), N, (DW[0], DW[1] + w_off), rc, DB if has_b else None,
                             K, N, n * d))
    r = fg.ref_group(probs, ar.bufs)

    def rows(name, h, dim, segs, zero_uncovered):
        t = r.exp[name][h[1]:h[1] + n * dim].view(n, dim).clone()
        w = r.written[name][h[1]:h[1] + n * dim].view(n, dim)
        if zero_uncovered:
            t[~w] = 0.0  # a segment no pair writes: the modules return zeros there
        inv = torch.empty(dim, dtype=torch.long)
        inv[segs.perm_from_e3nn()] = torch.arange(dim)
        return t[:, inv]

    assert _rel(rows("y", Y, so.dim, so, True), y.detach()) < 1e-12
    assert _rel(rows("dx", DX, si.dim, si, True), grads[0]) < 1e-12
    names = [k for k, _ in ref.named_parameters()]
    gw = grads[1 + names.index("tp.weight")]
    assert _rel(r.exp["dw"][DW[1]:DW[1] + wn] - init["dw"][DW[1]:DW[1] + wn], gw) < 1e-12
    if DB is not None:
        gb = grads[1 + names.index("bias.0")]
        assert _rel(r.exp["db"][DB[1]:DB[1] + gb.numel()] - init["db"][DB[1]:DB[1] + gb.numel()], gb) < 1e-12


def test_planes_are_exact_bf16_and_sum_to_the_value():
    g = torch.Generator().manual_seed(7)
    x = torch.cat([torch.randn(4096, generator=g) * 10.0 ** torch.randint(-30, 30, (4096,), generator=g).float(),
                   fg.operands("ties", 64, 16, 4, g)[0].reshape(-1), torch.tensor([0.0, -0.0, 1.0, 2.0 ** -126])])
    p = fg.planes(x, 3)
    for q in p:
        assert torch.equal(q.bfloat16().float(), q)  # every plane survives the round trip through bf16
    assert torch.equal((p[0].double() + p[1].double() + p[2].double()).float(), x)  # 24 bits of x fit in three planes
    assert torch.equal(p[0], x.bfloat16().float())
    # a tie goes to the even neighbour: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    t = fg.planes(torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8]), 2)
    assert t[0].tolist() == [1.0, 1.0 + 2.0 ** -6] and t[1].tolist() == [2.0 ** -8, -(2.0 ** -8)]


@pytest.mark.parametrize("family", ["randn", "scaled"])
def test_ref_split6_is_float32_class(family):
    """3 + 3 planes, 6 products drop only terms below 2^-24 of a product: within 1e-6 per row of the float64 contraction
    (64 terms; the dropped terms are at most 3 * 2^-24 = 1.8e-7 of sum |a||b|), for all four kinds"""
    ar = fg.Arena(8)
    probs = [fg.add_problem(ar, "p%d" % k, k, 45, 37, 64, d=3 if k != 1 else 1, family=family, accumulate=k == 1)
             for k in range(4)]
    r, s = fg.ref_group(probs, ar.bufs), fg.ref_split(probs, ar.bufs, "split6")
    for n, what, name, ix in r.outs:
        assert fo.per_row_rel(s.exp[name][ix], r.exp[name][ix]) < 1e-6, (n, what)
        assert torch.equal(s.written[name], r.written[name])
    # ... and the two-plane modes are not: the yardstick tells the modes apart
    b = fg.ref_split(probs, ar.bufs, "bf16")
    n, what, name, ix = r.outs[-1]
    assert fo.per_row_rel(b.exp[name][ix], r.exp[name][ix]) > 1e-4


def test_untouched_regions_of_a_two_level_problem():
    """gaps between degree rows (inner > N), after a node's rows (ld > d * inner), rows past M and the guard bands are not
    marked as written, and the written count is exactly M * N"""
    ar = fg.Arena(9)
    p = fg.add_problem(ar, "p", 0, 3 * 13, 33, 29, d=3, ipad=2, lpad=4, c_off=2)
    r = fg.ref_group([p], ar.bufs)
    w = r.written["p.C"]
    assert int(w.sum()) == 39 * 33 and not w[:fg.GUARD + 2].any() and not w[-fg.GUARD:].any()
    assert p.rc == (3, 3 * 35 + 4, 35)
    row0 = fg.GUARD + 2
    assert w[row0:row0 + 33].all() and not w[row0 + 33:row0 + 35].any() and w[row0 + 35]
    assert not w[row0 + 3 * 35:row0 + 3 * 35 + 4].any()
    with pytest.raises(AssertionError):  # a problem that reaches into a guard band is refused before it can run
        fg.ref_group([fg.Prob(0, p.A, p.ra, p.B, p.ldb, p.C, p.rc, None, p.M + 6, p.N, p.K)], ar.bufs)
    with pytest.raises(AssertionError):  # K <= 0 in a rows kind is an argument error
        fg.ref_group([fg.Prob(0, p.A, p.ra, p.B, p.ldb, p.C, p.rc, None, p.M, p.N, 0)], ar.bufs)
