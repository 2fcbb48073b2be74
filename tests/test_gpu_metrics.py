"""eqf_metrics_accumulate (csrc/metrics.hip) alone, on the GPU, against an fp64 torch restatement on the SAME fp32 predictions.

Bounds.  The kernel and the restatement form every term in fp64 from the same fp32 inputs; what separates them is the order of
the summation (and an fma the compiler may contract).  A sum of n non-negative fp64 terms is within n 2^-53 relative of the exact
sum in any order; the largest sum here has 3 (4 W + 3) = 3 081 < 10^4 terms: 10^4 2^-53 < 1.2e-12, so the bound is 1e-12 relative.
Counts (graphs, atoms, errors under the threshold) are exact: the targets are drawn so that no |e| of the restatement lies
within 1e-9 of the threshold (asserted), twelve orders of magnitude above what the two sides can differ by.
Wall time of this file on an MI355X, one run each (pytest's figure): 2.5 s at the parent commit, 2.4 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py)."""
import pytest
import torch
from poison import guard_input, poisoned_ops  # noqa: E402,F401  (the fixture of the tests that run on poisoned, guarded allocations)

pytestmark = pytest.mark.gpu

W = 256  # the kernel's workgroup (ops.METRICS_THREADS, asserted below)
MEAN, STD, THR = 5.0, 1.7, 0.02
GRAPHS = (1, 63, 64, 65, W - 1, W, W + 1)
NODES = (0, 1, 63, 64, 65, W - 1, W, W + 1, 4 * W + 3)
COUNTS = (0, 4, 5)  # graphs, errors under the threshold, atoms


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _case(n_graphs, N, seed, flip=0):
    """fp32 CPU tensors: pred_y, y [n_graphs + 1], pred_dy, dy [N, 3], mask [N] with a third of the rows phantom.  Row b's error
    is drawn inside the threshold when (b + flip) is even, outside otherwise."""
    g = torch.Generator().manual_seed(seed)
    rows = n_graphs + 1
    pred_y = torch.randn(rows, generator=g)
    inside = (torch.arange(rows) + flip) % 2 == 0
    mag = torch.where(inside, 0.1 + 0.8 * torch.rand(rows, generator=g, dtype=torch.float64),
                      1.5 + 50.0 * torch.rand(rows, generator=g, dtype=torch.float64)) * THR
    sign = torch.where(torch.rand(rows, generator=g) < 0.5, -1.0, 1.0).double()
    y = (pred_y.double() * STD + MEAN - sign * mag).float()
    pred_dy, dy = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g) * 2
    mask = (torch.rand(N, generator=g) > 0.33).float()
    return pred_y, y, pred_dy, dy, mask


def _ref(pred_y, y, n_graphs, pred_dy=None, dy=None, mask=None, check_threshold=True):
    """the ten sums in plain torch fp64 from the fp32 inputs (CPU)"""
    p, t = pred_y.double().reshape(-1)[:n_graphs], y.double().reshape(-1)[:n_graphs]
    e = p * STD + MEAN - t
    if check_threshold:
        assert float((e.abs() - THR).abs().min()) > 1e-9  # no error within 1e-9 of the threshold: the count is well defined
    out = [float(n_graphs), float((p - (t - MEAN) / STD).abs().sum()), float(e.abs().sum()), float((e * e).sum()),
           float((e.abs() < THR).sum())]
    if pred_dy is None or pred_dy.shape[0] == 0:
        return out + [0.0] * 5
    keep = torch.ones(pred_dy.shape[0], dtype=torch.bool) if mask is None else mask != 0
    pd, d = pred_dy.double()[keep], dy.double()[keep]
    a, r = pd - d / STD, pd * STD - d
    return out + [float(keep.sum()), float(a.norm(dim=1).sum()), float(a.abs().sum()), float(r.abs().sum()), float((r * r).sum())]


def _assert_sums(got, want, what):
    for q, (a, b) in enumerate(zip(got, want)):
        if q in COUNTS or b == 0.0:
            assert a == b, (what, q, a, b)
        else:
            assert abs(a - b) <= 1e-12 * abs(b), (what, q, a, b, abs(a - b) / abs(b))


def _run(meter, pred_y, y, n_graphs, pred_dy=None, dy=None, mask=None, reset=True):
    dev = _dev()
    if reset:
        meter.reset()
    mv = lambda t: None if t is None else guard_input(t.to(dev))  # noqa: E731  (NaN right behind the last row: tests/poison.py)
    meter.update(mv(pred_y), mv(y), n_graphs, mv(pred_dy), mv(dy), mv(mask))
    return meter.acc.clone()


@pytest.fixture(scope="module")
def meter():
    from equiformer_amd import ops
    from equiformer_amd.evaluate import Meter
    assert ops.METRICS_THREADS == W
    return Meter(MEAN, STD, THR, device=_dev())


@pytest.mark.usefixtures("poisoned_ops")
@pytest.mark.parametrize("n_graphs", GRAPHS)
def test_sums_against_fp64_at_every_size(meter, n_graphs):
    """every n_graphs x N, with and without forces, with and without a mask; rows = n_graphs + 1"""
    inside = outside = False
    worst = 0.0
    for N in NODES:
        for flip in (0, 1):
            pred_y, y, pred_dy, dy, mask = _case(n_graphs, N, seed=1000 * n_graphs + 2 * N + flip, flip=flip)
            for forces, use_mask in ((False, False), (True, False), (True, True)):
                args = (pred_dy, dy, mask if use_mask else None) if forces else (None, None, None)
                want = _ref(pred_y, y, n_graphs, *args)
                got = _run(meter, pred_y, y, n_graphs, *args).tolist()
                _assert_sums(got, want, (n_graphs, N, forces, use_mask))
                worst = max([worst] + [abs(a - b) / abs(b) for a, b in zip(got, want) if b != 0.0])
                inside, outside = inside or want[4] > 0, outside or want[4] < n_graphs
                if forces and use_mask and N >= 63:
                    assert 0 < want[5] < N  # the mask really excludes rows
    assert inside and outside  # errors on both sides of the threshold occurred
    print("n_graphs %d: worst relative deviation of a sum %.2e" % (n_graphs, worst))


def test_a_mask_without_forces_and_energies_of_other_shapes_and_dtypes(meter):
    """[B, 1] predictions, fp64 targets (cast by the meter), a mask handed over without forces: the force terms are skipped"""
    pred_y, y, pred_dy, dy, mask = _case(65, 64, seed=5)
    want = _ref(pred_y, y, 65)
    got = _run(meter, pred_y.view(-1, 1), y.double().view(-1, 1), 65, None, None, mask).tolist()
    _assert_sums(got, want, "shapes")
    want = _ref(pred_y, y, 65, pred_dy, dy, mask)
    got = _run(meter, pred_y, y, 65, pred_dy, dy.double(), mask.double()).tolist()
    _assert_sums(got, want, "dtypes")
    with pytest.raises(ValueError):
        meter.update(pred_y.to(_dev()), y.to(_dev()), 65, pred_dy.to(_dev()), None)
    with pytest.raises(ValueError):
        meter.update(pred_y.to(_dev()), y.to(_dev()), 67)  # more graphs than rows


@pytest.mark.usefixtures("poisoned_ops")
@pytest.mark.parametrize("n_graphs,N", [(1, 1), (65, W + 1), (W + 1, 4 * W + 3)])
def test_nan_and_inf_in_excluded_rows_change_no_bit(meter, n_graphs, N):
    pred_y, y, pred_dy, dy, mask = _case(n_graphs, N, seed=7 + N)
    mask[0] = 1.0
    if N > 1:
        mask[N // 2] = 0.0
    clean = _run(meter, pred_y, y, n_graphs, pred_dy, dy, mask)
    assert bool(torch.isfinite(clean).all())
    phantom = mask == 0
    for bad in (float("nan"), float("inf"), -float("inf")):
        py, yy, pd, d = pred_y.clone(), y.clone(), pred_dy.clone(), dy.clone()
        py[n_graphs:], yy[n_graphs:] = bad, bad
        pd[phantom], d[phantom] = bad, bad
        assert torch.equal(_run(meter, py, yy, n_graphs, pd, d, mask), clean), bad
    # the unmasked run of the same rows is another result (the mask is not decoration) -- when it excludes something
    if int(phantom.sum()):
        assert not torch.equal(_run(meter, pred_y, y, n_graphs, pred_dy, dy, None), clean)


def test_two_launches_accumulate_and_reset_clears(meter):
    a = _case(65, W + 1, seed=11)
    b = _case(W - 1, 63, seed=12, flip=1)
    _run(meter, a[0], a[1], 65, a[2], a[3], a[4])
    got = _run(meter, b[0], b[1], W - 1, b[2], b[3], b[4], reset=False).tolist()
    cat = _ref(torch.cat([a[0][:65], b[0][:W - 1]]), torch.cat([a[1][:65], b[1][:W - 1]]), 65 + W - 1,
               torch.cat([a[2], b[2]]), torch.cat([a[3], b[3]]), torch.cat([a[4], b[4]]))
    _assert_sums(got, cat, "a then b")
    from equiformer_amd.evaluate import SUMS
    sums = meter.read()
    assert list(sums) == list(SUMS) and list(sums.values()) == got
    meter.reset()
    assert meter.acc.tolist() == [0.0] * 10
    # a launch without forces after one with forces leaves the force sums alone
    _run(meter, a[0], a[1], 65, a[2], a[3], a[4])
    before = meter.acc.clone()
    after = _run(meter, b[0], b[1], 1, reset=False)
    assert torch.equal(after[5:], before[5:]) and float(after[0]) == 66.0


def test_repeated_runs_give_identical_bits(meter):
    pred_y, y, pred_dy, dy, mask = _case(W + 1, 4 * W + 3, seed=13)
    first = _run(meter, pred_y, y, W + 1, pred_dy, dy, mask)
    for _ in range(4):
        assert torch.equal(_run(meter, pred_y, y, W + 1, pred_dy, dy, mask), first)
    # the raw operator on a buffer of its own gives the same bits as the meter
    from equiformer_amd import ops
    dev = _dev()
    acc = torch.zeros(10, dtype=torch.float64, device=dev)
    ops.metrics_accumulate(acc, pred_y.to(dev), y.to(dev), W + 1, MEAN, STD, THR, pred_dy.to(dev), dy.to(dev), mask.to(dev))
    assert torch.equal(acc, first)
    with pytest.raises(ValueError):
        ops.metrics_accumulate(acc[:9], pred_y.to(dev), y.to(dev), W + 1, MEAN, STD, THR)
    with pytest.raises(ValueError):
        ops.metrics_accumulate(acc.float(), pred_y.to(dev), y.to(dev), W + 1, MEAN, STD, THR)


def test_update_is_legal_inside_a_stream_capture(meter):
    """enqueue-only: captured once, every replay adds the batch that is in the static inputs then"""
    dev = _dev()
    a = _case(65, W + 1, seed=21)
    b = _case(65, W + 1, seed=22, flip=1)
    static = [t.to(dev).clone() for t in a]
    meter.reset()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        meter.update(static[0], static[1], 65, static[2], static[3], static[4])
    torch.cuda.synchronize()
    assert meter.acc.tolist() == [0.0] * 10  # capturing enqueued nothing
    graph.replay()
    for s, t in zip(static, b):
        s.copy_(t.to(dev))
    graph.replay()
    got = meter.acc.tolist()
    cat = _ref(torch.cat([a[0][:65], b[0][:65]]), torch.cat([a[1][:65], b[1][:65]]), 130,
               torch.cat([a[2], b[2]]), torch.cat([a[3], b[3]]), torch.cat([a[4], b[4]]))
    _assert_sums(got, cat, "two replays")
