"""eqf_meter_fold (csrc/meters.hip) through `train.RunningMeters` and through the C ABI: the fp64 (sum, count) pairs equal the
reference's AverageMeter (engine.py:23-27) fed the same fp32 values, bit for bit -- the products of an fp32 value and an
integer weight below 2^29 are exact in fp64, so both sides round the same additions in the same order.  Eager folds, and one
captured fold replayed with new stats before every replay; a skipped meter (weight 0) does not read its NaN value; argument
errors return a status and leave acc as it was."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
N_STATS = 24  # 0..11: values, 12..23: counts (some 0)
FOLDS = 7


class AverageMeter:
    """engine.py:12-27"""

    def __init__(self):
        self.sum, self.count = 0, 0

    def update(self, val, n=1):
        self.sum += val * n
        self.count += n


def _spec(M, seed):
    """M meters: values from stats or the loss, weights from the counts of stats, the graph count or 1"""
    from equiformer_amd import train
    g = torch.Generator().manual_seed(seed)
    spec = []
    for i in range(M):
        v = train.LOSS if i % 5 == 1 else int(torch.randint(0, 12, (1,), generator=g))
        w = (train.GRAPHS, train.ONE, int(torch.randint(12, 24, (1,), generator=g)))[i % 3]
        spec.append(("m%d" % i, v, w))
    return spec


def _inputs(seed):
    """FOLDS x (stats [24] fp32, loss fp32, graph count): values over many binades, counts below 2^24 with zeros among them"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(FOLDS):
        vals = torch.randn(12, generator=g) * torch.exp2(torch.randint(-20, 21, (12,), generator=g).float())
        counts = torch.randint(0, 1 << 20, (12,), generator=g).float()
        counts[torch.rand(12, generator=g) < 0.3] = 0.0
        loss = (torch.randn((), generator=g) * 1e3).float()
        graphs = int(torch.randint(1, (1 << 29) - 1, (1,), generator=g)) if k % 2 else int(torch.randint(1, 64, (1,), generator=g))
        out.append((torch.cat([vals, counts]).float(), loss, graphs))
    return out


def _restated(spec, inputs):
    from equiformer_amd import train
    meters = [AverageMeter() for _ in spec]
    for stats, loss, graphs in inputs:
        s = stats.tolist()  # (fp32 values, exactly as Python floats)
        for m, (_, v, w) in zip(meters, spec):
            n = graphs if w == train.GRAPHS else (1 if w == train.ONE else s[w])
            if n == 0:  # the reference's `if not loss_f.isnan()`
                continue
            m.update(float(loss) if v == train.LOSS else s[v], n)
    return torch.tensor([x for m in meters for x in (float(m.sum), float(m.count))], dtype=torch.float64)


def _bits_equal(got, want):
    got = got.detach().cpu()
    return torch.equal(got.view(torch.int64), want.view(torch.int64))


@pytest.mark.parametrize("M", [1, 6, 16])
def test_fold_equals_average_meter_bit_for_bit(M):
    from equiformer_amd import train
    spec = _spec(M, seed=M)
    inputs = _inputs(seed=100 + M)
    meters = train.RunningMeters(spec, DEV)
    stats = torch.zeros(N_STATS, dtype=torch.float32, device=DEV)
    loss = torch.zeros((), dtype=torch.float32, device=DEV)
    # eager
    for s, l, graphs in inputs:
        stats.copy_(s)
        loss.copy_(l)
        meters.fold(stats, loss, graphs)
    want = _restated(spec, inputs)
    got = meters.acc.cpu()
    print("M=%d eager: %s" % (M, got.tolist()[:4]))
    assert _bits_equal(got, want), (got, want)
    assert all(c > 0 for c in want.tolist()[1::2]) or M == 1, "every meter should have moved"
    # captured once, replayed FOLDS times with new stats (the graph count is the one of the capture)
    meters.reset()
    stats.copy_(inputs[0][0])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        meters.fold(stats, loss, inputs[0][2])
    torch.cuda.synchronize()
    assert meters.acc.abs().sum().item() == 0.0, "the capture ran the fold"
    for s, l, _ in inputs:
        stats.copy_(s)
        loss.copy_(l)
        graph.replay()
    frozen = [(s, l, inputs[0][2]) for s, l, _ in inputs]
    got = meters.acc.cpu()
    assert _bits_equal(got, _restated(spec, frozen))


def test_skipped_meter_does_not_read_its_value():
    from equiformer_amd import train
    spec = [("a", 0, 2), ("b", 1, 3), ("c", train.LOSS, 2), ("d", 4, train.ONE)]
    meters = train.RunningMeters(spec, DEV)
    stats = torch.tensor([float("nan"), 2.5, 0.0, 3.0, 0.75], device=DEV)
    loss = torch.tensor(float("nan"), device=DEV)
    for _ in range(3):
        meters.fold(stats, loss)
    got = meters.acc.cpu().tolist()
    assert got == [0.0, 0.0, 22.5, 9.0, 0.0, 0.0, 2.25, 3.0], got  # a and c untouched: NaN values under weight 0


def test_argument_errors_write_nothing(hip_lib):
    f = hip_lib.eqf_meter_fold
    acc = torch.full((8,), 1.25, dtype=torch.float64, device=DEV)
    stats = torch.ones(6, device=DEV)
    loss = torch.ones((), device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    I4, D4 = ctypes.c_int * 4, ctypes.c_double * 4
    vi, wi, wc = (0, -1, 5, 2), (-1, 3, 4, -1), (3.0, 0.0, 0.0, 1.0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fold(stats_=P(stats), n=6, loss_=P(loss), M=4, vi_=vi, wi_=wi, wc_=wc):
        return f(stats_, n, loss_, M, I4(*vi_), I4(*wi_), D4(*wc_), P(acc), stream)
    bad = [fold(M=0), fold(M=17), fold(n=5), fold(vi_=(0, -2, 5, 2)), fold(wi_=(-1, 6, 4, -1)), fold(stats_=None),
           fold(loss_=None), fold(wc_=(2.5, 0.0, 0.0, 1.0)), fold(wc_=(float(1 << 29), 0.0, 0.0, 1.0)),
           fold(wc_=(-3.0, 0.0, 0.0, 1.0)), f(P(stats), 6, P(loss), 4, I4(*vi), I4(*wi), D4(*wc), None, stream)]
    torch.cuda.synchronize()
    assert bad == [-1] * len(bad), bad
    assert acc.cpu().tolist() == [1.25] * 8, "a refused call wrote acc"
    assert fold() == 0
    torch.cuda.synchronize()
    assert acc.cpu().tolist() == [1.25 + 3.0, 1.25 + 3.0, 1.25 + 1.0, 1.25 + 1.0, 1.25 + 1.0, 1.25 + 1.0, 1.25 + 1.0, 1.25 + 1.0]
