"""Device-drawn stochastic depth, the host side (equiformer_amd/droppath.py): the Python restatement of csrc/rng.h against the
published splitmix64 sequence, `keep_factors` (a pure function of seed, call and graph), the `device_draws` scope, and
GraphDropPath outside the scope, which keeps the CPU-generator stream it had.  No GPU."""
import math
import re
import struct
from types import SimpleNamespace

import torch

from equiformer_amd import droppath


def _fp32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def test_mix64_reproduces_the_published_splitmix64_sequence():
    """splitmix64: state += 0x9E3779B97F4A7C15, output = finaliser(state); the first five outputs for state 1234567"""
    want = [6457827717110365317, 3203168211198807973, 9817491932198370423, 4593380528125082431, 16408922859458223821]
    state, got = 1234567, []
    for _ in want:
        state = (state + 0x9E3779B97F4A7C15) & ((1 << 64) - 1)
        got.append(droppath.mix64(state))
    assert got == want
    # the generator of rng.h on top of it: the tag is mixed into the key, the index into the draw
    key = droppath.mix64(7 + 0xD6E8FEB86659FD93 * 33)
    assert droppath.rand_bits(7, 32, 5) == droppath.mix64(key + 0x9E3779B97F4A7C15 * 6)
    u = droppath.rand_uniform(7, 32, 5)
    assert 0.0 <= u < 1.0 and u * 16777216.0 == int(u * 16777216.0) and _fp32(u) == u


def test_keep_factors_pinned_literal():
    """seed 7, p = 0.4, calls 0-3, graphs 0-4: computed from rng.h's formulas"""
    want = [[1, 1, 1, 1, 0], [1, 0, 1, 0, 0], [0, 0, 1, 0, 1], [1, 1, 0, 0, 1]]
    got = [(droppath.keep_factors(7, c, 5, 0.4) > 0).int().tolist() for c in range(4)]
    assert got == want, got


def test_keep_factors_properties():
    p = 0.4
    f = droppath.keep_factors(7, 0, 5, p)
    assert f.dtype == torch.float32 and f.shape == (5,)
    inv = _fp32(1.0 / (1.0 - p))
    for seed in (0, 7, (1 << 64) - 1, 2 ** 62 + 12345):
        for c in (0, 1, 11):
            a, b = droppath.keep_factors(seed, c, 6, p), droppath.keep_factors(seed, c, 7, p)
            assert torch.equal(b[:6], a), "the draw of a graph depends on the number of graphs"
            assert set(b.tolist()) <= {0.0, inv}, b
    assert not torch.equal(droppath.keep_factors(7, 0, 64, p), droppath.keep_factors(7, 1, 64, p)), "two calls, one mask"
    assert not torch.equal(droppath.keep_factors(7, 0, 64, p), droppath.keep_factors(8, 0, 64, p)), "two seeds, one mask"
    assert torch.equal(droppath.keep_factors(7 + (1 << 64), 0, 64, p), droppath.keep_factors(7, 0, 64, p)), "seed mod 2^64"
    assert torch.equal(droppath.keep_factors(3, 2, 9, 0.0), torch.ones(9))
    # the compare is made in fp32, as the kernel makes it: u >= fp32(p)
    us = [droppath.rand_uniform(7, droppath.DROPPATH_TAG, g) for g in range(64)]
    assert (droppath.keep_factors(7, 0, 64, p) > 0).tolist() == [u >= _fp32(p) for u in us]
    # call and graph share one 64-bit index: (call << 32) | graph
    assert droppath.rand_uniform(7, 32, (3 << 32) | 4) >= _fp32(p)  # kept in the literal above: call 3, graph 4
    assert float(droppath.keep_factors(7, 3, 5, p)[4]) == inv


def test_keep_factors_statistics():
    n, p = 4096, 0.25
    share = float((droppath.keep_factors(7, 0, n, p) > 0).double().mean())
    bound = 5 * math.sqrt(p * (1 - p) / n)
    print("kept share %.4f (0.75 +- %.4f)" % (share, bound))
    assert abs(bound - 0.034) < 5e-4 and abs(share - 0.75) <= bound
    assert abs(share - 0.7458) < 5e-5


def test_device_draws_nests_restores_and_counts_from_zero():
    assert droppath.active() is None
    with droppath.device_draws(7) as outer:
        assert droppath.active() is outer and outer.seed == 7 and outer.word is None
        assert [outer.next_call(), outer.next_call()] == [0, 1]
        with droppath.device_draws(9) as inner:
            assert droppath.active() is inner and inner.seed == 9
            assert inner.next_call() == 0, "the counter restarts per entry"
        assert droppath.active() is outer and outer.next_call() == 2, "the outer scope continues its own count"
        try:
            with droppath.device_draws(11):
                raise KeyError("x")
        except KeyError:
            pass
        assert droppath.active() is outer
    assert droppath.active() is None
    with droppath.device_draws(7) as again:
        assert again.next_call() == 0
    # a base seed given as a callable is resolved by the first use only
    seen = []
    word = torch.zeros(1, dtype=torch.int64)  # (a CPU stand-in: the scope only carries it)
    with droppath.device_draws(word, base=lambda: seen.append(1) or 41) as d:
        assert d.word is word and not seen
        assert d.seed == 41 and d.seed == 41 and seen == [1]
    with droppath.device_draws(word) as d:
        assert d.seed == 0


def test_graph_drop_path_outside_the_scope_keeps_its_cpu_generator_stream(monkeypatch):
    """Outside `device_draws` the layer draws what it drew before: one fp64 uniform per graph from torch's CPU generator,
    s = floor(keep + r) / keep.  Inside the scope it consumes nothing and hands (seed, call, word) to the device operator."""
    from equiformer_amd.nets import layers
    calls = []
    monkeypatch.setattr(layers.ops, "segment_scale", lambda x, s, seg: calls.append(s) or x)
    monkeypatch.setattr(layers.droppath, "segment_droppath", lambda x, seg, p, seed, call, word: calls.append((p, seed, call, word)) or x)
    m = layers.GraphDropPath(0.4).train()
    graph = SimpleNamespace(num_graphs=5, batch=torch.zeros(3, dtype=torch.int32))
    x = torch.ones(3, 4)
    torch.manual_seed(5)
    m(x, graph)
    state = torch.get_rng_state()
    torch.manual_seed(5)
    r = torch.rand((5, 1), dtype=torch.float64)
    assert torch.equal(torch.get_rng_state(), state), "the layer consumed another amount of the generator's stream"
    want = ((0.6 + r).floor() / 0.6).to(torch.float32).view(-1)
    assert torch.equal(calls[0], want) and 0 < int((want > 0).sum()) < 5
    # inside the scope: nothing consumed, the calls counted
    torch.manual_seed(5)
    state = torch.get_rng_state()
    with droppath.device_draws(123):
        m(x, graph)
        m(x, graph)
        assert m.eval()(x, graph) is x  # eval mode: the identity, no call taken
        m.train()
        m(x, graph)
    assert torch.equal(torch.get_rng_state(), state)
    assert calls[1:] == [(0.4, 123, 0, None), (0.4, 123, 1, None), (0.4, 123, 2, None)]
    m(x, graph)
    assert len(calls) == 5 and torch.is_tensor(calls[4]), "outside the scope again: the host draw"


def test_entry_point_is_declared_and_bound_with_equal_argument_counts():
    import os
    from equiformer_amd import lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(root, "include", "equiformer_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+eqf_segment_droppath\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert m, "eqf_segment_droppath is not declared"
    assert len([a for a in m.group(1).split(",") if a.strip()]) == len(lib.SIGNATURES["eqf_segment_droppath"]) == 11


def test_cpu_tensor_is_refused():
    import pytest
    from equiformer_amd.ops import HipOnlyError
    with pytest.raises(HipOnlyError):
        droppath.segment_droppath(torch.zeros(2, 4), torch.zeros(2, dtype=torch.int32), 0.4, 7, 0)
