"""Per-graph stochastic depth drawn on the device (csrc/edge.hip: eqf_segment_droppath).

`GraphDropPath` outside this module's scope draws its keep mask on the host from torch's CPU generator; a HIP-graph capture
freezes that mask.  Here the draw of graph g in the `call`-th stochastic-depth call of a step is a pure function of
(seed, call, g) computed inside the kernel (csrc/rng.h, stream tag 32), and the seed is `seed + *seed_word` with `seed_word` a
device word the host advances between replays -- the scheme of the attention dropout (ops.dropout_seed_offset).  The draw of a
graph does not depend on how many graphs the batch has: the phantom molecule of a padded batch is graph B with a draw of its
own, so a padded and an unpadded step drop the same real graphs.

  segment_droppath(x, seg_of, drop_prob, seed, call, seed_word=None)   the differentiable operator
  keep_factors(seed, call, num_graphs, drop_prob)                      the same factors on the host, in Python integers
  device_draws(seed)                                                   the scope in which GraphDropPath draws this way
"""
import contextlib
import struct

import torch
from torch.autograd import Function

from .ops import HipOnlyError, _c, _chk, _p, _stream
from .ops import call as _call

_MASK64 = (1 << 64) - 1
DROPPATH_TAG = 32  # the stream tag of csrc/edge.hip (dens.hip: 0-2, is2rs.hip: 16-18)


# ---- csrc/rng.h, restated in Python integers ----------------------------------------------------------------------------------
def mix64(z):
    """eqf_mix64: the splitmix64 finaliser"""
    z &= _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def step_seed(seed, k):
    """The seed of step k (0-based) of a run seeded with `seed`: (seed + k * 0x9E3779B97F4A7C15) mod 2^64 -- of the corruption
    (dens.py), of the perturbation (is2rs.py), of stochastic depth and the equivariant dropouts (capture.py).  The kernels
    hash the seed, so consecutive values give unrelated draws."""
    return (int(seed) + int(k) * 0x9E3779B97F4A7C15) & _MASK64


def rand_bits(seed, tag, idx):
    """eqf_rand_bits: the 64 bits of draw `idx` of stream `tag`"""
    key = mix64(int(seed) + 0xD6E8FEB86659FD93 * (int(tag) + 1))
    return mix64(key + 0x9E3779B97F4A7C15 * (int(idx) + 1))


def rand_uniform(seed, tag, idx):
    """eqf_rand_uniform: the top 24 bits as an exact float in [0, 1)"""
    return (rand_bits(seed, tag, idx) >> 40) / 16777216.0


def _fp32(v):
    return struct.unpack("f", struct.pack("f", float(v)))[0]


def _inv_keep(drop_prob):
    """1 / (1 - p) rounded to fp32 on the host: the bits of the factor do not depend on the device's division"""
    return _fp32(1.0 / (1.0 - float(drop_prob)))


def keep_factors(seed, call, num_graphs, drop_prob):
    """The factors eqf_segment_droppath applies in stochastic-depth call `call` of a step seeded with `seed` (the TOTAL seed:
    by-value part plus device word, mod 2^64): float32 [num_graphs], 0 for a dropped graph, fp32(1 / (1 - drop_prob)) for a
    kept one.  A pure host function -- log it to know which graphs a step dropped."""
    seed, call = int(seed) & _MASK64, int(call)
    if not 0 <= call < (1 << 32):
        raise ValueError("call index out of range")
    p, inv = _fp32(drop_prob), _inv_keep(drop_prob)
    return torch.tensor([inv if rand_uniform(seed, DROPPATH_TAG, (call << 32) | g) >= p else 0.0
                         for g in range(int(num_graphs))], dtype=torch.float32)


# ---- the operator ---------------------------------------------------------------------------------------------------------------
class _SegmentDropPath(Function):
    @staticmethod
    def forward(ctx, x, seg_of, drop_p, seed, seed_word, call_idx):
        x = _c(x)
        _chk(x, seg_of)
        if x.dim() != 2:
            raise HipOnlyError("segment_droppath takes [rows, D] features")
        out = torch.empty_like(x)
        _call("eqf_segment_droppath", _p(x), _p(seg_of), _p(out), x.shape[0], x.shape[1], drop_p, _inv_keep(drop_p), seed,
              _p(seed_word), call_idx, _stream())
        ctx.seg_of, ctx.seed_word, ctx.args = seg_of, seed_word, (drop_p, seed, call_idx)
        return out

    @staticmethod
    def backward(ctx, dout):
        # linear in x: its own backward at every order, redrawing the mask from the saved (seed, seed_word, call)
        drop_p, seed, call_idx = ctx.args
        return _SegmentDropPath.apply(dout, ctx.seg_of, drop_p, seed, ctx.seed_word, call_idx), None, None, None, None, None


def segment_droppath(x, seg_of, drop_prob, seed, call, seed_word=None):
    """out[q] = f(seg_of[q]) * x[q], f = keep_factors(seed + seed_word, call, ., drop_prob) drawn inside the kernel.
    seed: Python int (by value); seed_word: None or a one-element int64 CUDA tensor added to it mod 2^64 when the kernel runs."""
    drop_prob = float(drop_prob)
    if not 0.0 <= drop_prob < 1.0:
        raise ValueError("drop_prob must lie in [0, 1), got %r" % drop_prob)
    call = int(call)
    if not 0 <= call < (1 << 32):
        raise ValueError("call index out of range")
    if seed_word is not None:
        if not seed_word.is_cuda:
            raise HipOnlyError("the seed word lives on the GPU (got a %s tensor)" % seed_word.device)
        if seed_word.dtype != torch.int64 or seed_word.numel() != 1:
            raise HipOnlyError("the seed word is one int64, got %s x %d" % (seed_word.dtype, seed_word.numel()))
    return _SegmentDropPath.apply(x, seg_of, drop_prob, int(seed) & _MASK64, seed_word, call)


# ---- the scope ------------------------------------------------------------------------------------------------------------------
class _Draws:
    """The state of one `device_draws` scope: the seed (by value and / or device word) and the call counters -- one for
    stochastic depth, one for the equivariant dropout (dropout.py), which draws from the same seed under another stream tag."""

    def __init__(self, seed, base):
        if torch.is_tensor(seed):
            self.word, self._seed = seed, base
        else:
            self.word, self._seed = None, int(seed)
        self.calls = 0
        self.dropout_calls = 0  # the equivariant dropout's calls (dropout.py, stream tag 33) count apart from stochastic depth's

    @property
    def seed(self):
        if callable(self._seed):  # resolved by the first call that really drops, and only then
            self._seed = int(self._seed())
        return self._seed

    def next_call(self):
        c = self.calls
        self.calls += 1
        return c

    def next_dropout_call(self):
        c = self.dropout_calls
        self.dropout_calls += 1
        return c


_active = [None]


def active():
    """the innermost `device_draws` scope, or None"""
    return _active[0]


@contextlib.contextmanager
def device_draws(seed, base=0):
    """Inside, a training-mode GraphDropPath with drop_prob > 0 draws its keep mask on the device.  seed: a Python int passed
    by value, or a one-element int64 CUDA tensor used as the device word (the by-value part is then `base`: 0, or a callable
    evaluated once by the first call that really drops -- the step classes' lazily drawn base seed).  The scope counts the
    calls from 0: every GraphDropPath.forward that really drops takes the next value.  The equivariant dropout modules
    (dropout.EquivariantDropout, EquivariantScalarsDropout: out_drop, proj_drop) draw in the kernel from the same seed in this
    scope, counting their calls separately.  Scopes nest; leaving one restores the outer scope with its counters."""
    prev = _active[0]
    _active[0] = d = _Draws(seed, base)
    try:
        yield d
    finally:
        _active[0] = prev
