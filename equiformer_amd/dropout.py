"""Equivariant dropout drawn on the device (csrc/dropout.hip: eqf_irreps_dropout): `out_drop` and `proj_drop`.

[ref: nets/drop.py:68-108]  One keep factor per irrep instance of a row, shared by its 2l+1 components
(`EquivariantDropout`), or the same on the 0e segments alone with everything else copied (`EquivariantScalarsDropout`).  The
factor of (row, channel c) in the `call`-th dropout call of a step is a pure function of (seed, call, row, c) computed inside
the kernel (csrc/rng.h, stream tag 33), and the seed is `seed + *seed_word` with `seed_word` a device word the host advances
between replays -- the scheme of the per-graph stochastic depth (droppath.py), whose `device_draws` scope the modules below
share.  The factor of a row does not depend on how many rows the batch has: the phantom rows of a padded batch take nothing
from the real ones.

  irreps_dropout(x, layout_or_irreps, drop_prob, seed, call, seed_word=None, scalars_only=False)   the differentiable operator
  keep_mask(seed, call, rows, irreps, drop_prob, scalars_only=False, expand=None)                  the same factors on the host
  expand_mask(mask, irreps, order="cf")                                                            [rows, num_irreps] -> [rows, D]
  EquivariantDropout(irreps, drop_prob), EquivariantScalarsDropout(irreps, drop_prob)              the reference's modules
"""
import numpy as np
import torch
from torch import nn
from torch.autograd import Function

from . import droppath, ops
from .droppath import _MASK64, _fp32, _inv_keep
from .irreps import Irreps
from .layout import RowLayout
from .ops import HipOnlyError, _c, _chk, _p, _stream
from .ops import call as _call

DROPOUT_TAG = 33  # the stream tag of csrc/dropout.hip (dens.hip: 0-2, is2rs.hip: 16-18, stochastic depth: 32)
_CALL_BITS = _CHANNEL_BITS = 16  # a draw's index packs (call, row, channel) into 16 + 32 + 16 bits


def _layout(layout_or_irreps):
    return layout_or_irreps if isinstance(layout_or_irreps, RowLayout) else RowLayout(Irreps(layout_or_irreps))


def _check(layout, drop_prob, call):
    drop_prob, call = float(drop_prob), int(call)
    if not 0.0 <= drop_prob < 1.0:
        raise ValueError("drop_prob must lie in [0, 1), got %r" % drop_prob)
    if not 0 <= call < (1 << _CALL_BITS):
        raise ValueError("dropout call index out of range: %d (a step has at most 2^16 dropout calls)" % call)
    if layout.num_irreps >= (1 << _CHANNEL_BITS):
        raise ValueError("dropout rows hold fewer than 2^16 irreps, got %d" % layout.num_irreps)
    return drop_prob, call


# ---- csrc/rng.h in wrapping numpy.uint64 arithmetic -----------------------------------------------------------------------------
def _mix64(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def rand_uniform(seed, tag, idx):
    """eqf_rand_uniform over an array of indices: float64 values k / 2^24 (exact floats), as droppath.rand_uniform gives them
    one Python integer at a time"""
    with np.errstate(over="ignore"):
        key = _mix64(np.array([(int(seed) + 0xD6E8FEB86659FD93 * (int(tag) + 1)) & _MASK64], dtype=np.uint64))
        z = _mix64(key + np.uint64(0x9E3779B97F4A7C15) * (np.asarray(idx, dtype=np.uint64) + np.uint64(1)))
    return (z >> np.uint64(40)).astype(np.float64) / 16777216.0


def _dropped_columns(layout, scalars_only):
    """bool [num_irreps]: the channels whose segment the operator drops on"""
    cols = []
    for (mul, l), p in zip(layout.segs, layout.par):
        cols.append(np.full(mul, (not scalars_only) or (l == 0 and p == 1)))
    return np.concatenate(cols) if cols else np.zeros(0, dtype=bool)


def expand_mask(mask, irreps, order="cf"):
    """[rows, num_irreps] factors -> [rows, D]: every irrep's factor repeated over its 2l+1 components, in this project's row
    layout (order "cf": a segment is [2l+1][mul]) or in e3nn's (order "e3nn": [mul][2l+1])."""
    if order not in ("cf", "e3nn"):
        raise ValueError("order is 'cf' or 'e3nn', got %r" % (order,))
    layout, parts, c = _layout(irreps), [], 0
    for mul, l in layout.segs:
        f = mask[:, c:c + mul]
        parts.append(f.repeat(1, 2 * l + 1) if order == "cf" else f.repeat_interleave(2 * l + 1, dim=1))
        c += mul
    return torch.cat(parts, dim=1) if parts else mask.new_zeros((mask.shape[0], 0))


def keep_mask(seed, call, rows, irreps, drop_prob, scalars_only=False, expand=None):
    """The factors eqf_irreps_dropout applies in dropout call `call` of a step seeded with `seed` (the TOTAL seed: by-value part
    plus device word, mod 2^64): float32 [rows, num_irreps], 0 for a dropped irrep, fp32(1 / (1 - drop_prob)) for a kept one, and
    exactly 1 on the columns a scalars_only call copies.  expand="cf" / "e3nn": already [rows, D] (expand_mask).  A pure host
    function -- log it to know what a step dropped."""
    layout = _layout(irreps)
    drop_prob, call = _check(layout, drop_prob, call)
    rows, n = int(rows), layout.num_irreps
    if not 0 <= rows < (1 << 31):
        raise ValueError("rows out of range")
    idx = ((np.uint64(call) << np.uint64(48)) | (np.arange(rows, dtype=np.uint64)[:, None] << np.uint64(16))
           | np.arange(n, dtype=np.uint64)[None, :])
    u = rand_uniform(int(seed) & _MASK64, DROPOUT_TAG, idx)
    f = np.where(u >= _fp32(drop_prob), np.float32(_inv_keep(drop_prob)), np.float32(0.0)).astype(np.float32)
    f[:, ~_dropped_columns(layout, scalars_only)] = 1.0
    mask = torch.from_numpy(f)
    return mask if expand is None else expand_mask(mask, layout, expand)


# ---- the operator ---------------------------------------------------------------------------------------------------------------
class _IrrepsDropout(Function):
    @staticmethod
    def forward(ctx, x, layout, scalars_only, drop_p, seed, seed_word, call_idx):
        x = _c(x)
        _chk(x)
        if x.dim() != 2 or x.shape[1] != layout.dim:
            raise HipOnlyError("irreps_dropout takes [rows, %d] rows of %r, got %r" % (layout.dim, layout.irreps, tuple(x.shape)))
        out = torch.empty_like(x)
        _call("eqf_irreps_dropout", _p(x), _p(out), x.shape[0], layout.c_ref, int(scalars_only), drop_p, _inv_keep(drop_p),
              seed, _p(seed_word), call_idx, _stream())
        ctx.layout, ctx.seed_word, ctx.args = layout, seed_word, (scalars_only, drop_p, seed, call_idx)
        return out

    @staticmethod
    def backward(ctx, dout):
        # linear in x: its own backward at every order, redrawing the mask from the saved (seed, seed_word, call)
        scalars_only, drop_p, seed, call_idx = ctx.args
        return (_IrrepsDropout.apply(dout, ctx.layout, scalars_only, drop_p, seed, ctx.seed_word, call_idx),
                None, None, None, None, None, None)


def irreps_dropout(x, layout_or_irreps, drop_prob, seed, call, seed_word=None, scalars_only=False):
    """out = x * keep_mask(seed + seed_word, call, rows, irreps, drop_prob, scalars_only, expand="cf"), the mask drawn inside the
    kernel.  seed: Python int (by value); seed_word: None or a one-element int64 CUDA tensor added to it mod 2^64 when the kernel
    runs."""
    layout = _layout(layout_or_irreps)
    drop_prob, call = _check(layout, drop_prob, call)
    if seed_word is not None:
        if not seed_word.is_cuda:
            raise HipOnlyError("the seed word lives on the GPU (got a %s tensor)" % seed_word.device)
        if seed_word.dtype != torch.int64 or seed_word.numel() != 1:
            raise HipOnlyError("the seed word is one int64, got %s x %d" % (seed_word.dtype, seed_word.numel()))
    return _IrrepsDropout.apply(x, layout, bool(scalars_only), drop_prob, int(seed) & _MASK64, seed_word, call)


# ---- the modules ----------------------------------------------------------------------------------------------------------------
class EquivariantDropout(nn.Module):
    """[ref: nets/drop.py:68-86] one Bernoulli draw per irrep of every row, shared by the irrep's components.  The identity
    (the input object itself, no launch) in eval mode and at drop_prob == 0.  In training mode the mask is drawn in the kernel:
    inside a `droppath.device_draws` scope from the scope's seed and device word, `call` counting the dropout calls of the scope
    (a counter of their own: the stochastic-depth calls keep theirs); outside a scope from one seed per forward drawn from
    torch's CPU generator (as the attention dropout draws its seed), call 0, and the attention dropout's device word
    (ops.dropout_seed_offset), so that a bare capture still redraws."""

    scalars_only = False

    def __init__(self, irreps, drop_prob):
        super().__init__()
        self.irreps = Irreps(irreps)
        self.num_irreps = self.irreps.num_irreps
        self.drop_prob = drop_prob
        self.layout = RowLayout(self.irreps)

    def forward(self, x):
        if not self.training or self.drop_prob == 0.0:
            return x
        draws = droppath.active()
        if draws is not None:
            seed, call, word = draws.seed, draws.next_dropout_call(), draws.word
        else:
            seed, call, word = int(torch.randint(0, 2 ** 62, (1,)).item()), 0, ops._seed_offset[0]
        return irreps_dropout(x, self.layout, self.drop_prob, seed, call, word, self.scalars_only)

    def extra_repr(self):
        return "irreps={}, drop_prob={}".format(self.irreps, self.drop_prob)


class EquivariantScalarsDropout(EquivariantDropout):
    """[ref: nets/drop.py:89-108] dropout on the 0e channels alone; every other segment passes bit for bit."""

    scalars_only = True
