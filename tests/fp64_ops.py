"""Plain float64 restatements of the row, segment and attention operators (TEST INFRASTRUCTURE, not product code).

Each function states one operator of `equiformer_amd.ops` from its definition, a few lines of torch in the project's row
layout (a row holds its irreps segments one after the other, the segment of degree l stored as [2l+1][mul]).  Nothing
here imports `equiformer_amd.ops` or touches HIP; gradients come from autograd on these functions.
tests/test_fp64_ops.py pins them on the CPU against the oracle modules (e3nn layout) at 1e-12, tests/test_gpu_op_edges.py
and tests/test_gpu_dp_edges.py (kv_split, kv_merge, dp_logits) compare the HIP kernels with them.  The functions work in whatever dtype their inputs have: float64 is the reference,
the same call in float32 is the yardstick for what fp32 arithmetic can deliver on an input (`yardstick` below).

Inputs of a comparison are float32-rounded values cast to double (`f32r`), so input rounding is never counted as
kernel error.
"""
import re

import torch


# ------------------------------------------------------------------------------------------------- layouts and metrics
class Segs:
    """Segments of a feature row: `segs` = [(mul, l)], `par` = [+1 / -1], `offsets`, `dim`.  Accepts an irreps string
    ("64x0e+32x1e+16x0e"), a list of (mul, l) or (mul, l, p), or any object with .segs (and .par): unlike RowLayout it
    does not ask for sorted, merged irreps, so it also describes rows with two 0e segments."""

    def __init__(self, spec):
        if isinstance(spec, str):
            items = []
            for term in spec.replace(" ", "").split("+"):
                m = re.fullmatch(r"(\d+)x(\d+)([eo])", term)
                items.append((int(m.group(1)), int(m.group(2)), 1 if m.group(3) == "e" else -1))
        elif hasattr(spec, "segs"):
            par = getattr(spec, "par", None) or [1] * len(spec.segs)
            items = [(mul, l, p) for (mul, l), p in zip(spec.segs, par)]
        else:
            items = [tuple(t) if len(t) == 3 else (t[0], t[1], 1) for t in spec]
        self.segs = [(mul, l) for mul, l, _ in items]
        self.par = [p for _, _, p in items]
        self.offsets, off = [], 0
        for mul, l in self.segs:
            self.offsets.append(off)
            off += mul * (2 * l + 1)
        self.dim = off

    def slices(self):
        """one slice of the row per segment"""
        return [slice(off, off + mul * (2 * l + 1)) for (mul, l), off in zip(self.segs, self.offsets)]

    def perm_from_e3nn(self):
        """idx with x_rows = x_e3nn[..., idx]: e3nn stores a segment as [mul][2l+1], the rows here as [2l+1][mul]"""
        idx = []
        for (mul, l), off in zip(self.segs, self.offsets):
            d = 2 * l + 1
            idx += [off + u * d + m for m in range(d) for u in range(mul)]
        return torch.tensor(idx, dtype=torch.long)

    def scalar(self, s):
        """segment s is an invariant scalar (0e): mean subtraction and bias"""
        return self.segs[s][1] == 0 and self.par[s] == 1


def f32r(t):
    """float32-rounded values as float64"""
    return t.float().double()


def per_row_rel(got, ref, floor=1e-3, slices=None):
    """max over rows (and over `slices` of a row, e.g. the segments of a layer norm) of
    max_c |got - ref| / max(max_c |ref|, floor * global max |ref|).
    The scale is taken per row, so a row of small magnitude is not divided by the largest value of the tensor; a row whose
    reference is exactly zero is compared absolutely (against the floor), not skipped.  A 1-D tensor is one element per
    row, or, with `slices`, ONE row cut into those slices (a parameter gradient per segment, or per element)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.numel() == 0:
        return 0.0
    nrow = 1 if (ref.dim() == 1 and slices is not None) else ref.shape[0]
    got, ref = got.reshape(nrow, -1), ref.reshape(nrow, -1)
    fl = floor * float(ref.abs().max())
    worst = 0.0
    for sl in (slices if slices is not None else [slice(None)]):
        err = (got[:, sl] - ref[:, sl]).abs().amax(dim=1)
        scale = ref[:, sl].abs().amax(dim=1).clamp_min(fl).clamp_min(1e-300)
        worst = max(worst, float((err / scale).max()))
    return worst


def ragged_graph(degrees, n_src, seed, device="cpu"):
    """Destination-sorted EdgeGraph whose node i has in-degree degrees[i]; sources are drawn at random from the first
    `n_src` nodes, with repeats.  The edge list is shuffled before it goes through EdgeGraph.from_edges."""
    from equiformer_amd.graph import EdgeGraph
    N = len(degrees)
    assert 0 < n_src <= N
    g = torch.Generator().manual_seed(seed)
    dst = torch.repeat_interleave(torch.arange(N), torch.tensor(degrees, dtype=torch.long))
    src = torch.randint(0, n_src, (dst.numel(),), generator=g)
    shuffle = torch.randperm(dst.numel(), generator=g)
    graph, _ = EdgeGraph.from_edges(src[shuffle].to(device), dst[shuffle].to(device), N)
    return graph


def evaluate(fn, inputs, grad_outputs, dtype, device="cpu", wrt=None):
    """(outputs, gradients) of fn at `inputs` (float64 CPU tensors; integer tensors and non-tensors pass through) in
    `dtype` on `device`; `grad_outputs` are the cotangents, one per output; gradients are taken wrt the floating inputs
    listed in `wrt` (default: all of them).  On a GPU every tensor the function receives, cotangents included, is a copy
    between guard bands (tests/poison.py: NaN around floating tensors, so that a load past the end shows in the result;
    index tensors keep valid contents); the floating inputs are leaves as before."""
    on_gpu = torch.device(device).type != "cpu"
    if on_gpu:
        from poison import guard_input
    put = (lambda t: guard_input(t.to(device))) if on_gpu else (lambda t: t.to(device))
    ins = []
    for t in inputs:
        if torch.is_tensor(t) and t.is_floating_point():
            ins.append(put(t.detach().to(dtype)).requires_grad_(True))
        elif torch.is_tensor(t):
            ins.append(put(t))
        else:
            ins.append(t)
    outs = fn(*ins)
    outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
    fl = [i for i, t in enumerate(ins) if torch.is_tensor(t) and t.is_floating_point()]
    wrt = fl if wrt is None else wrt
    gos = [put(g.to(dtype)) for g in grad_outputs]
    grads = torch.autograd.grad(outs, [ins[i] for i in wrt], gos, allow_unused=True)
    return [o.detach() for o in outs], list(grads)


def yardstick(fn, inputs, grad_outputs, wrt=None):
    """The restatement in float64 and the SAME restatement in float32 on the CPU: (ref outputs, ref gradients,
    f32 outputs, f32 gradients).  The float32 run is what plain fp32 arithmetic gives on these inputs."""
    ro, rg = evaluate(fn, inputs, grad_outputs, torch.float64, wrt=wrt)
    yo, yg = evaluate(fn, inputs, grad_outputs, torch.float32, wrt=wrt)
    return ro, rg, yo, yg


# ------------------------------------------------------------------------------------------------- row-local operators
def layer_norm(x, weight, bias, layout, eps=1e-5):
    """Equivariant layer norm, 'component' normalisation: per segment, the channel mean is subtracted on 0e only, the
    segment is divided by the root of its mean square over (component, channel) (+ eps), every channel has an affine
    weight and the 0e channels a bias."""
    lay = layout if isinstance(layout, Segs) else Segs(layout)
    out, iw, ib = [], 0, 0
    for s, ((mul, l), off) in enumerate(zip(lay.segs, lay.offsets)):
        d = 2 * l + 1
        f = x[:, off:off + mul * d].reshape(-1, d, mul)
        if lay.scalar(s):
            f = f - f.mean(dim=2, keepdim=True)
        f = f * (f.pow(2).mean(dim=(1, 2), keepdim=True) + eps).pow(-0.5) * weight[iw:iw + mul]
        iw += mul
        if lay.scalar(s):
            f = f + bias[ib:ib + mul]
            ib += mul
        out.append(f.reshape(-1, mul * d))
    return torch.cat(out, dim=1)


def add_layer_norm(a, b, weight, bias, layout, eps=1e-5):
    """(y, xsum) = (layer_norm(a + b), a + b)"""
    s = a + b
    return layer_norm(s, weight, bias, layout, eps), s


def gate(x, S, gated_layout, c_silu, c_sig):
    """[S scalars | one gate per gated channel | gated segments] -> [c_silu silu(scalars) | gated * c_sig sigmoid(gate)]"""
    lay = gated_layout if isinstance(gated_layout, Segs) else Segs(gated_layout)
    G = sum(mul for mul, _ in lay.segs)
    out, ig = [c_silu * x[:, :S] * torch.sigmoid(x[:, :S])], S
    for (mul, l), off in zip(lay.segs, lay.offsets):
        d = 2 * l + 1
        f = x[:, S + G + off:S + G + off + mul * d].reshape(-1, d, mul)
        out.append((f * (c_sig * torch.sigmoid(x[:, ig:ig + mul]))[:, None, :]).reshape(-1, mul * d))
        ig += mul
    return torch.cat(out, dim=1)


def scaled_silu(x, c):
    return c * x * torch.sigmoid(x)


def ln_silu(x, gamma, beta, eps=1e-5, groups=1):
    """silu(LayerNorm(x) * gamma + beta) on each of the `groups` column blocks of a row (biased variance)"""
    n, C = x.shape[0], x.shape[1] // groups
    f = x.reshape(n, groups, C)
    f = f - f.mean(dim=2, keepdim=True)
    z = f * (f.pow(2).mean(dim=2, keepdim=True) + eps).pow(-0.5) * gamma.reshape(groups, C) + beta.reshape(groups, C)
    return (z * torch.sigmoid(z)).reshape(n, groups * C)


def embedding(types, W, b, D):
    """rows W[type] (+ b) in the first C columns of a D-wide row, zeros after them"""
    y = W[types.long()] + (b if b is not None else 0.0)
    return torch.cat([y, y.new_zeros(y.shape[0], D - W.shape[1])], dim=1)


def fold_weight(W, w, row_start, w_of_row):
    """out[i] = W[i] * w[w_of_row[row(i)]] on a flat weight whose row r spans row_start[r]:row_start[r+1]"""
    rs = row_start.long()
    row_of = torch.repeat_interleave(torch.arange(rs.numel() - 1, device=W.device), rs[1:] - rs[:-1])
    return W * w[w_of_row.long()[row_of]]


# ------------------------------------------------------------------------------------------------- segments and graphs
def seg_of_ptr(ptr):
    p = ptr.long()
    return torch.repeat_interleave(torch.arange(p.numel() - 1, device=p.device), p[1:] - p[:-1])


def segment_sum(x, ptr, scale=1.0):
    """out[s] = scale * sum of rows ptr[s]:ptr[s+1]"""
    out = x.new_zeros((ptr.numel() - 1,) + tuple(x.shape[1:]))
    return scale * out.index_add(0, seg_of_ptr(ptr), x)


def segment_bcast(x, seg_of, scale=1.0):
    """out[q] = scale * x[seg_of[q]]"""
    return scale * x[seg_of.long()]


def segment_scale(x, s, seg_of):
    """out[q] = s[seg_of[q]] * x[q]"""
    return x * s[seg_of.long()][:, None]


def gather_add(a, b, src, dst):
    """msg[e] = a[src[e]] (+ b[dst[e]])"""
    msg = a[src.long()]
    return msg if b is None else msg + b[dst.long()]


# ------------------------------------------------------------------------------------------------- attention
def smooth_leaky_relu(x, slope=0.2):
    return ((1 + slope) / 2) * x + ((1 - slope) / 2) * x * (2 * torch.sigmoid(x) - 1)


def normalize2mom(f):
    """e3nn's second-moment constant of an activation: 1 / sqrt(mean f(z)^2) over 1e6 fp64 normal samples of seed 0"""
    z = torch.randn(1_000_000, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    return f(z).pow(2).mean().pow(-0.5).item()


_c_slrelu = []


def c_smooth_leaky_relu():
    if not _c_slrelu:
        _c_slrelu.append(normalize2mom(smooth_leaky_relu))
    return _c_slrelu[0]


def alpha_logits(a, alpha_dot, H, Kh, c=None):
    """logit[e, h] = sum_k c SmoothLeakyReLU_0.2(a[e, h, k]) alpha_dot[h, k]"""
    c = c_smooth_leaky_relu() if c is None else c
    return (c * smooth_leaky_relu(a.reshape(-1, H, Kh)) * alpha_dot.reshape(1, H, Kh)).sum(-1)


def head_of_column(layout, H):
    """head that owns each column of an all-heads row: inside a segment the channels are split into H equal blocks"""
    lay = layout if isinstance(layout, Segs) else Segs(layout)
    idx = []
    for mul, l in lay.segs:
        assert mul % H == 0
        idx += [u // (mul // H) for u in range(mul)] * (2 * l + 1)
    return torch.tensor(idx, dtype=torch.long)


def segment_softmax(logit, row_ptr):
    """per destination row and head: exp(x - max) / (sum + 1e-16); rows are the spans of row_ptr"""
    p = row_ptr.long().tolist()
    out = []
    for beg, end in zip(p[:-1], p[1:]):
        if end > beg:
            ex = torch.exp(logit[beg:end] - logit[beg:end].detach().amax(dim=0, keepdim=True))
            out.append(ex / (ex.sum(dim=0, keepdim=True) + 1e-16))
    return torch.cat(out, dim=0) if out else logit * 0.0


def attn_aggregate(logit, value, row_ptr, H, layout, keep=None):
    """(out, alpha): out[n] = sum over the edges of row n of alpha[e, head(col)] * keep[e, head(col)] * value[e];
    keep is the inverted-dropout mask (0 or 1 / (1 - p) per edge and head), None = no dropout"""
    alpha = segment_softmax(logit, row_ptr)
    wgt = alpha if keep is None else alpha * keep
    hoc = head_of_column(layout, H).to(value.device)
    return segment_sum(value * wgt[:, hoc], row_ptr), alpha


# ------------------------------------------------------------------------------------------------- dot-product attention
# `segs` describes the q / k / v row of all H heads: in the segment of degree l the channel index is (head, channel of the
# head), so mul = H * mul_of_head.  The key/value row holds 2H heads per segment, [2l+1][2 mul]: the first `mul` channels
# of every m-row are the keys, the last `mul` the values.
def _head_segs(segs, H):
    lay = segs if isinstance(segs, Segs) else Segs(segs)
    assert all(mul % H == 0 for mul, _ in lay.segs), (lay.segs, H)
    return lay


def kv_split(kv, segs, H):
    """kv [E, 2 D] -> (k, v), [E, D] each"""
    lay = _head_segs(segs, H)
    k, v, off = [], [], 0
    for mul, l in lay.segs:
        d = 2 * l + 1
        f = kv[:, off:off + 2 * mul * d].reshape(-1, d, 2 * mul)
        k.append(f[:, :, :mul].reshape(-1, d * mul))
        v.append(f[:, :, mul:].reshape(-1, d * mul))
        off += 2 * mul * d
    return torch.cat(k, dim=1), torch.cat(v, dim=1)


def kv_merge(k, v, segs, H):
    """the inverse of kv_split; a missing k or v is zero"""
    lay = _head_segs(segs, H)
    given = k if k is not None else v
    k = torch.zeros_like(given) if k is None else k
    v = torch.zeros_like(given) if v is None else v
    out = []
    for (mul, l), off in zip(lay.segs, lay.offsets):
        d = 2 * l + 1
        out.append(torch.cat([k[:, off:off + mul * d].reshape(-1, d, mul), v[:, off:off + mul * d].reshape(-1, d, mul)],
                             dim=2).reshape(-1, 2 * mul * d))
    return torch.cat(out, dim=1)


def dp_scales(segs, H):
    """scale_s = 1 / sqrt(sum_s mul_s / H) / sqrt(2 l_s + 1): the ScaleFactor of the dot-product attention, per segment"""
    lay = _head_segs(segs, H)
    num = sum(mul // H for mul, _ in lay.segs)
    return [1.0 / (num ** 0.5 * (2 * l + 1) ** 0.5) for _, l in lay.segs]


def dp_logits(q, k, dst, segs, H):
    """logit[e, h] = sum_s scale_s sum_{m, c} q[dst[e], s, m, h, c] k[e, s, m, h, c]"""
    lay = _head_segs(segs, H)
    qd = q[dst.long()]
    logit = 0.0
    for (mul, l), off, sc in zip(lay.segs, lay.offsets, dp_scales(lay, H)):
        d = 2 * l + 1
        qs = qd[:, off:off + mul * d].reshape(-1, d, H, mul // H)
        ks = k[:, off:off + mul * d].reshape(-1, d, H, mul // H)
        logit = logit + sc * (qs * ks).sum(dim=(1, 3))
    return logit


# ------------------------------------------------------------------------------------------------- shared cases
# The ragged inputs of tests/test_gpu_op_edges.py; tests/test_fp64_ops.py pins the restatements on the same ones.
# In-degrees of the attention graph: the tails of the four-edges-per-step loops (0..9), the wavefront boundary where the
# logits held in registers hand over to memory (62..69), rows of two and three wavefronts, empty rows first and last.
ATTN_DEGREES = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 32, 33, 62, 63, 64, 65, 66, 67, 68, 69, 127, 128, 129, 130, 0, 1, 0]
# (per-head irreps, heads): G = float4 groups per head = dim(head) / 4.  G <= 32 takes the half-wave kernels, G > 32 the
# full ones, whose slot s holds group lane + 64 s (slots 1..3 are used from G = 65 on).
ATTN_HEADS = [("32x0e+16x1e+8x2e", 4),            # G = 30: half kernels
              ("128x0e", 2),                      # G = 32: half kernels, at their limit
              ("32x0e+16x1e+16x2e+8x3e", 4),      # G = 54: full kernels, slot 0 only
              ("20x0e+80x1e", 1),                 # G = 65: one lane of slot 1
              ("128x0e+64x1e+32x2e", 2),          # G = 120: slots 0 and 1
              ("256x0e+256x1e", 1),               # G = 256: all four slots full
              ("4x0e", 16)]                       # G = 1, H = 16: the head limit (1024 threads)
SEG_LENGTHS = [0, 1, 3, 4, 5, 8, 9, 0, 130, 0]
LN_IRREPS = ["128x0e+64x1e+32x2e", "128x0e+64x1e+64x2e+32x3e", "512x0e", "8x0e+4x1e", "64x0e+32x1e+16x0e"]
LN_FAMILIES = ["randn", "randn+100", "1e-3*randn", "1e3*randn", "zero-and-constant"]


def all_heads_layout(head_irreps, H):
    """row of all H heads: every segment of the head, H times as wide"""
    return Segs([(mul * H, l, p) for (mul, l), p in zip(Segs(head_irreps).segs, Segs(head_irreps).par)])


def head_groups(head_irreps):
    return Segs(head_irreps).dim // 4


def ln_input(family, rows, layout, seed):
    """float32-rounded rows (as float64) of one input family of the layer-norm tests"""
    lay = layout if isinstance(layout, Segs) else Segs(layout)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, lay.dim, generator=g, dtype=torch.float64)
    if family == "randn+100":
        x = x + 100.0
    elif family == "1e-3*randn":
        x = x * 1e-3
    elif family == "1e3*randn":
        x = x * 1e3
    elif family == "zero-and-constant":
        sl0 = lay.slices()[[s for s in range(len(lay.segs)) if lay.scalar(s)][-1]]  # the LAST 0e segment
        x[0::3] = 0.0            # all-zero rows: rsqrt(0 + eps) in every segment
        x[1::3, sl0] = 1.5       # a constant 0e segment: zero after the mean subtraction
    else:
        assert family == "randn", family
    return f32r(x)


def attn_logits(regime, E, H, row_ptr, seed):
    """float32-rounded logits (as float64): "randn" 3 randn; "+80" / "-80" shifted; "peak": one logit per row and head
    60 above the rest (a near one-hot softmax)"""
    g = torch.Generator().manual_seed(seed)
    lg = 3.0 * torch.randn(E, H, generator=g, dtype=torch.float64)
    if regime == "+80":
        lg = lg + 80.0
    elif regime == "-80":
        lg = lg - 80.0
    elif regime == "peak":
        p = row_ptr.long().tolist()
        for beg, end in zip(p[:-1], p[1:]):
            if end > beg:
                pick = torch.randint(beg, end, (H,), generator=g)
                lg[pick, torch.arange(H)] += 60.0
    else:
        assert regime == "randn", regime
    return f32r(lg)
