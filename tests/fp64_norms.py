"""Plain float64 restatements of the graph norm and the instance norm (TEST INFRASTRUCTURE, not product code), in the
project's row layout (`fp64_ops.Segs`: a segment of degree l is stored as [2l+1][mul]).  Written from the definition:
for a channel u of a segment of dimension d = 2l+1, in a graph g with n_g nodes,

    0e segments (l == 0, even):  mu[g,u] = (1/n_g) sum_nodes x[.,u],   c = x - mean_shift[u] mu[g,u]
    all other segments:          c = x                                  (a pseudo-scalar 0o is not centred)
    v[g,u] = (1/(n_g d)) sum_nodes sum_m c^2,     y = c (v[g,u] + eps)^(-1/2) weight[u]   (+ bias[u] on 0e)

`mean_shift=None` is the instance norm (mean_shift == 1).  `ptr` is the list of graph boundaries (len B + 1; empty graphs
allowed), rows sorted by graph.  Nothing here imports `equiformer_amd.ops`; gradients come from autograd; the functions
work in the dtype of their inputs (float64: reference, float32: yardstick).  tests/test_norm_restatements.py pins them to
hand-computed answers and to the reference's own classes.
"""
import torch

from fp64_ops import Segs


def graph_norm(x, mean_shift, weight, bias, layout, ptr, eps=1e-5):
    lay = layout if isinstance(layout, Segs) else Segs(layout)
    ptr = [int(p) for p in ptr]
    assert ptr[0] == 0 and ptr[-1] == x.shape[0]
    out, iw, ib = [], 0, 0
    for s, ((mul, l), off) in enumerate(zip(lay.segs, lay.offsets)):
        d = 2 * l + 1
        f = x[:, off:off + mul * d].reshape(-1, d, mul)
        w = weight[iw:iw + mul]
        iw += mul
        parts = []
        for g in range(len(ptr) - 1):
            fg = f[ptr[g]:ptr[g + 1]]
            if fg.shape[0] == 0:
                continue
            if lay.scalar(s):
                mu = fg.mean(dim=0, keepdim=True)
                fg = fg - (mu if mean_shift is None else mu * mean_shift[ib:ib + mul])
            v = fg.pow(2).mean(dim=(0, 1), keepdim=True)
            fg = fg * (v + eps).pow(-0.5) * w
            if lay.scalar(s):
                fg = fg + bias[ib:ib + mul]
            parts.append(fg)
        if lay.scalar(s):
            ib += mul
        out.append(torch.cat(parts, dim=0).reshape(-1, mul * d) if parts else f.reshape(-1, mul * d))
    return torch.cat(out, dim=1)


def add_graph_norm(a, b, mean_shift, weight, bias, layout, ptr, eps=1e-5):
    """(y, xsum) = (graph_norm(a + b), a + b)"""
    s = a + b
    return graph_norm(s, mean_shift, weight, bias, layout, ptr, eps), s


def instance_norm(x, weight, bias, layout, ptr, eps=1e-5):
    return graph_norm(x, None, weight, bias, layout, ptr, eps)


def add_instance_norm(a, b, weight, bias, layout, ptr, eps=1e-5):
    return add_graph_norm(a, b, None, weight, bias, layout, ptr, eps)
