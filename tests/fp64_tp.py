"""Plain float64 restatements of the depth-wise tensor product family from its path table (TEST INFRASTRUCTURE, not
product code): the coupling M(sh), the un-fused product T(x, M, w) and the fused SeparableFCTP

    M[e, m_off + i d3 + k]                    = sum_j cg[i, j, k] * sh[e, l2^2 + j]
    mid[e, seg(l3,p3), k, out_ch + u]         = w[e, w_off + u] * sum_i M[e, m_off + i d3 + k] * x[e, in_off + i mul + u]
    out1[e, seg(l,p)] = mid[e, seg(l,p)] . W_(l,p)  (+ bias on 0e)        out2[e] = mid[e, seg(0e)] . W2 + bias2

A few lines of torch each, differentiable any number of times by autograd; nothing here imports `equiformer_amd.ops` or
touches HIP (the `spec` / `table` arguments are read for their path table and layouts only).
tests/test_tp_restatements.py pins them on the CPU against the oracle modules (e3nn layout) at 1e-10: values, first and
second derivatives.  tests/test_gpu_sfc_e3.py and tests/test_gpu_second_order_ops.py compare the HIP kernels with them."""
import torch


def blocks(spec, weight):
    """the [K, N1] matrix of every consumer segment of the flat main weight, in spec.degs order"""
    return [weight[o:o + K * N].view(K, N) for (_, K, N, _), o in zip(spec.degs, spec.w_offs)]


def _mid(table, x, M, w):
    """{(l3, p3): [(out_ch, [E, d3, mul])]}: the product of every path, before the paths of a segment are joined"""
    E = x.shape[0]
    mid = {}
    for p in table.paths:
        d1, d3, mul = 2 * p["l1"] + 1, 2 * p["l3"] + 1, p["mul"]
        xs = x[:, p["in_off"]:p["in_off"] + d1 * mul].view(E, d1, mul)
        Mp = M[:, p["m_off"]:p["m_off"] + d1 * d3].view(E, d1, d3)
        t = torch.einsum("eik,eiu->eku", Mp, xs)
        if w is not None:
            t = t * w[:, None, p["w_off"]:p["w_off"] + mul]
        mid.setdefault((p["l3"], p["p3"]), []).append((p["out_ch"], t))
    return mid


def _segment(mid, l3, par):
    return torch.cat([t for _, t in sorted(mid[(l3, par)], key=lambda q: q[0])], dim=2)  # [E, d3, K]


def reference(spec, x, M, w, blocks, weight2, bias, bias2):
    """fp64, differentiable.  blocks: one [K, N1] matrix per consumer segment, in spec.degs order."""
    table = spec.table
    E = x.shape[0]
    mid = _mid(table, x, M, w)
    outs, out2 = [], None
    for (l3, K, N1, _), par, W in zip(spec.degs, spec.pars, blocks):
        m = _segment(mid, l3, par)
        assert m.shape[2] == K
        o = m @ W
        if (l3, par) == (0, 1):
            if bias is not None:
                o = o + bias
            if spec.n2:
                out2 = m[:, 0] @ weight2.view(K, spec.n2) + bias2
        outs.append(o.reshape(E, -1))
    return torch.cat(outs, dim=1), out2


def product(table, x, M, w):
    """the un-fused depth-wise tensor product T(x, M, w): the `mid` tensor of `reference`, one [d3][K] block per segment of
    table.layout_out"""
    mid = _mid(table, x, M, w)
    lay = table.layout_out
    return torch.cat([_segment(mid, l3, par).reshape(x.shape[0], -1) for (_, l3), par in zip(lay.segs, lay.par)], dim=1)


def coupling(table, sh):
    """M(sh): per path the [d1, d3] matrix sum_j cg[i, j, k] sh[l2^2 + j], at the path's m_off.  cg: the float64 values
    (so3.path_table) that table.cg holds rounded to float32 -- tests/test_tp_restatements.py checks that they are the same
    table -- so the oracle can be matched to 1e-10 and the rounding of the constants counts as the kernel's."""
    from equiformer_amd import so3
    E = sh.shape[0]
    M = [None] * len(table.paths)
    for n, p in enumerate(table.paths):
        d1, d2, d3 = 2 * p["l1"] + 1, 2 * p["l2"] + 1, 2 * p["l3"] + 1
        cg = torch.from_numpy(so3.path_table(p["l1"], p["l2"], p["l3"])).to(sh.dtype).reshape(d1, d2, d3)
        y = sh[:, p["l2"] ** 2:p["l2"] ** 2 + d2]
        M[n] = torch.einsum("ijk,ej->eik", cg, y).reshape(E, d1 * d3)
    order = sorted(range(len(M)), key=lambda n: table.paths[n]["m_off"])
    return torch.cat([M[n] for n in order], dim=1)
