"""fp64 restatements of EdgeDegreeEmbeddingNetwork on the repository's parameter and row layout (pure torch, CPU or GPU):

  full(...)       the operator as written -- exp(ones) gathered to the edges, every depth-wise path of the table, the
                  projection, the scaled scatter -- with the paths read generically from a DtpTable-like object;
  collapsed(...)  the identity of csrc/edgedeg.hip: only the l1 == 0 blocks (an `ops.EdgeDegSpec.blocks` list), one
                  [sum N_l, 64] matrix At and vector a, z = h At^T + a, scatter of coupling (x) z.

Parameters travel as a dict with the module's state_dict names (`exp.tp.weight`, `exp.bias.0`, `rad.net.0.weight`, ...,
`rad.offset`, `proj.tp.weight`, `proj.bias.0`); rows are channel-fastest ([2l+1][mul] inside a segment).
"""
import torch
import torch.nn.functional as F

from equiformer_amd import so3


def params_of(module, dtype=torch.float64, device=None):
    """{name: leaf copy that requires grad} of a module's parameters"""
    return {k: v.detach().to(dtype=dtype, device=device).clone().requires_grad_(True) for k, v in module.named_parameters()}


def hidden(P, edge_scalars):
    """activation in front of the radial MLP's last layer"""
    x = edge_scalars
    for i in (0, 3):
        x = F.linear(x, P["rad.net.%d.weight" % i], P["rad.net.%d.bias" % i])
        x = F.silu(F.layer_norm(x, x.shape[-1:], P["rad.net.%d.weight" % (i + 1)], P["rad.net.%d.bias" % (i + 1)], 1e-5))
    return x


def coupling(table, sh):
    """[E, m_numel]: per path the (2 l1 + 1) x (2 l3 + 1) matrix sum_j cg[i, j, k] Y_l2[j], at the path's m_off"""
    M = sh.new_zeros((sh.shape[0], table.m_numel))
    for p in table.paths:
        l1, l2, l3 = p["l1"], p["l2"], p["l3"]
        cg = torch.from_numpy(so3.path_table(l1, l2, l3)).to(sh)
        blk = torch.einsum("ijk,ej->eik", cg, sh[:, l2 * l2:(l2 + 1) * (l2 + 1)])
        M[:, p["m_off"]:p["m_off"] + (2 * l1 + 1) * (2 * l3 + 1)] = blk.reshape(sh.shape[0], -1)
    return M


def _x0(P):
    b = P.get("exp.bias.0")
    return P["exp.tp.weight"] if b is None else P["exp.tp.weight"] + b


def _scatter(e, dst, N, s):
    return torch.zeros((N, e.shape[1]), dtype=e.dtype, device=e.device).index_add(0, dst, e) * s


def full(P, table, proj_pairs, D, M, edge_scalars, dst, N, avg, h=None):
    """proj_pairs: LinearSpec.pairs of the projection; D: its output row length; M: coupling(table, sh); h: the hidden
    activation when it is an input of its own (a leaf in the tests)"""
    E = M.shape[0]
    w = F.linear(hidden(P, edge_scalars) if h is None else h, P["rad.net.6.weight"]) + P["rad.offset"]
    x0 = _x0(P)
    C = x0.numel()
    x = M.new_zeros((E, table.layout_in.dim))
    i0 = table.layout_in.seg_index(0, 1)
    o0 = table.layout_in.offsets[i0]
    x = torch.cat([x[:, :o0], x0.expand(E, C), x[:, o0 + C:]], 1)
    dtp = M.new_zeros((E, table.layout_out.dim))
    for p in table.paths:
        d1, d3, mul = 2 * p["l1"] + 1, 2 * p["l3"] + 1, p["mul"]
        xin = x[:, p["in_off"]:p["in_off"] + d1 * mul].reshape(E, d1, mul)
        c = M[:, p["m_off"]:p["m_off"] + d1 * d3].reshape(E, d1, d3)
        o = torch.einsum("eik,eiu->eku", c, xin) * w[:, None, p["w_off"]:p["w_off"] + mul]
        full_o = M.new_zeros((E, d3, p["out_k"]))
        full_o = torch.cat([full_o[:, :, :p["out_ch"]], o, full_o[:, :, p["out_ch"] + mul:]], 2)
        pad = M.new_zeros((E, table.layout_out.dim))
        dtp = dtp + torch.cat([pad[:, :p["out_off"]], full_o.reshape(E, -1), pad[:, p["out_off"] + d3 * p["out_k"]:]], 1)
    out = M.new_zeros((E, D))
    for (l, in_off, K, out_off, Nl, w_off) in proj_pairs:
        d = 2 * l + 1
        W = P["proj.tp.weight"][w_off:w_off + K * Nl].view(K, Nl)
        y = dtp[:, in_off:in_off + d * K].reshape(E, d, K) @ W
        if l == 0 and "proj.bias.0" in P:
            y = y + P["proj.bias.0"]
        out = out + torch.cat([out[:, :out_off] * 0, y.reshape(E, -1), out[:, out_off + d * Nl:] * 0], 1)
    return _scatter(out, dst, N, avg ** -0.5)


def fold(P, blocks, C):
    """(At [sum N, 64], a [sum N]) of the blocks, in their order"""
    x0 = _x0(P)
    W3, off, Wp = P["rad.net.6.weight"], P["rad.offset"], P["proj.tp.weight"]
    At, a = [], []
    for b in blocks:
        Wl = Wp[b["pw_off"]:b["pw_off"] + b["K"] * b["N"]].view(b["K"], b["N"])[b["out_ch"]:b["out_ch"] + C]
        At.append(torch.einsum("un,u,uj->nj", Wl, x0, W3[b["w_off"]:b["w_off"] + C]))
        a.append(torch.einsum("un,u,u->n", Wl, x0, off[b["w_off"]:b["w_off"] + C]))
    return torch.cat(At), torch.cat(a)


def scatter(z, blocks, M, bias, D, dst, N, s):
    E = z.shape[0]
    out = z.new_zeros((N, D))
    deg = torch.zeros(N, dtype=z.dtype, device=z.device).index_add(0, dst, torch.ones(E, dtype=z.dtype, device=z.device))
    zo = 0
    for b in blocks:
        d = 2 * b["l"] + 1
        e = M[:, b["m_off"]:b["m_off"] + d, None] * z[:, None, zo:zo + b["N"]]
        node = torch.zeros((N, d, b["N"]), dtype=z.dtype, device=z.device).index_add(0, dst, e)
        if b["l"] == 0 and bias is not None:
            node = node + deg[:, None, None] * bias
        o = b["node_off"]
        out = out + torch.cat([out[:, :o] * 0, node.reshape(N, -1), out[:, o + d * b["N"]:] * 0], 1)
        zo += b["N"]
    return out * s


def collapsed(P, blocks, C, D, M, edge_scalars, dst, N, avg, h=None):
    """blocks: ops.EdgeDegSpec(...).blocks; h: the hidden activation when it is an input of its own (a leaf in the tests)"""
    At, a = fold(P, blocks, C)
    h = hidden(P, edge_scalars) if h is None else h
    return scatter(h @ At.t() + a, blocks, M, P.get("proj.bias.0"), D, dst, N, avg ** -0.5)
