"""Size-independent properties of the HIP path at BASELINE.json's full sizes (where the CPU oracle would take minutes),
and the degenerate inputs: molecules without edges, a batch without any edge.
Wall time of this file on an MI355X, one run each (pytest's figure): 3.7 s at the parent commit, 3.8 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py)."""
import math

import pytest
import torch

from oracle import nets as onets
from poison import poisoned_model  # noqa: E402,F401  (the fixture of the tests that run on poisoned, guarded allocations)

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rot(seed):
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    if torch.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q.float()


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def test_qm9_full_batch_invariances():
    """128 molecules x 18 atoms (the bench workload): energies are invariant under a global rotation + translation,
    under a permutation of the atoms inside every molecule, and do not depend on the other molecules of the batch."""
    from equiformer_amd import nets
    from equiformer_amd.synthetic import qm9_like_batch
    dev = _dev()
    torch.manual_seed(0)
    model = nets.model_entrypoint("graph_attention_transformer_nonlinear_l2")(irreps_in="5x0e", radius=5.0,
                                                                               num_basis=128).to(dev).eval()
    d = {k: v.to(dev) for k, v in qm9_like_batch(128, 18, side=6.5, seed=11).items()}
    with torch.no_grad():
        y = model(f_in=None, pos=d["pos"], batch=d["batch"], node_atom=d["z"])
        R = _rot(1).to(dev)
        y_rot = model(f_in=None, pos=d["pos"] @ R.T + torch.tensor([0.3, -1.2, 2.0], device=dev), batch=d["batch"],
                      node_atom=d["z"])
        g = torch.Generator().manual_seed(2)
        perm = torch.cat([m * 18 + torch.randperm(18, generator=g) for m in range(128)]).to(dev)
        y_perm = model(f_in=None, pos=d["pos"][perm], batch=d["batch"], node_atom=d["z"][perm])
        half = 64 * 18
        y_a = model(f_in=None, pos=d["pos"][:half], batch=d["batch"][:half], node_atom=d["z"][:half])
        y_b = model(f_in=None, pos=d["pos"][half:], batch=d["batch"][half:] - 64, node_atom=d["z"][half:])
    assert y.shape == (128, 1) and torch.isfinite(y).all()
    print("rotation %.2e  permutation %.2e  batch split %.2e"
          % (_rel(y_rot, y), _rel(y_perm, y), _rel(torch.cat([y_a, y_b]), y)))
    assert _rel(y_rot, y) < 1e-4 and _rel(y_perm, y) < 1e-4 and _rel(torch.cat([y_a, y_b]), y) < 1e-5


def test_md17_forces_equivariant_and_sum_to_zero():
    from equiformer_amd import nets
    from equiformer_amd.synthetic import md17_aspirin_batch
    dev = _dev()
    torch.manual_seed(0)
    model = nets.model_entrypoint("graph_attention_transformer_nonlinear_exp_l2_md17")(
        irreps_in="64x0e", radius=5.0, num_basis=32).to(dev).eval()
    d = {k: v.to(dev) for k, v in md17_aspirin_batch(8, seed=3).items()}
    E, F = model(node_atom=d["z"], pos=d["pos"], batch=d["batch"])
    R = _rot(5).to(dev)
    E2, F2 = model(node_atom=d["z"], pos=d["pos"] @ R.T, batch=d["batch"])
    assert _rel(E2, E) < 1e-4 and _rel(F2, F @ R.T) < 1e-4
    net = torch.zeros(8, 3, device=dev).index_add(0, d["batch"], F)
    assert float(net.abs().max()) < 1e-4 * float(F.abs().max()) * math.sqrt(21)


@pytest.mark.usefixtures("poisoned_model")
def test_molecules_without_edges_and_empty_graph():
    """A single-atom molecule and a far-apart pair have no edges: their energy comes from the embeddings alone and
    must equal the oracle's; a batch in which NO molecule has an edge (E = 0 everywhere on the path) runs as well."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as mg
    from weights import fill_deterministic
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    dev = _dev()
    kw = dict(irreps_in="5x0e", max_radius=5.0, number_of_basis=32, **mg.SMALL_L2)
    ref = fill_deterministic(onets.GraphAttentionTransformer(**kw), 9).double().eval()
    mod = fill_deterministic(GraphAttentionTransformer(**kw), 9).to(dev).eval()
    g = torch.Generator().manual_seed(4)
    pos = torch.cat([torch.rand(6, 3, generator=g) * 3.0,            # ordinary molecule
                     torch.zeros(1, 3),                               # single atom
                     torch.tensor([[0.0, 0.0, 0.0], [9.0, 0.0, 0.0]]),  # pair beyond the cut-off
                     torch.rand(5, 3, generator=g) * 3.0])
    batch = torch.tensor([0] * 6 + [1] + [2] * 2 + [3] * 5)
    z = torch.tensor([1, 6, 7, 8, 9, 6, 8, 1, 6, 6, 1, 1, 7, 8])
    with torch.no_grad():
        yr = ref(None, pos.double(), batch, z)
        y = mod(None, pos.to(dev), batch.to(dev), z.to(dev))
        assert _rel(y, yr) < 1e-4, (y, yr)
        # no edge at all (the reference's Vec2AttnHeads cannot reshape an empty edge tensor, so there is no oracle
        # value; the energies must be those the same molecules get inside the mixed batch above)
        sel = torch.tensor([6, 7, 8])
        b2 = torch.tensor([0, 1, 1])
        y2 = mod(None, pos[sel].to(dev), b2.to(dev), z[sel].to(dev))
        assert torch.isfinite(y2).all() and _rel(y2, y[1:3]) < 1e-5
    # and the backward pass of the edge-free batch is finite
    y3 = mod(None, pos[sel].to(dev), b2.to(dev), z[sel].to(dev))
    y3.sum().backward()
    assert all(torch.isfinite(p.grad).all() for p in mod.parameters() if p.grad is not None)
