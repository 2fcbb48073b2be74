"""ocpmodels-style batches that carry their own periodic edge list (`edge_index`, `cell_offsets`, `neighbors`, `cell`), shared by
tests/test_given_edges.py (CPU: the inputs have the properties the GPU tests rely on) and tests/test_gpu_given_edges.py (GPU:
EdgeGraph.from_edges_pbc and the step classes with edges="batch" on those inputs).  The edge lists come from oracle/pbc.py on the
structures of tests/periodic_inputs.py; `expected` is the pure-torch statement of what the builder has to return.  Plain CPU
tensors; nothing here touches a GPU.  Cases and expectations are built once per process and must be left unchanged."""
import functools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import periodic_inputs as pi  # noqa: E402

R = pi.R
FIELDS = ("pos", "cell", "batch", "edge_index", "cell_offsets", "neighbors")


def attach(d, cap, dtype=torch.int64):
    """d (pos, cell, batch, natoms) + the oracle's search at radius R and `cap` neighbours, edges as the search emits them"""
    from oracle import pbc
    natoms = [int(n) for n in d["natoms"]]
    ei, co, nb = pbc.radius_graph_pbc(d["pos"], d["cell"], natoms, R, cap)
    out = dict(d, natoms=natoms, edge_index=ei.to(dtype), cell_offsets=co.to(dtype), neighbors=nb)
    return out


def shuffled(d, seed=0):
    """the same batch with the edges permuted INSIDE every structure's range (never across)"""
    g = torch.Generator().manual_seed(seed)
    perm, start = [], 0
    for n in d["neighbors"].tolist():
        perm.append(start + torch.randperm(n, generator=g))
        start += n
    perm = torch.cat(perm) if perm else torch.zeros(0, dtype=torch.long)
    return dict(d, edge_index=d["edge_index"][:, perm].contiguous(), cell_offsets=d["cell_offsets"][perm].contiguous())


def reordered(d, structures):
    """the structures of d (pos, cell, batch, natoms) in another order"""
    ptr = [0]
    for n in d["natoms"]:
        ptr.append(ptr[-1] + int(n))
    natoms = [int(d["natoms"][s]) for s in structures]
    pos = torch.cat([d["pos"][ptr[s]:ptr[s + 1]] for s in structures])
    return dict(pos=pos, cell=d["cell"][list(structures)].clone(), batch=pi._batch_of(natoms), natoms=natoms)


def with_structure(d, pos, cell):
    """d plus one more structure at the end"""
    natoms = [int(n) for n in d["natoms"]] + [int(pos.shape[0])]
    return dict(pos=torch.cat([d["pos"], pos]), cell=torch.cat([d["cell"], cell[None]]), batch=pi._batch_of(natoms), natoms=natoms)


def insert_self_loops(d, structure, where):
    """zero-length edges (j == i, zero image) inserted into the input range of `structure`, at the positions `where` of the range
    as it is AFTER the insertions (ascending); `neighbors` raised to match.  The looped atom is the structure's first."""
    nb = d["neighbors"].clone()
    start = int(nb[:structure].sum())
    node = sum(int(n) for n in d["natoms"][:structure])
    ei, co = d["edge_index"], d["cell_offsets"]
    for w in where:
        at = start + int(w)
        loop = torch.full((2, 1), node, dtype=ei.dtype)
        ei = torch.cat([ei[:, :at], loop, ei[:, at:]], dim=1)
        co = torch.cat([co[:at], torch.zeros((1, 3), dtype=co.dtype), co[at:]])
        nb[structure] += 1
    return dict(d, edge_index=ei.contiguous(), cell_offsets=co.contiguous(), neighbors=nb)


def _lone_atoms(n):
    natoms = [1] * n
    cell = 20.0 * torch.eye(3)[None].repeat(n, 1, 1)
    pos = torch.tensor([[1.0 + i, 2.0, 3.0] for i in range(n)])
    return dict(pos=pos, cell=cell, batch=pi._batch_of(natoms), natoms=natoms)


def joined(*ds):
    """the structures of several batches (pos, cell, batch, natoms) in one"""
    natoms = [int(n) for d in ds for n in d["natoms"]]
    return dict(pos=torch.cat([d["pos"] for d in ds]), cell=torch.cat([d["cell"] for d in ds]), batch=pi._batch_of(natoms),
                natoms=natoms)


TRICLINIC_ATOMS = 9    # one structure of 9 atoms: ~590 edges, more than two passes of the fill kernel (EDGES_PASS = 256) ...
TRICLINIC_SMALL = 4    # ... and three of 4 atoms (~110 edges each): four structures, as the "dropped" case has (a padded refill)
DROP_STRUCTURE = 1    # the structure of the "dropped" case that receives the three zero-length edges


@functools.lru_cache(maxsize=None)
def cases():
    """{name: batch} -- see the issue's list: in order, shuffled, empty structure (three placements), dropped, truncated, no edges"""
    out = {}
    out["in order"] = attach(pi.small_cubic(), 500)
    tri = joined(pi.small_triclinic(seed=5, structures=1, atoms=TRICLINIC_SMALL), pi.small_triclinic(structures=1, atoms=TRICLINIC_ATOMS),
                 pi.small_triclinic(seed=7, structures=2, atoms=TRICLINIC_SMALL))
    out["shuffled"] = shuffled(attach(tri, 500, torch.int32), seed=1)
    empty = pi.with_an_empty_structure()
    out["empty structure"] = attach(empty, 50)
    out["empty structure first"] = attach(reordered(empty, (1, 0, 2)), 50)
    out["empty structure last"] = attach(reordered(empty, (0, 2, 1)), 50)
    # dropped edges: three zero-length edges in structure 1 (first, middle, last place of its range) and a one-atom structure in a
    # 20 A cell (no edge at r = 5) that is given ONE edge, a zero-length self-loop: its row and the whole structure are dropped
    tri = with_structure(pi.small_triclinic(), torch.tensor([[1.0, 1.0, 1.0]]), 20.0 * torch.eye(3))
    d = attach(tri, 500)
    assert int(d["neighbors"][-1]) == 0
    n1 = int(d["neighbors"][DROP_STRUCTURE])
    d = insert_self_loops(d, DROP_STRUCTURE, (0, (n1 + 3) // 2, n1 + 2))
    d = insert_self_loops(d, len(d["natoms"]) - 1, (0,))
    out["dropped"] = d
    out["truncated"] = attach(pi.dense_cells(), pi.DENSE_CAP)
    lone = _lone_atoms(3)
    out["no edges"] = dict(lone, edge_index=torch.zeros((2, 0), dtype=torch.long), cell_offsets=torch.zeros((0, 3), dtype=torch.long),
                           neighbors=torch.zeros(3, dtype=torch.long))
    return out


def _scan(counts):
    return torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)])


def expected_of(d):
    """What EdgeGraph.from_edges_pbc has to return for the batch d, in pure torch (fp64 geometry, stable sorts):
    keep [E_in] bool (get_pbc_distances in fp64: zero-length edges dropped), order [E] (input index of the edge in every slot: the
    stable argsort of the kept destinations), src / dst / row_ptr / cell_offsets / src_perm / src_ptr / batch / mol_ptr (int32),
    offsets [E, 3] fp64 and offsets_bound [E, 3] = 4 * 2^-24 * sum_k |n_k cell_kj|."""
    pos, cell = d["pos"].double(), d["cell"].double()
    N, B = pos.shape[0], cell.shape[0]
    ei, co, nb = d["edge_index"].long(), d["cell_offsets"].long(), d["neighbors"].long()
    per_edge = torch.repeat_interleave(cell, nb, dim=0)
    terms = co.double()[:, :, None] * per_edge  # [E_in, k, j]
    cart = terms.sum(1)
    vec = pos[ei[0]] - pos[ei[1]] + cart
    keep = vec.norm(dim=-1) != 0
    kept = keep.nonzero().view(-1)
    order = kept[torch.argsort(ei[1][kept], stable=True)]
    src, dst = ei[0][order], ei[1][order]
    i32 = torch.int32
    return dict(keep=keep, order=order.to(i32), src=src.to(i32), dst=dst.to(i32),
                row_ptr=_scan(torch.bincount(dst, minlength=N)).to(i32), cell_offsets=co[order].to(i32),
                offsets=cart[order], offsets_bound=4.0 * 2.0 ** -24 * terms.abs().sum(1)[order],
                src_perm=torch.argsort(src, stable=True).to(i32), src_ptr=_scan(torch.bincount(src, minlength=N)).to(i32),
                batch=d["batch"].to(i32), mol_ptr=_scan(torch.bincount(d["batch"], minlength=B)).to(i32), lengths=vec.norm(dim=-1))


@functools.lru_cache(maxsize=None)
def expected(name):
    return expected_of(cases()[name])


def slab_batches_with_edges(n=16, seed=0, shuffle_seed=7):
    """periodic_inputs.slab_batches(n) with the oracle's edge lists at R / SLAB_CAP attached, shuffled inside every structure"""
    out = []
    for k, d in enumerate(pi.slab_batches(n, seed)):
        e = shuffled(attach(dict(d, natoms=d["natoms"].tolist()), pi.SLAB_CAP), seed=shuffle_seed + k)
        out.append(dict(e, natoms=d["natoms"]))
    return out
