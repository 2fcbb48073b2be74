"""Periodic inputs shared by tests/test_periodic_capture.py (CPU: the inputs really have repeated (source, destination) pairs
and truncated rows, checked with oracle/pbc.py) and tests/test_gpu_periodic_capture.py (GPU: the kernels on those inputs).
Plain CPU tensors; nothing here touches a GPU."""
import torch

R = 5.0
SLAB_CELL = (8.0, 8.0, 20.0)
SLAB_CAP = 50          # max_neighbors of the slab batches
DENSE_CAP = 10         # max_neighbors of the dense cells: far below their ~50 candidates per atom, every row is truncated


def _batch_of(natoms):
    return torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(natoms)])


def small_triclinic(seed=3, structures=3, atoms=7, side=4.0):
    """`structures` x `atoms` atoms in cells side * I + 0.3 * rand: with r = 5 every neighbour is seen through several images."""
    g = torch.Generator().manual_seed(seed)
    cell = side * torch.eye(3)[None].repeat(structures, 1, 1) + 0.3 * torch.rand(structures, 3, 3, generator=g)
    frac = torch.rand(structures * atoms, 3, generator=g)
    natoms = [atoms] * structures
    batch = _batch_of(natoms)
    pos = torch.bmm(frac[:, None, :], cell[batch]).squeeze(1)
    return dict(pos=pos, cell=cell, batch=batch, natoms=natoms)


def small_cubic(seed=4):
    """2 x 10 atoms, cubic cells of side 6.0"""
    g = torch.Generator().manual_seed(seed)
    natoms = [10, 10]
    cell = 6.0 * torch.eye(3)[None].repeat(2, 1, 1)
    pos = torch.rand(20, 3, generator=g) * 6.0
    return dict(pos=pos, cell=cell, batch=_batch_of(natoms), natoms=natoms)


def with_an_empty_structure(seed=5):
    """three structures; the middle one is a single atom in a 20 A cell: no edge at r = 5 (its own images are 20 A away)"""
    g = torch.Generator().manual_seed(seed)
    natoms = [6, 1, 5]
    cell = torch.stack([5.0 * torch.eye(3), 20.0 * torch.eye(3), 4.5 * torch.eye(3)])
    batch = _batch_of(natoms)
    pos = torch.bmm(torch.rand(12, 3, generator=g)[:, None, :], cell[batch]).squeeze(1)
    return dict(pos=pos, cell=cell, batch=batch, natoms=natoms)


def dense_cells(seed=6, jitter=0.0, jitter_seed=0):
    """3 x 12 atoms in cells 5.0 * I + 0.3 * rand (~50 candidates per atom): with max_neighbors = DENSE_CAP every row is truncated,
    so the edge COUNT is 36 * DENSE_CAP whatever the positions are, while the edge LIST follows them.  jitter: Gaussian
    displacement (Angstrom) of every atom, drawn from jitter_seed."""
    d = small_triclinic(seed, 3, 12, 5.0)
    if jitter:
        d["pos"] = d["pos"] + jitter * torch.randn(d["pos"].shape, generator=torch.Generator().manual_seed(1000 + jitter_seed))
    return d


def slab_batches(n=16, seed=0):
    """n batches of 4 slab structures of 20-36 atoms in an 8 x 8 x 20 A cell (equiformer_amd.synthetic)"""
    from equiformer_amd.synthetic import oc20_like_varying_batches
    return oc20_like_varying_batches(n, 4, (20, 36), cell=SLAB_CELL, seed=seed)


def repeated_pairs(src, dst, n_nodes):
    """edges whose (source, destination) pair occurred before, and the largest multiplicity of a pair"""
    key = src.long() * int(n_nodes) + dst.long()
    _, counts = torch.unique(key, return_counts=True)
    return int((counts - 1).sum()), int(counts.max()) if counts.numel() else 0
