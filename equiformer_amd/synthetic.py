"""Synthetic molecule batches with the shapes BASELINE.json / SURVEY.md section 8(d) prescribe (no datasets offline)."""
import numpy as np
import torch

QM9_Z = np.array([1, 6, 7, 8, 9])
QM9_P = np.array([0.51, 0.35, 0.06, 0.07, 0.01])


def _sample_points(rng, n, side, min_dist):
    pts = []
    while len(pts) < n:
        p = rng.uniform(0.0, side, size=3)
        if all(np.linalg.norm(p - q) >= min_dist for q in pts):
            pts.append(p)
    return np.stack(pts)


def qm9_like_batch(num_molecules, atoms_per_molecule=18, side=6.5, min_dist=0.9, seed=0):
    """B molecules x N atoms, positions uniform in a cube of edge `side` (Angstrom) with a minimum pair distance.
    side=6.5 gives ~200 directed edges / molecule at r=5 (the north-star point), side=5.0 gives ~277 (QM9 statistics).
    Returns dict(pos [B*N,3] f32, z [B*N] i64 atomic numbers, batch [B*N] i64, y [B] f32)."""
    rng = np.random.default_rng(seed)
    pos = np.concatenate([_sample_points(rng, atoms_per_molecule, side, min_dist) for _ in range(num_molecules)])
    z = rng.choice(QM9_Z, size=num_molecules * atoms_per_molecule, p=QM9_P)
    batch = np.repeat(np.arange(num_molecules), atoms_per_molecule)
    y = rng.standard_normal(num_molecules)
    return dict(pos=torch.from_numpy(pos.astype(np.float32)), z=torch.from_numpy(z.astype(np.int64)),
                batch=torch.from_numpy(batch.astype(np.int64)), y=torch.from_numpy(y.astype(np.float32)))


# a plausible aspirin geometry (Angstrom): 9 C, 4 O, 8 H  [SURVEY.md section 8(d): Z = 6x9, 8x4, 1x8]
_ASPIRIN_Z = [6] * 9 + [8] * 4 + [1] * 8
_ASPIRIN_POS = np.array([
    [1.24, 0.72, 0.0], [2.45, 0.02, 0.0], [2.45, -1.38, 0.0], [1.24, -2.08, 0.0], [0.03, -1.38, 0.0],
    [0.03, 0.02, 0.0], [-1.25, 0.77, 0.1], [-1.10, -3.35, 0.9], [-2.10, -4.30, 1.4],
    [-1.35, 1.98, 0.3], [-2.33, -0.02, -0.1], [-1.17, -2.10, 0.2], [-0.20, -3.65, 1.3],
    [1.23, 1.81, 0.0], [3.39, 0.56, 0.0], [3.39, -1.93, 0.0], [1.25, -3.17, 0.0], [-3.12, 0.53, 0.0],
    [-1.70, -5.25, 1.8], [-2.80, -4.55, 0.6], [-2.70, -3.85, 2.2]]) * 0.85  # compact: ~350 directed edges at r=5


def md17_aspirin_batch(num_frames, jitter=0.05, seed=0):
    rng = np.random.default_rng(seed)
    n = len(_ASPIRIN_Z)
    pos = np.concatenate([_ASPIRIN_POS + rng.normal(0.0, jitter, size=(n, 3)) for _ in range(num_frames)])
    z = np.tile(np.array(_ASPIRIN_Z), num_frames)
    batch = np.repeat(np.arange(num_frames), n)
    return dict(pos=torch.from_numpy(pos.astype(np.float32)), z=torch.from_numpy(z.astype(np.int64)),
                batch=torch.from_numpy(batch.astype(np.int64)), y=torch.from_numpy(rng.standard_normal(num_frames).astype(np.float32)),
                dy=torch.from_numpy(rng.standard_normal((num_frames * n, 3)).astype(np.float32)))


def qm9_like_varying_batches(num_batches, num_molecules, atoms_range=(12, 24), side=6.5, min_dist=0.9, seed=0):
    """What a real loader yields: `num_batches` batches of `num_molecules` molecules whose atom counts are drawn uniformly from
    atoms_range (inclusive) -- different sizes inside a batch, different node / edge totals between batches.  A list of dicts
    like `qm9_like_batch`'s, plus num_graphs (int) and natoms [B] i64."""
    rng = np.random.default_rng(seed)
    lo, hi = int(atoms_range[0]), int(atoms_range[1])
    out = []
    for _ in range(num_batches):
        natoms = rng.integers(lo, hi + 1, size=num_molecules)
        pos = np.concatenate([_sample_points(rng, int(n), side, min_dist) for n in natoms])
        z = rng.choice(QM9_Z, size=int(natoms.sum()), p=QM9_P)
        batch = np.repeat(np.arange(num_molecules), natoms)
        y = rng.standard_normal(num_molecules)
        out.append(dict(pos=torch.from_numpy(pos.astype(np.float32)), z=torch.from_numpy(z.astype(np.int64)),
                        batch=torch.from_numpy(batch.astype(np.int64)), y=torch.from_numpy(y.astype(np.float32)),
                        num_graphs=int(num_molecules), natoms=torch.from_numpy(natoms.astype(np.int64))))
    return out


def oc20_like_varying_batches(num_batches, num_structures, atoms_range=(60, 96), cell=(11.0, 11.0, 30.0), seed=0):
    """What an OC20 loader yields: `num_batches` batches of `num_structures` slab-shaped periodic structures (orthorhombic cell
    with the given edge lengths in Angstrom, atoms uniform in its lower 45 %: slab + adsorbate below vacuum, SURVEY.md section
    8(d)) whose atom counts are drawn uniformly from atoms_range (inclusive).  A list of dicts: pos [N, 3] f32, atomic_numbers
    [N] i64 (1..83), tags [N] i64 (0..2), batch [N] i64 ascending, cell [B, 3, 3] f32, natoms [B] i64, num_graphs (int),
    y [B] f32 (energy targets)."""
    rng = np.random.default_rng(seed)
    lo, hi = int(atoms_range[0]), int(atoms_range[1])
    edge = np.asarray(cell, dtype=np.float64).reshape(3)
    out = []
    for _ in range(num_batches):
        natoms = rng.integers(lo, hi + 1, size=num_structures)
        n = int(natoms.sum())
        pos = rng.uniform(0.0, 1.0, size=(n, 3)) * np.array([1.0, 1.0, 0.45]) * edge
        cells = np.tile(np.diag(edge)[None], (num_structures, 1, 1))
        out.append(dict(pos=torch.from_numpy(pos.astype(np.float32)),
                        atomic_numbers=torch.from_numpy(rng.integers(1, 84, size=n).astype(np.int64)),
                        tags=torch.from_numpy(rng.integers(0, 3, size=n).astype(np.int64)),
                        batch=torch.from_numpy(np.repeat(np.arange(num_structures), natoms).astype(np.int64)),
                        cell=torch.from_numpy(cells.astype(np.float32)), natoms=torch.from_numpy(natoms.astype(np.int64)),
                        num_graphs=int(num_structures), y=torch.from_numpy(rng.standard_normal(num_structures).astype(np.float32))))
    return out


def attach_given_edges(batch, radius, max_num_neighbors=50):
    """The fields an OC20 LMDB adds to a periodic batch (the reference's otf_graph=False contract), taken from the GPU neighbour
    search (EdgeGraph.from_radius_pbc) at the given radius and cap: `edge_index` [2, E] int64 (neighbour, centre), `cell_offsets`
    [E, 3] int64, `neighbors` [B] int64 (edges per structure).  batch: a dict of oc20_like_varying_batches with its tensors on the
    GPU; returns a new dict on the same device (the tensors of `batch` are shared, not copied)."""
    from .graph import EdgeGraph
    B = int(batch["num_graphs"]) if "num_graphs" in batch else int(batch["cell"].reshape(-1, 3, 3).shape[0])
    g, _, cell_offsets = EdgeGraph.from_radius_pbc(batch["pos"], batch["cell"], batch["batch"], radius,
                                                   max_num_neighbors=max_num_neighbors, num_graphs=B)
    ends = g.row_ptr.long()[g.mol_ptr.long()]  # first edge of every structure's first row, and the edge count
    out = dict(batch)
    out["edge_index"] = torch.stack([g.src.long(), g.dst.long()])
    out["cell_offsets"] = cell_offsets.long()
    out["neighbors"] = ends[1:] - ends[:-1]
    return out
