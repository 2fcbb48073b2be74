"""Inputs of tests/test_gpu_graph_edges.py (TEST INFRASTRUCTURE): radius-graph batches, periodic structures and edge-geometry
graphs at the edges of csrc/graph.hip and csrc/geom.h.  Plain CPU tensors; nothing here touches a GPU or the HIP library.
tests/test_graph_edge_inputs.py proves from the oracle alone that every case is DECIDABLE: no float32 rounding of a distance
can move a pair across a bound or change which candidates a truncated periodic row keeps.

  no ambiguous pair   the float64 squared distance of the float32 positions of every same-structure pair (and every periodic
                      image) differs from r^2 by more than MARGIN * r^2 -- unless it EQUALS r^2: pairs a case places on the
                      bound with integer or dyadic coordinates are computed exactly in either precision.  Periodic
                      candidates stay clear of the lower bound 1e-4 in the same way (this builder keeps them outside
                      [0.5e-4, 1.5e-4], far more than MARGIN asks).
  no ambiguous cut    in a truncated periodic row the max_nbr-th and the next candidate (float64 distance order) differ by
                      more than MARGIN relative.  Exempt: two mirror images (j == i, n) and (j == i, -n), and the ties of a
                      case flagged `exact` (integer / dyadic cell and positions): those distances are equal in any precision
                      and are cut in candidate order by the oracle and by the kernel alike.
Random structures are drawn again (next seed, per structure) until both hold.
"""
import math

import torch

from oracle import nets as onets
from oracle import pbc

MARGIN = 1e-4          # relative clearance of a squared distance from a bound, and of the two candidates around a cut
LOW = 1e-4             # lower bound of the periodic search (squared distance)
LOW_CLEAR = 0.5e-4     # periodic candidates keep |d^2 - LOW| above this


def batch_of(sizes):
    return torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(sizes)] or [torch.zeros(0, dtype=torch.long)])


def _f32(t):
    """float32-rounded values (what the kernels receive)"""
    return t.to(torch.float32)


# ------------------------------------------------------------------------------------------------- decidability
def pair_d2(pos):
    """float64 squared distances of the float32-rounded positions of ONE molecule, [n, n]"""
    p = pos.float().double()
    return (p[:, None, :] - p[None, :, :]).pow(2).sum(-1)


def ambiguous_pairs(pos, r):
    """pairs i != j of one molecule whose squared distance is within MARGIN r^2 of r^2 without being equal to it"""
    d2 = pair_d2(pos)
    r2 = float(r) * float(r)
    off = ~torch.eye(d2.shape[0], dtype=torch.bool)
    return int((off & ((d2 - r2).abs() <= MARGIN * r2) & (d2 != r2)).sum())


def pbc_candidates(pos, cell, r):
    """(d2 [n, n * I] float64 in the kernel's candidate order (j, n1, n2, n3), j_of [n * I], image_of [n * I, 3]) of ONE
    periodic structure, every image of the repeat box, whether or not it survives the distance test"""
    p, c = pos.float().double(), cell.float().double()
    r1, r2_, r3 = pbc.cell_repeats(c, r)
    imgs = torch.tensor([(i, j, k) for i in range(-r1, r1 + 1) for j in range(-r2_, r2_ + 1) for k in range(-r3, r3 + 1)],
                        dtype=torch.float64)
    d = (p[None, :, None, :] + (imgs @ c)[None, None, :, :] - p[:, None, None, :]).pow(2).sum(-1)  # [i, j, I]
    n, I = p.shape[0], imgs.shape[0]
    return d.reshape(n, n * I), torch.arange(n).repeat_interleave(I), imgs.long().repeat(n, 1)


def pbc_ambiguous_pairs(pos, cell, r):
    """candidates within MARGIN r^2 of r^2 (not equal to it), plus candidates within LOW_CLEAR of the lower bound"""
    d2, _, _ = pbc_candidates(pos, cell, r)
    r2 = float(r) * float(r)
    hi = ((d2 - r2).abs() <= MARGIN * r2) & (d2 != r2)
    lo = (d2 - LOW).abs() <= LOW_CLEAR
    return int(hi.sum()) + int(lo.sum())


def pbc_ambiguous_cuts(pos, cell, r, max_nbr, exact=False):
    """truncated rows whose max_nbr-th and next candidate are closer than MARGIN relative (exemptions: module docstring)"""
    d2, j_of, img = pbc_candidates(pos, cell, r)
    r2 = float(r) * float(r)
    bad = 0
    for i in range(d2.shape[0]):
        keep = ((d2[i] <= r2) & (d2[i] > LOW)).nonzero().flatten()
        if keep.numel() <= max_nbr:
            continue
        order = torch.sort(d2[i][keep], stable=True).indices
        a, b = keep[order[max_nbr - 1]], keep[order[max_nbr]]
        da, db = float(d2[i][a]), float(d2[i][b])
        if abs(db - da) > MARGIN * db:
            continue
        tie = da == db
        mirror = tie and int(j_of[a]) == i and int(j_of[b]) == i and bool((img[a] == -img[b]).all())
        if not (mirror or (tie and exact)):
            bad += 1
    return bad


def truncated_rows(pos, cell, r, max_nbr):
    d2, _, _ = pbc_candidates(pos, cell, r)
    r2 = float(r) * float(r)
    return int((((d2 <= r2) & (d2 > LOW)).sum(1) > max_nbr).sum())


# ------------------------------------------------------------------------------------------------- radius-graph cases
LATTICE = [(0, 0, 0), (3, 4, 0), (0, 0, 5), (3, 0, 0), (0, 4, 3), (6, 8, 0)]
RAGGED_SIZES = [1, 2, 63, 64, 65, 0, 129, 3, 0]   # around the 64-thread stride; an empty id in the middle and one at the end


def _molecule(n, r, seed):
    """n atoms uniform in a cube that holds ~12 neighbours per atom at cut-off r; drawn again until no pair is ambiguous"""
    side = max(1.5 * r, (n * 4.19 * r ** 3 / 12.0) ** (1.0 / 3.0))
    for k in range(1000):
        g = torch.Generator().manual_seed(100003 * seed + k)
        pos = _f32(torch.rand(n, 3, generator=g, dtype=torch.float64) * side)
        if ambiguous_pairs(pos, r) == 0:
            return pos
    raise AssertionError("no unambiguous molecule found")


def molecules(sizes, r, seed):
    pos = [_molecule(n, r, seed * 1000 + i) for i, n in enumerate(sizes) if n > 0]
    return dict(pos=torch.cat(pos) if pos else torch.zeros(0, 3), batch=batch_of(sizes), sizes=list(sizes), r=float(r),
                num_graphs=len(sizes))


def radius_cases():
    """name -> dict(pos f32 [N,3], batch [N], sizes, r, num_graphs)"""
    lat = dict(pos=torch.tensor(LATTICE, dtype=torch.float32), batch=torch.zeros(6, dtype=torch.long), sizes=[6], r=5.0,
               num_graphs=1)
    return {
        "lattice": lat,                                   # 8 ordered pairs at d^2 = r^2 exactly, excluded by the strict <
        "ragged": molecules(RAGGED_SIZES, 3.0, 1),
        "n1024": molecules([32] * 32, 2.5, 2),            # exactly 1024 nodes: the scan's last one-element chunks
        "n1040": molecules([40] * 26, 2.5, 3),            # more than 1024 nodes: chunks of 2
        "trunc": molecules([5, 20, 1, 13], 3.0, 4),       # the batch of the max_num_neighbors sweep
    }


def coincident_case():
    """atoms 0 and 1 coincide (a zero-length edge both ways), atom 2 is 1.5 away"""
    pos = torch.tensor([[0.5, 1.0, -2.0], [0.5, 1.0, -2.0], [0.5, 2.5, -2.0]], dtype=torch.float32)
    return dict(pos=pos, batch=torch.zeros(3, dtype=torch.long), sizes=[3], r=5.0, num_graphs=1)


def radius_reference(case, max_num_neighbors=1000, dtype=torch.float64):
    """(src, dst) of oracle.nets.radius_graph on the case's float32 positions cast to `dtype`"""
    return onets.radius_graph(case["pos"].float().to(dtype), case["r"], case["batch"], max_num_neighbors=max_num_neighbors)


# ------------------------------------------------------------------------------------------------- periodic cases
def _structure(n, cell, r, caps, seed):
    """n atoms at random fractional coordinates of `cell`, drawn again until pairs and cuts are unambiguous"""
    for k in range(1000):
        g = torch.Generator().manual_seed(100003 * seed + k)
        pos = _f32(torch.rand(n, 3, generator=g, dtype=torch.float64) @ cell.double())
        if pbc_ambiguous_pairs(pos, cell, r) == 0 and all(pbc_ambiguous_cuts(pos, cell, r, c) == 0 for c in caps):
            return pos
    raise AssertionError("no unambiguous structure found")


def _pbc_case(structs, r, caps, exact=False):
    """structs: [(pos, cell)]"""
    natoms = [int(p.shape[0]) for p, _ in structs]
    return dict(pos=torch.cat([_f32(p) for p, _ in structs]), cell=torch.stack([_f32(c) for _, c in structs]),
                natoms=natoms, batch=batch_of(natoms), r=float(r), caps=list(caps), exact=exact)


LEFT_HANDED = [[1.5, 5.5, 0.0], [6.0, 0.0, 0.0], [0.8, -1.1, 7.0]]      # rows 0 and 1 of a right-handed cell exchanged: det < 0
SKEWED = [[2.2, 0.0, 0.0], [0.7, 3.1, 0.0], [0.4, -0.6, 6.3]]           # repeats [3, 2, 1] at r = 5
SLAB = [[11.0, 0.0, 0.0], [0.0, 11.0, 0.0], [0.0, 0.0, 25.0]]
CAPS = [1, 9, 50]


def pbc_cases():
    """name -> dict(pos, cell [B,3,3], natoms, batch, r, caps (the max_nbr values the case is run at), exact)"""
    T = lambda rows: torch.tensor(rows, dtype=torch.float32)  # noqa: E731
    one = torch.zeros(1, 3)
    r = 5.0
    close = torch.tensor([[1.0, 1.0, 1.0], [1.005, 1.0, 1.0], [4.1, 3.7, 4.4], [4.12, 3.7, 4.4], [6.5, 2.25, 5.3]])
    cases = {
        "cubic_a3": _pbc_case([(one, 3.0 * torch.eye(3))], r, [1000, 4], exact=True),      # 18 edges; a six-way tie at the cut
        "cubic_a2.5": _pbc_case([(one, 2.5 * torch.eye(3))], r, [1000], exact=True),       # 32 edges, six of them at d = r
        "close_pairs": _pbc_case([(close, 8.0 * torch.eye(3))], r, CAPS),                   # 0.005 apart: dropped; 0.02: kept
        "cells": _pbc_case([(_structure(7, T(LEFT_HANDED), r, CAPS, 11), T(LEFT_HANDED)),
                            (_structure(3, T(SKEWED), r, CAPS, 12), T(SKEWED)),
                            (_structure(30, T(SLAB), r, CAPS, 13), T(SLAB))], r, CAPS),
        "sizes": _pbc_case([(_structure(1, T(LEFT_HANDED), r, CAPS, 14), T(LEFT_HANDED)),
                            (_structure(2, T([[6.0, 0.0, 0.0], [0.0, 5.0, 0.0], [0.0, 0.0, 7.0]]), r, CAPS, 15),
                             T([[6.0, 0.0, 0.0], [0.0, 5.0, 0.0], [0.0, 0.0, 7.0]])),
                            (_structure(65, T(SLAB), r, CAPS, 16), T(SLAB))], r, CAPS),
    }
    return cases


def pbc_structures(case):
    """[(pos, cell)] of a case"""
    out, start = [], 0
    for b, n in enumerate(case["natoms"]):
        out.append((case["pos"][start:start + n], case["cell"][b]))
        start += n
    return out


def pbc_reference(case, max_nbr, dtype=torch.float64):
    """(edge_index [2,E] = (neighbour, centre), cell_offsets [E,3], neighbours per structure) of oracle.pbc.radius_graph_pbc"""
    return pbc.radius_graph_pbc(case["pos"].float().to(dtype), case["cell"].float().to(dtype), case["natoms"], case["r"],
                                max_nbr)


# ------------------------------------------------------------------------------------------------- edge-geometry graphs
# Special directions, each realised EXACTLY: the destination of a special edge sits at the origin and, without offsets, its
# source at the vector itself (with offsets: both at the origin and the vector is the edge's offset), so the kernel's
# pos[src] - pos[dst] (+ offset) is that float32 vector bit for bit.  y is the polar axis of the harmonics.
_S = 1.0 / math.sqrt(2.0)
SPECIAL_DIRECTIONS = [
    (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),                       # the six axes
    (_S, _S, 0), (0.6, -0.8, 0), (0, _S, -_S), (0, 0.28, 0.96), (_S, 0, _S), (-0.8, 0, 0.6),   # the three coordinate planes
    (1e-4, 1, 0), (-6e-5, 1, 5e-5), (3e-6, -1, -1e-6), (0, -1, 1e-4), (7e-5, -1, 7e-5),        # within 1e-4 of +-y
]
SPECIAL_LENGTHS = [1.0, 1e-3, 20.0, 0.01, 5.0, 0.1, 2.5]    # cycled over the special edges: lengths from 1e-3 to 20
GEOM_POOL = 12         # nodes with incoming AND outgoing edges (random edges run among them)
GEOM_ISOLATED = 5      # nodes without any edge


def geometry_case(E, with_offsets, seed):
    """dict(pos [N,3], src [E], dst [E], offsets [E,3] or None, N, isolated, only_out, only_in): min(E, 17) special edges on
    dedicated node pairs (their sources have no incoming, their destinations no outgoing edge), the rest random edges among
    GEOM_POOL nodes on a 1/64 grid (float32 subtracts grid points exactly: the direction the kernel sees is the one the
    float64 reference sees), then GEOM_ISOLATED nodes that no edge touches.  Edge e is special edge (e + seed) mod 17."""
    g = torch.Generator().manual_seed(seed)
    ns = min(E, len(SPECIAL_DIRECTIONS))
    pos, src, dst, off = [], [], [], []
    for k in range(ns):
        d = torch.tensor(SPECIAL_DIRECTIONS[(k + seed) % len(SPECIAL_DIRECTIONS)], dtype=torch.float64)
        v = (d * SPECIAL_LENGTHS[(k + seed) % len(SPECIAL_LENGTHS)]).float()
        src.append(2 * k), dst.append(2 * k + 1)
        pos += [torch.zeros(3) if with_offsets else v, torch.zeros(3)]
        off.append(v if with_offsets else torch.zeros(3))
    base = 2 * ns
    while True:  # pool positions: pairwise distinct grid points in [-4, 4]^3
        pool = torch.randint(-256, 257, (GEOM_POOL, 3), generator=g).float() / 64.0
        if torch.unique(pool, dim=0).shape[0] == GEOM_POOL:
            break
    pos += list(pool)
    for _ in range(E - ns):
        a, b = torch.randperm(GEOM_POOL, generator=g)[:2].tolist()
        src.append(base + a), dst.append(base + b)
        o = torch.randint(-512, 513, (3,), generator=g).float() / 64.0
        while with_offsets and bool((pool[a] - pool[b] + o == 0).all()):
            o = torch.randint(-512, 513, (3,), generator=g).float() / 64.0
        off.append(o)
    iso0 = len(pos)
    pos += list(torch.randint(-256, 257, (GEOM_ISOLATED, 3), generator=g).float() / 64.0)
    N = len(pos)
    return dict(pos=torch.stack(pos), src=torch.tensor(src, dtype=torch.long), dst=torch.tensor(dst, dtype=torch.long),
                offsets=torch.stack(off) if with_offsets else None, N=N, isolated=list(range(iso0, N)),
                only_out=[2 * k for k in range(ns)], only_in=[2 * k + 1 for k in range(ns)])


def geometry_vectors(case):
    """float64 edge vectors pos[src] - pos[dst] (+ offsets) of the float32 inputs"""
    p = case["pos"].float().double()
    v = p[case["src"]] - p[case["dst"]]
    return v if case["offsets"] is None else v + case["offsets"].float().double()
