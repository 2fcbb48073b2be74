"""The cases of tests/graph_edge_inputs.py are decidable and their known answers hold -- from the oracle alone, on the CPU.
Nothing here loads the HIP library."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_edge_inputs as gi  # noqa: E402
from oracle import e3 as oe3  # noqa: E402
from oracle import nets as onets  # noqa: E402
from oracle import pbc  # noqa: E402


@pytest.fixture(scope="module")
def radius_cases():
    return gi.radius_cases()


@pytest.fixture(scope="module")
def pbc_cases():
    return gi.pbc_cases()


def _per_molecule(case):
    start = 0
    for n in case["sizes"]:
        yield case["pos"][start:start + n]
        start += n


# ------------------------------------------------------------------------------------------------- radius graph
def test_no_ambiguous_pair_in_a_radius_case(radius_cases):
    for name, case in list(radius_cases.items()) + [("coincident", gi.coincident_case())]:
        r2 = case["r"] ** 2
        assert case["pos"].dtype == torch.float32 and case["pos"].shape[0] == sum(case["sizes"]) == case["batch"].numel()
        for pos in _per_molecule(case):
            d2 = gi.pair_d2(pos)
            off = ~torch.eye(d2.shape[0], dtype=torch.bool)
            clear = ((d2 - r2).abs() > gi.MARGIN * r2) | (d2 == r2)
            assert bool((clear | ~off).all()), name


def test_radius_oracle_agrees_with_itself_in_float32(radius_cases):
    for name, case in list(radius_cases.items()) + [("coincident", gi.coincident_case())]:
        for cap in (1000, 3):
            s64, d64 = gi.radius_reference(case, cap, torch.float64)
            s32, d32 = gi.radius_reference(case, cap, torch.float32)
            assert torch.equal(s64, s32) and torch.equal(d64, d32), (name, cap)


def test_lattice_known_answer(radius_cases):
    case = radius_cases["lattice"]
    d2 = gi.pair_d2(case["pos"])
    off = ~torch.eye(6, dtype=torch.bool)
    assert int(((d2 == 25.0) & off).sum()) == 8           # ordered pairs exactly on the cut-off ...
    assert int(((d2 < 25.0) & off).sum()) == 8            # ... and strictly inside it
    src, dst = gi.radius_reference(case)
    assert src.numel() == 8                                 # the strict < of torch_cluster excludes the eight on the bound
    assert sorted(zip(dst.tolist(), src.tolist())) == [(0, 3), (1, 3), (1, 4), (2, 4), (3, 0), (3, 1), (4, 1), (4, 2)]


def test_ragged_batch_shapes(radius_cases):
    assert radius_cases["ragged"]["sizes"] == [1, 2, 63, 64, 65, 0, 129, 3, 0] and radius_cases["ragged"]["num_graphs"] == 9
    assert radius_cases["n1024"]["pos"].shape[0] == 1024 and radius_cases["n1040"]["pos"].shape[0] > 1024
    # the truncation sweep has something to truncate, and no molecule is so dense that nothing is left to tell apart
    src, dst = gi.radius_reference(radius_cases["trunc"])
    deg = torch.bincount(dst, minlength=39)
    assert int(deg.max()) >= 4 and int(deg.min()) == 0 and deg.unique().numel() > 3
    for name in ("ragged", "n1024", "n1040"):
        s, _ = gi.radius_reference(radius_cases[name])
        assert s.numel() > 2 * radius_cases[name]["pos"].shape[0], name


def test_coincident_atoms_have_an_edge_of_length_zero():
    case = gi.coincident_case()
    src, dst = gi.radius_reference(case)
    assert sorted(zip(dst.tolist(), src.tolist())) == [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
    p = case["pos"].double()
    vec = p[src] - p[dst]
    zero = vec.norm(dim=1) == 0
    assert int(zero.sum()) == 2
    sh = oe3.spherical_harmonics(3, vec)
    want = torch.zeros(16, dtype=torch.float64)
    want[0] = 1.0
    assert torch.equal(sh[zero], want.expand(2, 16)) and bool(torch.isfinite(sh).all())


# ------------------------------------------------------------------------------------------------- periodic graph
def test_no_ambiguous_pair_in_a_periodic_case(pbc_cases):
    for name, case in pbc_cases.items():
        r2 = case["r"] ** 2
        for pos, cell in gi.pbc_structures(case):
            d2, _, _ = gi.pbc_candidates(pos, cell, case["r"])
            assert bool((((d2 - r2).abs() > gi.MARGIN * r2) | (d2 == r2)).all()), name
            assert bool(((d2 - gi.LOW).abs() > gi.MARGIN * gi.LOW).all()), name
            assert gi.pbc_ambiguous_pairs(pos, cell, case["r"]) == 0, name


def test_no_ambiguous_cut_in_a_periodic_case(pbc_cases):
    truncated = {}
    for name, case in pbc_cases.items():
        for cap in case["caps"]:
            for pos, cell in gi.pbc_structures(case):
                assert gi.pbc_ambiguous_cuts(pos, cell, case["r"], cap, exact=case["exact"]) == 0, (name, cap)
                truncated[(name, cap)] = truncated.get((name, cap), 0) + gi.truncated_rows(pos, cell, case["r"], cap)
    # the sweep really truncates: every random case at 1, the dense cells and the 65-atom slab at 9 as well
    assert truncated[("close_pairs", 1)] > 0
    for name in ("cells", "sizes"):
        assert truncated[(name, 1)] > 0 and truncated[(name, 9)] > 0, name
    assert truncated[("cubic_a3", 4)] == 1
    # without the exemption the a = 3 cell IS a tie at the cut (the six images at d = 3)
    pos, cell = gi.pbc_structures(pbc_cases["cubic_a3"])[0]
    assert gi.pbc_ambiguous_cuts(pos, cell, 5.0, 4, exact=False) == 1


def test_periodic_oracle_agrees_with_itself_in_float32(pbc_cases):
    for name, case in pbc_cases.items():
        for cap in case["caps"]:
            a = gi.pbc_reference(case, cap, torch.float64)
            b = gi.pbc_reference(case, cap, torch.float32)
            assert all(torch.equal(x, y) for x, y in zip(a, b)), (name, cap)


def test_single_atom_known_answers(pbc_cases):
    a3, a25 = pbc_cases["cubic_a3"], pbc_cases["cubic_a2.5"]
    assert pbc.cell_repeats(a3["cell"][0], 5.0) == [2, 2, 2]
    ei, off, nb = gi.pbc_reference(a3, 1000)
    assert ei.shape[1] == 18 and nb.tolist() == [18]
    ei, off, nb = gi.pbc_reference(a3, 4)
    assert off.tolist() == [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, 1]]     # a six-way exact tie, cut in candidate order
    # r |a x a| / vol = 5 * 6.25 / 15.625 = 2 exactly: ceil(2 - 1e-12) keeps the repeats at 2
    assert pbc.cell_repeats(a25["cell"][0], 5.0) == [2, 2, 2]
    ei, off, nb = gi.pbc_reference(a25, 1000)
    assert ei.shape[1] == 32
    d2 = (off.double() * 2.5).pow(2).sum(1)
    assert int((d2 == 25.0).sum()) == 6                                          # at d = r exactly, kept by the periodic <=


def test_close_pairs_and_cells(pbc_cases):
    ei, off, nb = gi.pbc_reference(pbc_cases["close_pairs"], 1000)
    pairs = set(zip(ei[1].tolist(), ei[0].tolist(), map(tuple, off.tolist())))
    assert (0, 1, (0, 0, 0)) not in pairs and (1, 0, (0, 0, 0)) not in pairs    # 0.005 apart: d^2 = 2.5e-5 < 1e-4
    assert (2, 3, (0, 0, 0)) in pairs and (3, 2, (0, 0, 0)) in pairs            # 0.02 apart: d^2 = 4e-4
    cells = pbc_cases["cells"]["cell"]
    assert float(torch.linalg.det(cells[0].double())) < 0                       # left-handed
    assert pbc.cell_repeats(cells[1], 5.0) == [3, 2, 1]                         # three different repeat counts
    assert cells[2].diagonal().tolist() == [11.0, 11.0, 25.0]                   # the slab
    assert pbc_cases["sizes"]["natoms"] == [1, 2, 65]
    assert max(max(c["natoms"]) for c in pbc_cases.values()) <= 70
    # rows that hold one source several times (what eqf_csr_by_source_multi is for)
    for name in ("cubic_a3", "cells", "sizes"):
        ei, _, _ = gi.pbc_reference(pbc_cases[name], 50)
        key = ei[0] * 100000 + ei[1]
        assert int(torch.unique(key, return_counts=True)[1].max()) > 1, name


# ------------------------------------------------------------------------------------------------- edge geometry
@pytest.mark.parametrize("with_offsets", [False, True])
@pytest.mark.parametrize("E", [1, 255, 256, 257])
def test_geometry_graph(E, with_offsets):
    case = gi.geometry_case(E, with_offsets, seed=E)
    src, dst, N = case["src"], case["dst"], case["N"]
    assert src.numel() == E and case["pos"].shape == (N, 3)
    indeg, outdeg = torch.bincount(dst, minlength=N), torch.bincount(src, minlength=N)
    for n in case["isolated"]:
        assert indeg[n] == 0 and outdeg[n] == 0
    assert len(case["isolated"]) == gi.GEOM_ISOLATED
    for n in case["only_out"]:
        assert indeg[n] == 0 and outdeg[n] == 1
    for n in case["only_in"]:
        assert indeg[n] == 1 and outdeg[n] == 0
    v = gi.geometry_vectors(case)
    L = v.norm(dim=1)
    assert float(L.min()) > 0
    # float32 forms the same vectors exactly
    p32 = case["pos"]
    v32 = p32[src] - p32[dst] if case["offsets"] is None else p32[src] - p32[dst] + case["offsets"]
    assert torch.equal(v32.double(), v)
    if E >= 17:
        u = v[:17] / L[:17, None]
        assert abs(float(L[:17].min()) - 1e-3) < 1e-9 and abs(float(L[:17].max()) - 20.0) < 1e-5
        assert int(((u.abs() == 1).sum(1) == 1).sum()) == 6                       # the six axes, exactly
        assert int((((u == 0).sum(1) == 1)).sum()) >= 6                           # in a coordinate plane, exactly
        polar = (u[:, 1].abs() < 1) & ((1 - u[:, 1].abs()) < 1e-8)
        assert int(polar.sum()) == 5                                              # within 1e-4 of +-y, not on it


def test_radial_oracles_vanish_from_the_cut_off_on():
    """the reference itself returns exact zeros at and beyond the cut-off, in float64 and in float32"""
    for dt in (torch.float64, torch.float32):
        d = torch.tensor([5.0, 5.0 * (1 + 1e-3)], dtype=torch.float32).to(dt)
        assert bool((onets.ExpNormalSmearing(0.0, 5.0, 50).to(dt)(d) == 0).all())
        assert bool((onets.RadialBasis(8, 5.0).to(dt)(d[:1]) == 0).all())
