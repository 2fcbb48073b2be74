"""Graph construction, edge geometry and the radial bases (csrc/graph.hip, csrc/geom.h) against the float64 oracle at their
edges.  Inputs: tests/graph_edge_inputs.py (tests/test_graph_edge_inputs.py proves on the CPU that no case depends on how
float32 rounds a distance).  References: oracle.nets.radius_graph, oracle.pbc.radius_graph_pbc, oracle.e3.spherical_harmonics,
oracle.nets.GaussianRadialBasisLayer / ExpNormalSmearing / RadialBasis, all in float64 on the CPU on float32-rounded inputs.

Index tensors (src, dst, row_ptr, mol_ptr, src_ptr, src_perm, cell_offsets) are compared for EQUALITY.  Floating results use
`fp64_ops.per_row_rel` (harmonics: one slice per degree; parameter gradients: one element per row) with the figures of
tests/test_gpu_ops.py::test_edge_geometry_and_rbf applied per row: sh 2e-6, length 1e-6, bases 1e-5, gradients 5e-5.  Where
plain fp32 cannot meet that (Bessel arguments of hundreds of radians, Gaussians far out in a tail, gradients that cancel in a
node's row) the bound is max(project bound, 4 x the SAME oracle call evaluated in float32 on the CPU on the same inputs): the
rule and the factor of tests/test_gpu_op_edges.py.  Every test prints "FIG <case> <quantity> err=... yard=... bound=..." lines;
profiles/graph_edges/figures.txt holds those of one MI355X run.

Measured on an MI355X, the worst case of each quantity (largest err / bound) in that run:
  radius / periodic graph   every index tensor equal in all cases; offsets 3.5e-8, yard 3.5e-8 (1e-6; cells, max_nbr = 50)
  edge geometry             length 5.9e-8 (1e-6), sh 4.2e-7, yard 2.2e-7 (2e-6; lmax = 3, E = 256), d_pos 9.6e-7, yard 2.4e-7
                            (5e-5), the same through the null-pointer entry; vec_sh 4.9e-7, yard 3.3e-7 (2e-6)
  Gaussian                  out 3.3e-7 (1e-5); d_len 3.8e-5, yard 4.5e-5 -> 1.8e-4 (R = 65, E = 257); d_std 2.2e-4, yard 2.2e-4
                            -> 9.0e-4 (R = 63, E = 64); d_mean 8.3e-6, d_weight 4.7e-6, d_bias 2.1e-6 (5e-5)
  ExpNorm                   out 4.0e-6, yard 3.9e-6 -> 1.6e-5; d_len 5.5e-5, yard 4.2e-5 -> 1.7e-4 (R = 65)
  Bessel                    out 6.1e-6, yard 5.7e-6 -> 2.3e-5 (R = 65, E = 5); d_len 3.9e-5, yard 3.8e-5 -> 1.5e-4;
                            d_freq 2.2e-4, yard 1.6e-4 -> 6.3e-4 (R = 128, E = 257)
  negative controls         lattice with <=: src, dst, row_ptr, src_ptr, src_perm and the counts differ; a = 2.5 with <: those
                            and cell_offsets; exchanged degree-3 components 2.0 against 3.1e-7; d_std without the sign 2.0
                            against 1.0e-6
Two defects this file found are fixed in csrc/graph.hip.  The Gaussian kernels formed x = weight * len * (1 / cutoff) + bias
in float: (x - mean) / std at std = 0.05 turned its one to two ulps into d_len 1.2e-4 (R = 63, E = 257) and 3.2e-4 (R = 65,
E = 63) against bounds of 1.0e-4 and 2.0e-4 -- x - mean is formed in double now.  The Bessel envelope in its expanded form
cancelled towards x = 1: out 2.3e-5 against 1.1e-5 at x = 0.91 (R = 8, E = 4) -- it is evaluated in factored form.
Wall time of this file on an MI355X, one run each (pytest's figure): 3.7 s at the parent commit, 4.1 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_ops as fo  # noqa: E402
import graph_edge_inputs as gi  # noqa: E402
from oracle import e3 as oe3  # noqa: E402
from oracle import nets as onets  # noqa: E402
from poison import guard_input, poisoned_ops  # noqa: E402,F401  (every launch of this file runs on poisoned, guarded allocations)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_ops")]

B_SH, B_LEN, B_BASIS, B_GRAD = 2e-6, 1e-6, 1e-5, 5e-5


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _randn(shape, seed, scale=1.0):
    return fo.f32r(torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale)


def _rand(shape, seed, lo=0.0, hi=1.0):
    return fo.f32r(torch.rand(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * (hi - lo) + lo)


class _Checker:
    """collects every comparison of a test, prints its figures and fails at the end, so that one run shows them all;
    bound of a comparison: max(project bound, 4 x yardstick), the yardstick being the float32 CPU evaluation of the reference"""

    def __init__(self, case):
        self.case, self.bad, self.worst = case, [], {}

    def cmp(self, name, got, ref, bound, y32=None, slices=None, tag=""):
        assert got is not None and torch.isfinite(got).all(), (self.case, name, tag, "not finite")
        err = fo.per_row_rel(got, ref, slices=slices)
        yard = fo.per_row_rel(y32, ref, slices=slices) if y32 is not None else None
        lim = bound if yard is None else max(bound, 4.0 * yard)
        w = self.worst.get(name)
        if w is None or err / lim > w[0] / w[2]:
            self.worst[name] = (err, yard, lim)
        if not err < lim:
            self.bad.append((name + tag, err, yard, lim))
        return err, lim

    def done(self):
        for name, (err, yard, lim) in self.worst.items():
            print("FIG %s %s err=%.2e yard=%s bound=%.2e" % (self.case, name, err, "-" if yard is None else "%.2e" % yard, lim))
        assert not self.bad, (self.case, self.bad)


def _evaluate(fn, inputs, gouts, dtype, device="cpu", wrt=()):
    """(outputs, gradients wrt inputs[wrt]) of fn in `dtype` on `device`; ONLY the inputs listed in wrt require a gradient"""
    ins = []
    for i, t in enumerate(inputs):
        if torch.is_tensor(t) and t.is_floating_point():
            ins.append(t.detach().to(dtype).to(device).requires_grad_(i in wrt))
        else:
            ins.append(t.to(device) if torch.is_tensor(t) else t)
    outs = fn(*ins)
    outs = list(outs) if isinstance(outs, (tuple, list)) else [outs]
    grads = []
    if wrt:
        # (an output that does not depend on the inputs -- the constant degree-0 harmonic of the reference -- has no graph)
        pairs = [(o, g.to(dtype).to(device)) for o, g in zip(outs, gouts) if o.requires_grad]
        grads = list(torch.autograd.grad([o for o, _ in pairs], [ins[i] for i in wrt], [g for _, g in pairs], allow_unused=True))
    return [o.detach() for o in outs], grads


def _degree_slices(lmax):
    return [slice(l * l, (l + 1) * (l + 1)) for l in range(lmax + 1)]


@pytest.fixture(scope="module")
def radius_cases():
    return gi.radius_cases()


@pytest.fixture(scope="module")
def pbc_cases():
    return gi.pbc_cases()


# ------------------------------------------------------------------------------------------------- radius graph
def _ptr(counts):
    return torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)])


def _graph_mismatches(g, src, dst, N, sizes):
    """names of the index tensors of graph `g` that differ from what the (src, dst) edge list implies"""
    want = {"src": src, "dst": dst, "row_ptr": _ptr(torch.bincount(dst, minlength=N)),
            "mol_ptr": _ptr(torch.tensor(sizes, dtype=torch.long)), "src_ptr": _ptr(torch.bincount(src, minlength=N)),
            "src_perm": torch.argsort(src, stable=True)}
    bad = []
    for name, w in want.items():
        got = getattr(g, name).cpu().long()
        if got.shape != w.shape or not torch.equal(got, w):
            bad.append(name)
    if g.E != src.numel() or g.N != N:
        bad.append("counts")
    return bad


def _radius(case, cap=1000):
    from equiformer_amd.graph import EdgeGraph
    dev = _dev()
    return EdgeGraph.from_radius(case["pos"].to(dev), case["batch"].to(dev), case["r"], max_num_neighbors=cap,
                                 num_graphs=case["num_graphs"])


@pytest.mark.parametrize("name", ["lattice", "ragged", "n1024", "n1040"])
def test_radius_graph_edges(radius_cases, name):
    """pairs exactly on the cut-off (strict <), molecule sizes around the 64-thread stride with empty ids in the middle and
    at the end, the scan at exactly 1024 nodes and beyond (chunks of 2)"""
    case = radius_cases[name]
    src, dst = gi.radius_reference(case)
    g = _radius(case)
    assert g.E > 0 and _graph_mismatches(g, src, dst, case["pos"].shape[0], case["sizes"]) == []
    assert g.num_graphs == case["num_graphs"] and torch.equal(g.batch.cpu().long(), case["batch"])


def test_radius_graph_truncated(radius_cases):
    """max_num_neighbors around the largest degree of the batch: the truncated graph is asymmetric and its by-source view is
    still the stable sort"""
    case = radius_cases["trunc"]
    N = case["pos"].shape[0]
    s, d = gi.radius_reference(case)
    dmax = int(torch.bincount(d, minlength=N).max())
    counts = {}
    for cap in sorted({1, 2, dmax - 1, dmax, dmax + 1}):
        src, dst = gi.radius_reference(case, cap)
        counts[cap] = src.numel()
        g = _radius(case, cap)
        assert _graph_mismatches(g, src, dst, N, case["sizes"]) == [], cap
    assert counts[1] < counts[2] < counts[dmax - 1] < counts[dmax] == counts[dmax + 1] == s.numel()
    src, dst = gi.radius_reference(case, 2)
    fwd = set(zip(src.tolist(), dst.tolist()))
    assert any((b, a) not in fwd for a, b in fwd)  # asymmetric


def test_coincident_atoms():
    """two atoms at one point: the edge exists, its length is 0, its harmonics are [1, 0, ...], everything is finite"""
    from equiformer_amd import ops
    case = gi.coincident_case()
    src, dst = gi.radius_reference(case)
    g = _radius(case)
    assert _graph_mismatches(g, src, dst, 3, [3]) == []
    _, length, sh = ops.edge_geometry(case["pos"].to(_dev()), None, g, 3)
    p = case["pos"].double()
    vec = p[src] - p[dst]
    zero = vec.norm(dim=1) == 0
    assert int(zero.sum()) == 2
    assert bool(torch.isfinite(length).all()) and bool(torch.isfinite(sh).all())
    assert bool((length.cpu()[zero] == 0).all())
    want = torch.zeros(16)
    want[0] = 1.0
    assert torch.equal(sh.cpu()[zero], want.expand(2, 16))
    ck = _Checker("coincident")
    ck.cmp("length", length, vec.norm(dim=1), B_LEN)
    ck.cmp("sh", sh, oe3.spherical_harmonics(3, vec), B_SH, slices=_degree_slices(3))
    ck.done()


def test_lattice_edges_built_with_le_are_seen(radius_cases):
    """negative control: an expectation that keeps the pairs ON the cut-off fails the comparison of test_radius_graph_edges"""
    case = radius_cases["lattice"]
    g = _radius(case)
    d2 = gi.pair_d2(case["pos"])
    adj = (d2 <= 25.0) & ~torch.eye(6, dtype=torch.bool)
    dst_w, src_w = adj.nonzero(as_tuple=True)
    assert src_w.numel() == 16
    src, dst = gi.radius_reference(case)
    assert _graph_mismatches(g, src, dst, 6, [6]) == []
    bad = _graph_mismatches(g, src_w, dst_w, 6, [6])
    print("lattice with <=: mismatching", bad)
    assert "src" in bad and "dst" in bad and "row_ptr" in bad and "counts" in bad


# ------------------------------------------------------------------------------------------------- periodic graph
def _pbc_graph(case, cap):
    from equiformer_amd.graph import EdgeGraph
    dev = _dev()
    return EdgeGraph.from_radius_pbc(case["pos"].to(dev), case["cell"].to(dev), case["batch"].to(dev), case["r"],
                                     max_num_neighbors=cap)


def _pbc_mismatches(g, cell_off, ei, off, N, natoms):
    bad = _graph_mismatches(g, ei[0], ei[1], N, natoms)
    got = cell_off.cpu().long()
    if got.shape != off.shape or not torch.equal(got, off):
        bad.append("cell_offsets")
    return bad


def _pbc_check(case, cap, name):
    ei, off, nb = gi.pbc_reference(case, cap)
    g, offsets, cell_off = _pbc_graph(case, cap)
    N = case["pos"].shape[0]
    assert _pbc_mismatches(g, cell_off, ei, off, N, case["natoms"]) == [], (name, cap)
    assert g.E > 0
    # offsets = cell_offsets . cell (Cartesian), the cell of the edge's structure
    cpe = torch.repeat_interleave(case["cell"].double(), nb, dim=0)
    cart = torch.bmm(off.double().view(-1, 1, 3), cpe).view(-1, 3)
    cart32 = torch.bmm(off.float().view(-1, 1, 3), cpe.float()).view(-1, 3)
    ck = _Checker("pbc[%s,max_nbr=%d]" % (name, cap))
    ck.cmp("offsets", offsets, cart, B_LEN, cart32)
    ck.done()
    return g, ei, off


@pytest.mark.parametrize("name", ["cubic_a3", "cubic_a2.5", "close_pairs", "cells", "sizes"])
def test_periodic_graph_edges(pbc_cases, name):
    """single-atom known answers (pairs AT the cut-off are kept by the periodic <=; a six-way tie cut in candidate order), the
    lower bound d^2 > 1e-4, a left-handed, a skewed and a slab cell, structures of 1, 2 and 65 atoms, max_nbr 1 / 9 / 50; the
    by-source view of eqf_csr_by_source_multi on rows that hold one source several times"""
    case = pbc_cases[name]
    for cap in case["caps"]:
        g, ei, off = _pbc_check(case, cap, name)
        if name == "cubic_a3":
            assert g.E == (18 if cap == 1000 else 4)
            if cap == 4:
                assert off.tolist() == [[-1, 0, 0], [0, -1, 0], [0, 0, -1], [0, 0, 1]]
        if name == "cubic_a2.5":
            assert g.E == 32
    if name in ("cubic_a3", "cells", "sizes"):  # (checked above against the stable sort) a row holds a source several times
        ei, _, _ = gi.pbc_reference(case, case["caps"][-1] if name != "cubic_a3" else 1000)
        assert int(torch.unique(ei[0] * 100000 + ei[1], return_counts=True)[1].max()) > 1


def test_periodic_lt_is_seen(pbc_cases):
    """negative control: the a = 2.5 cell with a strict < at the cut-off (26 edges) fails the comparison"""
    case = pbc_cases["cubic_a2.5"]
    ei, off, nb = gi.pbc_reference(case, 1000)
    g, offsets, cell_off = _pbc_graph(case, 1000)
    assert _pbc_mismatches(g, cell_off, ei, off, 1, [1]) == []
    inside = (off.double() * 2.5).pow(2).sum(1) < 25.0
    assert int(inside.sum()) == 26
    bad = _pbc_mismatches(g, cell_off, ei[:, inside], off[inside], 1, [1])
    print("a = 2.5 with <: mismatching", bad)
    assert "src" in bad and "row_ptr" in bad and "cell_offsets" in bad and "counts" in bad


# ------------------------------------------------------------------------------------------------- edge geometry
def _geometry(E, with_offsets, lmax):
    from equiformer_amd.graph import EdgeGraph
    case = gi.geometry_case(E, with_offsets, seed=E)
    dev = _dev()
    graph, order = EdgeGraph.from_edges(case["src"].to(dev), case["dst"].to(dev), case["N"])
    order = order.cpu()
    src, dst = case["src"][order], case["dst"][order]
    assert torch.equal(graph.src.cpu().long(), src) and torch.equal(graph.dst.cpu().long(), dst)
    offsets = fo.f32r(case["offsets"][order]) if with_offsets else None

    def ref(pos):
        vec = pos[src] - pos[dst]
        if offsets is not None:
            vec = vec + offsets.to(pos.dtype)
        return vec.norm(dim=1), oe3.spherical_harmonics(lmax, vec)

    return case, graph, offsets, ref


@pytest.mark.parametrize("with_offsets", [False, True], ids=["plain", "offsets"])
@pytest.mark.parametrize("E", [1, 255, 256, 257])
@pytest.mark.parametrize("lmax", [0, 1, 2, 3])
def test_edge_geometry_edges(lmax, E, with_offsets):
    """length, sh per degree, and d_pos for cotangents on sh only, on length only, on both, and on one degree of sh at a time
    -- through autograd (ops.edge_geometry) and through the backward entry with the absent cotangent passed as a null pointer
    (the d_sh == nullptr / d_len == nullptr branches of geom_grad).  Directions: the six axes, the coordinate planes, within
    1e-4 of the polar axis, random; lengths 1e-3 .. 20; nodes without edges, with only incoming, with only outgoing edges."""
    from equiformer_amd import ops
    case, graph, offsets, ref = _geometry(E, with_offsets, lmax)
    dev = _dev()
    N, S = case["N"], (lmax + 1) ** 2
    pos = fo.f32r(case["pos"])
    off_dev = offsets.float().to(dev) if offsets is not None else None
    sl = _degree_slices(lmax)
    ck = _Checker("geom[lmax=%d,E=%d,%s]" % (lmax, E, "offsets" if with_offsets else "plain"))

    def hip(p):
        _, length, sh = ops.edge_geometry(p, off_dev, graph, lmax)
        return length, sh

    go_len, go_sh = _randn((E,), 70 + E), _randn((E, S), 71 + E)
    cots = [("both", go_len, go_sh), ("len", go_len, None), ("sh", None, go_sh)]
    for l in range(lmax + 1):
        one = torch.zeros_like(go_sh)
        one[:, sl[l]] = go_sh[:, sl[l]]
        cots.append(("sh%d" % l, None, one))
    zero_len, zero_sh = torch.zeros_like(go_len), torch.zeros_like(go_sh)
    vec_dev = None
    for tag, gl, gs in cots:
        gouts = [gl if gl is not None else zero_len, gs if gs is not None else zero_sh]
        (len_r, sh_r), (dp_r,) = _evaluate(ref, [pos], gouts, torch.float64, wrt=(0,))
        (len_y, sh_y), (dp_y,) = _evaluate(ref, [pos], gouts, torch.float32, wrt=(0,))
        (len_h, sh_h), (dp_h,) = _evaluate(hip, [pos], gouts, torch.float32, device=dev, wrt=(0,))
        if tag == "both":
            ck.cmp("length", len_h, len_r, B_LEN, len_y)
            ck.cmp("sh", sh_h, sh_r, B_SH, sh_y, slices=sl)
            vec_dev = ops.edge_geometry(pos.float().to(dev), off_dev, graph, lmax)[0]
        ck.cmp("d_pos", dp_h, dp_r, B_GRAD, dp_y, tag=":" + tag)
        # the same cotangents through the backward entry, the absent one as a null pointer
        dp_n = ops._edge_geom_dpos(vec_dev, gs.float().to(dev) if gs is not None else None,
                                   gl.float().to(dev) if gl is not None else None, graph, lmax, N)
        ck.cmp("d_pos[null]", dp_n, dp_r, B_GRAD, dp_y, tag=":" + tag)
        for dp in (dp_h, dp_n):
            assert bool((dp.cpu()[case["isolated"]] == 0).all()), "an isolated node's d_pos is exactly zero"
    ck.done()


@pytest.mark.parametrize("keep_kind", ["none", "mixed"])
@pytest.mark.parametrize("N", [1, 257])
def test_vec_sh_edges(N, keep_kind):
    """ops.vec_sh against sh * |v| * scale for lmax 0..3; rows with keep == False are exactly zero"""
    from equiformer_amd import ops
    dev = _dev()
    case = gi.geometry_case(N, True, seed=N + 3)
    vec = gi.geometry_vectors(case)
    keep = None
    if keep_kind == "mixed":
        keep = (torch.arange(N) % 3 != 1) if N > 1 else torch.zeros(1, dtype=torch.bool)
    scale = 0.37
    ck = _Checker("vec_sh[N=%d,keep=%s]" % (N, keep_kind))
    for lmax in range(4):
        def ref(v):
            out = oe3.spherical_harmonics(lmax, v) * v.norm(dim=1, keepdim=True) * scale
            return out if keep is None else out * keep.to(v.dtype)[:, None]
        got = ops.vec_sh(vec.float().to(dev), keep.to(dev) if keep is not None else None, lmax, scale)
        ck.cmp("out[lmax=%d]" % lmax, got, ref(vec), B_SH, ref(vec.float()), slices=_degree_slices(lmax))
        if keep is not None:
            assert bool((got.cpu()[~keep] == 0).all())
    ck.done()


def test_lmax_4_is_refused():
    """every geometry entry point returns before any launch"""
    from equiformer_amd import ops
    from equiformer_amd.graph import EdgeGraph
    from equiformer_amd.lib import HipLibraryError
    dev = _dev()
    case = gi.geometry_case(5, False, seed=1)
    graph, _ = EdgeGraph.from_edges(case["src"].to(dev), case["dst"].to(dev), case["N"])
    pos = case["pos"].to(dev)
    with pytest.raises(HipLibraryError):
        ops.edge_geometry(pos, None, graph, 4)
    with pytest.raises(HipLibraryError):
        ops.vec_sh(pos, None, 4, 1.0)
    vec = ops.edge_geometry(pos, None, graph, 3)[0]
    with pytest.raises(HipLibraryError):
        ops._edge_geom_dpos(vec, torch.zeros(5, 25, device=dev), None, graph, 4, case["N"])


def test_exchanged_degree_3_components_are_seen():
    """negative control: harmonics with two degree-3 components exchanged fail the per-degree comparison"""
    from equiformer_amd import ops
    case, graph, offsets, ref = _geometry(257, False, 3)
    sh = ops.edge_geometry(case["pos"].to(_dev()), None, graph, 3)[2]
    sh_r = ref(fo.f32r(case["pos"]))[1]
    wrong = sh_r.clone()
    wrong[:, 10], wrong[:, 14] = sh_r[:, 14], sh_r[:, 10]
    sl = _degree_slices(3)
    bound = max(B_SH, 4.0 * fo.per_row_rel(ref(case["pos"].float())[1], sh_r, slices=sl))
    right_e = fo.per_row_rel(sh, sh_r, slices=sl)
    wrong_e = fo.per_row_rel(sh, wrong, slices=sl)
    print("exchanged degree-3 components: right %.2e wrong %.2e bound %.2e" % (right_e, wrong_e, bound))
    assert right_e < bound and wrong_e > 100 * bound
    # the degrees below 3 do not see it: it is the degree-3 slice that fails
    assert fo.per_row_rel(sh[:, :9], wrong[:, :9], slices=sl[:3]) < bound


# ------------------------------------------------------------------------------------------------- radial bases
E_VALUES = [1, 3, 4, 5, 63, 64, 65, 257]
RC = 5.0


def _lengths(E, seed, specials, lo, hi):
    """`specials` first (as many as fit), then float32 lengths spread over [lo, hi]: a jittered grid, so that every stretch
    of the range is hit at every E"""
    sp = list(specials)[:E]
    n = E - len(sp)
    g = torch.Generator().manual_seed(seed)
    grid = (torch.arange(n, dtype=torch.float64) + torch.rand(n, generator=g, dtype=torch.float64)) / max(n, 1)
    grid = grid[torch.randperm(n, generator=g)]
    return fo.f32r(torch.cat([torch.tensor(sp, dtype=torch.float64), lo + (hi - lo) * grid]))


def _basis_run(ck, names, hip, ref, inputs, gouts, bounds, wrt):
    ro, rg = _evaluate(ref, inputs, gouts, torch.float64, wrt=wrt)
    yo, yg = _evaluate(ref, inputs, gouts, torch.float32, wrt=wrt)
    ho, hg = _evaluate(hip, inputs, gouts, torch.float32, device=_dev(), wrt=wrt)
    for name, h, r, y in zip(names, ho + hg, ro + rg, yo + yg):
        ck.cmp(name, h, r, bounds[name], y)
    return ho, hg, ro, rg


GAUSS_BOUNDS = {"out": B_BASIS, "d_len": B_GRAD, "d_mean": B_GRAD, "d_std": B_GRAD, "d_weight": B_GRAD, "d_bias": B_GRAD}


def _gauss_inputs(E, R):
    """lengths over [0.02, 1.15] rc (E = 1: the middle), mean in [0, 1], std in +-[0.05, 3] with alternating signs,
    weight 1.3, bias -0.2"""
    length = _lengths(E, 300 + E + R, [0.45 * RC] if E == 1 else [], 0.02 * RC, 1.15 * RC)
    mean = _rand((R,), 301 + R)
    std = _rand((R,), 302 + R, 0.05, 3.0)
    std[(torch.arange(R) % 2) == (1 if R > 1 else 0)] *= -1.0
    one = lambda v: torch.tensor([v], dtype=torch.float32).double()  # noqa: E731
    return [length, mean, std, one(1.3), one(-0.2)]


def _gauss_fns(R):
    from equiformer_amd import ops
    mod = onets.GaussianRadialBasisLayer(R, RC)

    def ref(length, mean, std, weight, bias):
        return torch.func.functional_call(mod, {"mean": mean.view(1, R), "std": std.view(1, R), "weight": weight.view(1, 1),
                                                "bias": bias.view(1, 1)}, (length,))

    def hip(length, mean, std, weight, bias):
        return ops.rbf_gaussian(length, mean, std, weight, bias, RC)

    return hip, ref


@pytest.mark.parametrize("E", E_VALUES)
@pytest.mark.parametrize("R", [1, 63, 64, 65, 128, 256])
def test_gaussian_basis_edges(R, E):
    """out, d_len and the four parameter gradients; the backward runs one thread per basis function with the block rounded up
    to 64 (R = 1, 63, 65 leave idle lanes, 256 fills four waves), 64 edges per block (E = 63, 64, 65, 257); std of both signs"""
    hip, ref = _gauss_fns(R)
    inputs = _gauss_inputs(E, R)
    if R > 1:
        assert bool((inputs[2] > 0).any()) and bool((inputs[2] < 0).any())
    ck = _Checker("gauss[R=%d,E=%d]" % (R, E))
    _basis_run(ck, ["out", "d_len", "d_mean", "d_std", "d_weight", "d_bias"], hip, ref, inputs, [_randn((E, R), 310 + E + R)],
               GAUSS_BOUNDS, (0, 1, 2, 3, 4))
    ck.done()


def test_gaussian_backward_refuses_257():
    """R = 257 is refused before any launch: the outputs keep what they held"""
    from equiformer_amd import ops
    from equiformer_amd.lib import HipLibraryError, call
    dev = _dev()
    E, R = 5, 257
    f = lambda *s: guard_input(torch.full(s, 7.0, device=dev))  # noqa: E731  (nothing around them is written either)
    length, dout, mean, std = f(E), f(E, R), f(R), f(R)
    w, b = f(1), f(1)
    outs = [f(R), f(R), f(1), f(1), f(E)]
    with pytest.raises(HipLibraryError):
        call("eqf_rbf_gaussian_bwd", ops._p(length), ops._p(dout), E, R, ops._p(mean), ops._p(std), ops._p(w), ops._p(b), RC,
             *[ops._p(t) for t in outs], ops._stream())
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs)


def test_gaussian_d_std_without_the_sign_is_seen():
    """negative control: d_std taken wrt |std| (the sign dropped) fails the comparison"""
    R, E = 64, 65
    hip, ref = _gauss_fns(R)
    inputs = _gauss_inputs(E, R)
    go = [_randn((E, R), 310 + E + R)]
    _, rg = _evaluate(ref, inputs, go, torch.float64, wrt=(2,))
    _, yg = _evaluate(ref, inputs, go, torch.float32, wrt=(2,))
    _, hg = _evaluate(hip, inputs, go, torch.float32, device=_dev(), wrt=(2,))
    wrong = rg[0] * torch.sign(inputs[2])
    bound = max(B_GRAD, 4.0 * fo.per_row_rel(yg[0], rg[0]))
    right_e, wrong_e = fo.per_row_rel(hg[0], rg[0]), fo.per_row_rel(hg[0], wrong)
    print("d_std without the sign: right %.2e wrong %.2e bound %.2e" % (right_e, wrong_e, bound))
    assert right_e < bound and wrong_e > 100 * bound


@pytest.mark.parametrize("E", E_VALUES)
@pytest.mark.parametrize("R", [1, 50, 64, 65])
def test_expnorm_basis_edges(R, E):
    """out and d_len; lengths include 1e-3, exactly rc and rc (1 + 1e-3): out and d_len are exactly 0 from rc on"""
    from equiformer_amd import ops
    mod = onets.ExpNormalSmearing(0.0, RC, R)
    alpha = mod.alpha
    length = _lengths(E, 400 + E + R, [1e-3, RC, RC * (1 + 1e-3)], 0.02 * RC, 0.97 * RC)
    means, betas = fo.f32r(mod.means), fo.f32r(mod.betas)

    def ref(d, mu, be):
        return torch.func.functional_call(mod, {"means": mu, "betas": be}, (d,))

    def hip(d, mu, be):
        return ops.rbf_expnorm(d, mu, be, alpha, RC)

    ck = _Checker("expnorm[R=%d,E=%d]" % (R, E))
    ho, hg, ro, rg = _basis_run(ck, ["out", "d_len"], hip, ref, [length, means, betas], [_randn((E, R), 410 + E + R)],
                                {"out": B_BASIS, "d_len": B_GRAD}, (0,))
    beyond = length >= RC
    assert int(beyond.sum()) == min(max(E - 1, 0), 2)
    assert bool((ro[0][beyond] == 0).all()) and bool((rg[0][beyond] == 0).all())
    assert bool((ho[0].cpu()[beyond] == 0).all()) and bool((hg[0].cpu()[beyond] == 0).all())
    ck.done()


def _bessel_fns(R):
    from equiformer_amd import ops
    mod = onets.RadialBasis(R, RC)

    def ref(d, freq):
        return torch.func.functional_call(mod, {"rbf.frequencies": freq}, (d,))

    def hip(d, freq):
        return ops.rbf_bessel(d, freq, RC)

    # trainable frequencies: k pi as initialised (float32), moved by about a percent
    freq = fo.f32r(mod.rbf.frequencies.detach().double() * (1.0 + 0.01 * _randn((R,), 500 + R)))
    return hip, ref, freq


@pytest.mark.parametrize("E", E_VALUES)
@pytest.mark.parametrize("R", [1, 8, 64, 65, 128])
def test_bessel_basis_edges(R, E):
    """out, d_len and d_freq (64 edges per block, 4 per wave: d_freq is accumulated over up to five blocks); lengths 0.05 ..
    rc and exactly rc, where everything is 0; then the d_freq-only path (length without gradient: d_len is a null pointer) and
    the d_len-only path (frequencies frozen: d_freq is a null pointer).  No length is 0: the kernels divide by x."""
    hip, ref, freq = _bessel_fns(R)
    length = _lengths(E, 510 + E + R, [RC] if E > 1 else [0.45 * RC], 0.05, 0.97 * RC)
    assert float(length.min()) >= 0.049
    go = [_randn((E, R), 520 + E + R)]
    ck = _Checker("bessel[R=%d,E=%d]" % (R, E))
    bounds = {"out": B_BASIS, "d_len": B_GRAD, "d_freq": B_GRAD}
    ho, hg, ro, rg = _basis_run(ck, ["out", "d_len", "d_freq"], hip, ref, [length, freq], go, bounds, (0, 1))
    at_rc = length == RC
    assert int(at_rc.sum()) == (1 if E > 1 else 0)
    assert bool((ro[0][at_rc] == 0).all()) and bool((rg[0][at_rc] == 0).all())
    assert bool((ho[0].cpu()[at_rc] == 0).all()) and bool((hg[0].cpu()[at_rc] == 0).all())
    # one gradient at a time: the other output pointer is null
    bounds1 = {"out": B_BASIS, "d_freq[only]": B_GRAD, "d_len[only]": B_GRAD}
    _basis_run(ck, ["out", "d_freq[only]"], hip, ref, [length, freq], go, bounds1, (1,))
    _basis_run(ck, ["out", "d_len[only]"], hip, ref, [length, freq], go, bounds1, (0,))
    ck.done()
