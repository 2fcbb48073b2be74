"""Destination-sorted edge lists (CSR) for the segmented HIP kernels.

The reference builds `edge_index` with torch_cluster.radius_graph (nets/graph_attention_transformer.py:866-867) and
scatters with atomics; here the graph is produced already grouped by destination node (the order torch_cluster
emits as well), together with the CSR offsets and the by-source permutation that turn every scatter / gather
backward into an atomics-free segmented reduction.

Three edge sources -- the neighbour search, the periodic neighbour search, a GIVEN periodic edge list -- go through one
pipeline: a plan (`radius_plan`, `radius_pbc_plan`, `edges_pbc_plan`: counts, scans, the one host read-back), then the graph of
the plan, exact-shape (`_build_exact`) or padded to a capacity (`_build_padded`).  A source contributes its fill kernel, the
per-edge tensors it owns and its by-source entry point (`_Source`); everything else is written once.
"""
import collections
import ctypes

import torch

from . import ops
from .lib import call


def _i32(t):
    return t.to(torch.int32).contiguous()


def _ptr_from_counts(counts):
    z = torch.zeros(1, dtype=torch.int64, device=counts.device)
    return _i32(torch.cat([z, torch.cumsum(counts.to(torch.int64), 0)]))


def _P(t, byte_offset=0):
    return ctypes.c_void_p(ops._nonnull(t) + byte_offset) if t is not None else None


def _stream():
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:
        return ctypes.c_void_p(raw(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


CSR_MAX_NODES = 16384  # nodes per molecule the by-source kernel keeps cursors for (csrc/graph.hip)
EDGES_PASS = 256       # input edges per pass of eqf_edges_pbc_fill (csrc/graph.hip): a row's edges may straddle a pass boundary


class GraphDoesNotFit(ValueError):
    """The real node / edge counts of a batch do not fit the capacity it was to be padded to."""


def min_phantom_nodes(q):
    """Smallest P with P (P - 1) >= q: the phantom nodes that q phantom edges need (distinct ordered pairs, no self-loop)."""
    q = int(q)
    if q <= 0:
        return 0
    p = int((1.0 + (1.0 + 4.0 * q) ** 0.5) / 2.0)
    while p * (p - 1) < q:
        p += 1
    while p > 1 and (p - 1) * (p - 2) >= q:
        p -= 1
    return p


class RadiusPlan:
    """The first half of a radius graph build: per-node degrees, their scan and the host read-back of the edge count.  A caller
    that picks the capacity FROM the counts (equiformer_amd/capture.py: the bucket of a batch) runs the two halves itself:
    `plan = EdgeGraph.radius_plan(...)`, then `EdgeGraph.from_radius_plan(plan, capacity, into)`."""
    __slots__ = ("pos", "b32", "N", "E", "num_graphs", "mol_ptr", "row_ptr", "max_mol_nodes", "r", "max_num_neighbors")


class PbcPlan:
    """The first half of a periodic graph build (`EdgeGraph.radius_pbc_plan`): RadiusPlan's fields plus the cells, the candidate
    scan of the nearest-k selection and the candidate total (the size of its scratch)."""
    __slots__ = ("pos", "cell", "b32", "N", "E", "C", "num_graphs", "mol_ptr", "row_ptr", "cand_ptr", "max_mol_nodes", "r",
                 "max_num_neighbors")


class EdgesPbcPlan:
    """The first half of a build from a GIVEN periodic edge list (`EdgeGraph.edges_pbc_plan`): the input as the loader delivers
    it, the scan of `neighbors`, the kept mask and fp32 Cartesian offset per input edge, the kept in-degrees' scan and the host
    read-back (E = kept edges, E_in = input edges)."""
    __slots__ = ("pos", "cell", "b32", "N", "E", "E_in", "num_graphs", "mol_ptr", "nbr_ptr", "row_ptr", "max_mol_nodes",
                 "edge_index", "cell_offsets", "index64", "offsets64", "keep", "off")


# What an edge source contributes to the second half of a build.  fill(plan, g): the plan's E real edges into the head of g's
# per-edge tensors; per_edge: (name, trailing shape, dtype, value of a phantom edge's row) of the per-edge tensors it owns beside
# src / dst; by_source: the entry point of its by-source view; pbc / given: the flags its graphs carry (`_pbc`; `order` present);
# own_rows: an exact-shape graph keeps copies of the plan's row_ptr / batch / mol_ptr, not the plan's tensors themselves;
# too_large: the refusal of a padded graph with more than CSR_MAX_NODES nodes in a molecule.
_Source = collections.namedtuple("_Source", "fill per_edge by_source pbc given own_rows too_large")


def _sorted_by_source(src, N):
    """(src_perm, src_ptr) of an arbitrary edge list (it may repeat a source inside a row and need not be structure-blocked):
    stable device sort"""
    order = torch.argsort(src.to(torch.int64), stable=True)
    return _i32(order), _ptr_from_counts(torch.bincount(src.to(torch.int64), minlength=N))


class EdgeGraph:
    """N nodes, E directed edges sorted by dst.  All index tensors are int32 on the GPU."""

    # optional state, set by the builder that owns it.  _padded: padded to `capacity` with one phantom molecule; _pbc: periodic
    # (owns `offsets` / `cell_offsets`); _radius_static: every tensor is refilled in place by enqueue-only kernels (what a captured
    # step needs; a build that finds other counts clears it: abandoned); order: the input slot of each edge of a GIVEN edge list.
    _padded = _pbc = _radius_static = False
    z = order = offsets = cell_offsets = capacity = None

    def __init__(self, N, src, dst, row_ptr, batch=None, num_graphs=None, mol_ptr=None, max_mol_nodes=None, by_source_into=None):
        self.N = int(N)
        self.src, self.dst, self.row_ptr = src, dst, row_ptr
        self.E = int(src.shape[0])
        # by-source view: edges grouped by src (for gradients that flow back to the source node)
        if mol_ptr is not None and max_mol_nodes is not None and max_mol_nodes <= CSR_MAX_NODES and src.is_cuda:
            # radius graphs: molecule-blocked, no multi-edges -> one HIP launch instead of a device sort
            if by_source_into is not None:  # (a captured step's static graph: the same buffers every step)
                self.src_perm, self.src_ptr = by_source_into
            else:
                self.src_perm = torch.empty(self.E, dtype=torch.int32, device=src.device)
                self.src_ptr = torch.empty(self.N + 1, dtype=torch.int32, device=src.device)
            call("eqf_csr_by_source", _P(src), _P(row_ptr), _P(mol_ptr), int(mol_ptr.shape[0]) - 1, int(max_mol_nodes),
                 _P(self.src_perm), _P(self.src_ptr), _stream())
        else:
            self.src_perm, self.src_ptr = _sorted_by_source(src, self.N)
        self.batch = None
        if batch is not None:
            self.set_batch(batch, num_graphs)

    def set_batch(self, batch, num_graphs=None):
        self.batch = _i32(batch)
        if num_graphs is None:
            num_graphs = int(batch[-1].item()) + 1 if batch.numel() else 0
        self.num_graphs = int(num_graphs)
        self.mol_ptr = _ptr_from_counts(torch.bincount(batch.to(torch.int64), minlength=self.num_graphs))

    # ---- the second half of every build: the graph of a plan, exact-shape or padded --------------------------------------------
    @staticmethod
    def _new(source, N, E, num_graphs, dev, by_source=True):
        """a graph of `source`: src / dst, the per-edge tensors of the source and the by-source view allocated, nothing filled"""
        g = EdgeGraph.__new__(EdgeGraph)
        i32 = dict(dtype=torch.int32, device=dev)
        g.N, g.E, g.num_graphs = N, E, num_graphs
        g.src, g.dst = torch.empty(E, **i32), torch.empty(E, **i32)
        if by_source:
            g.src_perm, g.src_ptr = torch.empty(E, **i32), torch.empty(N + 1, **i32)
        for name, shape, dtype, _ in source.per_edge:
            setattr(g, name, torch.empty((E,) + shape, dtype=dtype, device=dev))
        g._pbc = source.pbc
        return g

    @staticmethod
    def _of_source(source, g):
        """g is a graph that `source` built and that is still refillable in place"""
        return (g is not None and g._radius_static and g._pbc == source.pbc and (g.order is not None) == source.given)

    @staticmethod
    def _build_exact(source, plan, into):
        """The exact-shape graph of `plan`.  into: an exact-shape graph of this source; with the plan's node, structure and edge
        counts every tensor of it is REWRITTEN in place and it is returned, otherwise the result is fresh and `into` is marked
        as abandoned (its owner falls back to an eager step on the fresh graph: equiformer_amd/capture.py)."""
        N, E, B = plan.N, plan.E, plan.num_graphs
        dev = plan.pos.device
        mol_ptr = plan.mol_ptr[:B + 1]
        refill = EdgeGraph._of_source(source, into) and not into._padded
        if refill and (into.N, into.E, into.num_graphs, into.src.device) != (N, E, B, dev):
            into._radius_static = refill = False
            if plan.row_ptr is into.row_ptr:  # (from_radius had the scan written straight into it)
                plan.row_ptr = plan.row_ptr.clone()  # (the caller's tensors must not alias the abandoned graph's)
        launch = refill or plan.max_mol_nodes <= CSR_MAX_NODES
        if refill:
            g = into
        else:
            g = EdgeGraph._new(source, N, E, B, dev, by_source=launch)
            if source.own_rows:
                i32 = dict(dtype=torch.int32, device=dev)
                g.row_ptr, g.batch, g.mol_ptr = torch.empty(N + 1, **i32), torch.empty(N, **i32), torch.empty(B + 1, **i32)
            else:
                g.row_ptr, g.batch, g.mol_ptr = plan.row_ptr, plan.b32, mol_ptr
        with torch.no_grad():
            for mine, planned in ((g.row_ptr, plan.row_ptr), (g.mol_ptr, mol_ptr), (g.batch, plan.b32)):
                if mine.data_ptr() != planned.data_ptr():
                    mine.copy_(planned)
        source.fill(plan, g)
        if launch:
            call(source.by_source, _P(g.src), _P(g.row_ptr), _P(g.mol_ptr), B, max(int(plan.max_mol_nodes), 1),
                 _P(g.src_perm), _P(g.src_ptr), _stream())
        else:  # (molecules beyond the cursor kernels' LDS)
            g.src_perm, g.src_ptr = _sorted_by_source(g.src, N)
        g._radius_static = launch  # (refillable in place: every tensor comes from an enqueue-only kernel)
        return g

    @staticmethod
    def _build_padded(source, plan, capacity, into, z):
        """The graph of `plan` padded to capacity = (N_cap, E_cap) with one phantom molecule (csrc/graph.hip eqf_graph_pad_tail):
        what `from_radius_plan` documents, for every source.  Phantom edges get the source's phantom row in its per-edge tensors.
        into: a padded graph of this source with the same capacity, molecule count and `z` presence, refilled in place and
        returned.  Raises GraphDoesNotFit before anything of `into` is written."""
        n_cap, e_cap = int(capacity[0]), int(capacity[1])
        N, E, B = plan.N, plan.E, plan.num_graphs
        P, Q = n_cap - N, e_cap - E
        # (P < 0 needs no test of its own: min_phantom_nodes(Q) >= 0 > P then)
        if Q < 0 or P < min_phantom_nodes(Q):
            raise GraphDoesNotFit("%d nodes / %d edges do not fit the capacity (%d, %d): %d phantom edges need %d phantom nodes"
                                  % (N, E, n_cap, e_cap, max(Q, 0), min_phantom_nodes(max(Q, 0))))
        if max(plan.max_mol_nodes, P) > CSR_MAX_NODES:
            raise ops.HipOnlyError(source.too_large % CSR_MAX_NODES)
        dev = plan.pos.device
        if (EdgeGraph._of_source(source, into) and into._padded and into.N == n_cap and into.E == e_cap
                and into.num_graphs == B + 1 and into.src.device == dev and (into.z is None) == (z is None)):
            g = into
        else:
            g = EdgeGraph._new(source, n_cap, e_cap, B + 1, dev)
            i32 = dict(dtype=torch.int32, device=dev)
            g.row_ptr, g.batch, g.mol_ptr = torch.empty(n_cap + 1, **i32), torch.empty(n_cap, **i32), torch.empty(B + 2, **i32)
            g.pos = torch.empty((n_cap, 3), dtype=torch.float32, device=dev)
            g.z = torch.empty(n_cap, dtype=torch.int64, device=dev) if z is not None else None
            g.node_mask = torch.empty(n_cap, dtype=torch.float32, device=dev)
            g.graph_mask = torch.empty(B + 1, dtype=torch.float32, device=dev)
            g._padded = g._radius_static = True
            g.capacity = (n_cap, e_cap)
        g.n_real, g.e_real, g.num_real_graphs = N, E, B
        with torch.no_grad():
            g.row_ptr[:N + 1].copy_(plan.row_ptr)
            g.mol_ptr[:B + 1].copy_(plan.mol_ptr[:B + 1])
            g.batch[:N].copy_(plan.b32)
            g.pos[:N].copy_(plan.pos)
            if z is not None:
                g.z[:N].copy_(z)
            if Q:
                for name, _, _, phantom in source.per_edge:
                    if phantom:
                        getattr(g, name)[E:].fill_(phantom)
                    else:
                        getattr(g, name)[E:].zero_()
        source.fill(plan, g)
        st = _stream()
        call("eqf_graph_pad_tail", N, E, n_cap, e_cap, B, _P(g.row_ptr), _P(g.src), _P(g.dst), _P(g.batch), _P(g.mol_ptr),
             _P(g.pos), _P(g.z), _P(g.node_mask), _P(g.graph_mask), st)
        call(source.by_source, _P(g.src), _P(g.row_ptr), _P(g.mol_ptr), B + 1, max(plan.max_mol_nodes, P, 1),
             _P(g.src_perm), _P(g.src_ptr), st)
        return g

    # ---- radius graph (csrc/graph.hip radius_graph_count / radius_graph_fill; by-source view: eqf_csr_by_source) ----------------
    @staticmethod
    def from_radius(pos, batch, r, max_num_neighbors=1000, num_graphs=None, into=None, capacity=None, z=None):
        """Radius graph per molecule (nodes of a molecule contiguous, `batch` ascending).  into: a graph of an earlier call; when
        this call finds the same node and edge counts its index tensors are REWRITTEN in place and `into` is returned -- the
        launches of a HIP-graph-captured step (equiformer_amd/capture.py) read those addresses.

        capacity=(N_cap, E_cap): the batch is padded to that shape with one phantom molecule (`from_radius_plan`); `into` is then
        a padded graph of the same capacity.  Raises GraphDoesNotFit, with `into` untouched, when the counts do not fit."""
        if capacity is not None:
            plan = EdgeGraph.radius_plan(pos, batch, r, max_num_neighbors, num_graphs)
            return EdgeGraph.from_radius_plan(plan, capacity, into=into, z=z)
        if num_graphs is None:
            num_graphs = int(batch[-1].item()) + 1
        # a candidate for in-place reuse gets the scan written straight into its row_ptr: if the edge count then differs the graph
        # is abandoned by its owner anyway -- equiformer_amd/capture.py falls back to an eager step on a fresh graph
        if not (EdgeGraph._of_source(_SEARCH, into) and not into._padded
                and (into.N, into.num_graphs, into.src.device) == (pos.shape[0], int(num_graphs), pos.device)):
            into = None
        plan = EdgeGraph.radius_plan(pos, batch, r, max_num_neighbors, num_graphs, row_ptr=None if into is None else into.row_ptr)
        return EdgeGraph._build_exact(_SEARCH, plan, into)

    @staticmethod
    def radius_plan(pos, batch, r, max_num_neighbors=1000, num_graphs=None, row_ptr=None):
        """Degrees + scan + the one host read-back of a radius graph build.  row_ptr: where the scan goes (`from_radius`: the
        row_ptr of the graph it may refill); by default a new tensor, and nothing of an earlier graph is touched."""
        if not pos.is_cuda:
            raise ops.HipOnlyError("radius graph construction runs on the GPU only")
        p = RadiusPlan()
        p.pos = pos.detach().to(torch.float32).contiguous()
        p.N = int(p.pos.shape[0])
        p.num_graphs = int(batch[-1].item()) + 1 if num_graphs is None else int(num_graphs)
        p.r, p.max_num_neighbors = float(r), int(max_num_neighbors)
        dev = p.pos.device
        p.b32 = _i32(batch)
        st = _stream()
        stats = torch.empty(2, dtype=torch.int32, device=dev)  # [E, nodes of the largest molecule]
        p.mol_ptr = torch.empty(p.num_graphs + 2, dtype=torch.int32, device=dev)  # (+ 1 entry: the phantom molecule's end)
        call("eqf_segment_ptr", _P(p.b32), p.N, p.num_graphs, _P(p.mol_ptr), _P(stats, 4), st)
        deg = torch.empty(p.N, dtype=torch.int32, device=dev)
        call("eqf_radius_graph_count", _P(p.pos), _P(p.mol_ptr), p.num_graphs, p.r, p.max_num_neighbors, _P(deg), st)
        p.row_ptr = torch.empty(p.N + 1, dtype=torch.int32, device=dev) if row_ptr is None else row_ptr
        call("eqf_exclusive_scan_i32", _P(deg), p.N, _P(p.row_ptr), _P(stats), st)
        p.E, p.max_mol_nodes = stats.tolist()  # the one host sync of graph construction (the reference syncs here as well)
        return p

    @staticmethod
    def _radius_fill(plan, g):
        """The E real edges of `plan` into the head of g.src / g.dst.  (An exact-shape graph's own mol_ptr / row_ptr are the
        plan's or equal them; a padded graph's have the phantom molecule behind the real rows, which the kernel must not see.)"""
        rows = plan if g._padded else g
        call("eqf_radius_graph_fill", _P(plan.pos), _P(rows.mol_ptr), plan.num_graphs, plan.r, plan.max_num_neighbors,
             _P(rows.row_ptr), _P(g.src), _P(g.dst), _stream())

    @staticmethod
    def from_radius_plan(plan, capacity, into=None, z=None):
        """Second half: the graph of `plan` padded to capacity = (N_cap, E_cap).  The result presents N = N_cap nodes, E = E_cap
        edges and num_graphs = B + 1 molecules to the kernels; the last molecule is a phantom that owns the tail nodes and edges
        and shares no edge with a real one.  The graph OWNS the padded per-node inputs the model is then called with: `pos`
        [N_cap, 3], `batch` [N_cap], `z` [N_cap] (int64; only when z is given), and the float masks `node_mask` [N_cap],
        `graph_mask` [B + 1] (1 real, 0 phantom); `n_real`, `e_real`, `num_real_graphs` hold the real counts (host integers:
        never use them inside a captured step).  into: a padded graph of the same capacity and molecule count, refilled in
        place and returned.  Raises GraphDoesNotFit before anything of `into` is written."""
        return EdgeGraph._build_padded(_SEARCH, plan, capacity, into, z)

    # ---- periodic radius graph (csrc/graph.hip pbc_count / pbc_fill; by-source view: eqf_csr_by_source_multi) ------------------
    @staticmethod
    def radius_pbc_plan(pos, cell, batch, r, max_num_neighbors=50, num_graphs=None):
        """Candidate counts, degrees, their scans and the one host read-back of a periodic graph build; nothing of an earlier
        graph is touched (`radius_plan` for the periodic search)."""
        if not pos.is_cuda:
            raise ops.HipOnlyError("radius graph construction runs on the GPU only")
        p = PbcPlan()
        p.pos = pos.detach().to(torch.float32).contiguous()
        p.cell = cell.detach().to(torch.float32).contiguous().view(-1, 3, 3)
        p.N = int(p.pos.shape[0])
        p.num_graphs = int(p.cell.shape[0]) if num_graphs is None else int(num_graphs)
        p.r, p.max_num_neighbors = float(r), int(max_num_neighbors)
        dev = p.pos.device
        p.b32 = _i32(batch)
        st = _stream()
        stats = torch.empty(3, dtype=torch.int32, device=dev)  # [E, nodes of the largest structure, candidates]
        p.mol_ptr = torch.empty(p.num_graphs + 2, dtype=torch.int32, device=dev)  # (+ 1 entry: a phantom structure's end)
        call("eqf_segment_ptr", _P(p.b32), p.N, p.num_graphs, _P(p.mol_ptr), _P(stats, 4), st)
        cand = torch.empty(p.N, dtype=torch.int32, device=dev)
        deg = torch.empty(p.N, dtype=torch.int32, device=dev)
        call("eqf_radius_graph_pbc_count", _P(p.pos), _P(p.cell), _P(p.mol_ptr), p.num_graphs, p.r, p.max_num_neighbors,
             _P(cand), _P(deg), st)
        p.row_ptr = torch.empty(p.N + 1, dtype=torch.int32, device=dev)
        p.cand_ptr = torch.empty(p.N + 1, dtype=torch.int32, device=dev)
        call("eqf_exclusive_scan_i32", _P(deg), p.N, _P(p.row_ptr), _P(stats), st)
        call("eqf_exclusive_scan_i32", _P(cand), p.N, _P(p.cand_ptr), _P(stats, 8), st)
        p.E, p.max_mol_nodes, p.C = stats.tolist()  # the one host sync
        return p

    @staticmethod
    def _pbc_fill(plan, g):
        """The E real edges of `plan` into the head of g's per-edge tensors (row_ptr of the plan: real rows only)."""
        scratch = torch.empty(max(plan.C, 1), dtype=torch.float32, device=plan.pos.device)
        call("eqf_radius_graph_pbc_fill", _P(plan.pos), _P(plan.cell), _P(plan.mol_ptr), plan.num_graphs, plan.r,
             plan.max_num_neighbors, _P(plan.row_ptr), _P(plan.cand_ptr), _P(scratch), _P(g.src), _P(g.dst), _P(g.cell_offsets),
             _P(g.offsets), _stream())

    @staticmethod
    def from_radius_pbc(pos, cell, batch, r, max_num_neighbors=50, num_graphs=None, into=None, capacity=None, z=None):
        """Periodic radius graph (ocpmodels radius_graph_pbc + get_pbc_distances semantics, see csrc/graph.hip).
        Returns (graph, offsets[E,3] Cartesian, cell_offsets[E,3] int32); edges are dst-sorted.  The graph keeps both per-edge
        tensors as `graph.offsets` / `graph.cell_offsets`.

        into: a periodic graph of an earlier call; when this call finds the same node, structure and edge counts every index
        tensor, `offsets` and `cell_offsets` are REWRITTEN in place and `into` is returned (what a captured step reads,
        equiformer_amd/capture.py); with other counts the result is a fresh graph and `into` is marked as abandoned.
        capacity=(N_cap, E_cap): the batch is padded to that shape with one phantom structure (`from_radius_pbc_plan`); raises
        GraphDoesNotFit, with `into` untouched, when the counts do not fit."""
        plan = EdgeGraph.radius_pbc_plan(pos, cell, batch, r, max_num_neighbors, num_graphs)
        if capacity is not None:
            g = EdgeGraph.from_radius_pbc_plan(plan, capacity, into=into, z=z)
        else:
            g = EdgeGraph._build_exact(_SEARCH_PBC, plan, into)
        return g, g.offsets, g.cell_offsets

    @staticmethod
    def from_radius_pbc_plan(plan, capacity, into=None, z=None):
        """Second half: the periodic graph of `plan` padded to capacity = (N_cap, E_cap) with one phantom structure
        (eqf_graph_pad_tail), as `from_radius_plan` pads the radius graph: N = N_cap, E = E_cap, num_graphs = B + 1, the padded
        inputs `pos`, `batch`, `z`, the masks `node_mask` / `graph_mask` and the host integers `n_real`, `e_real`,
        `num_real_graphs` have the same meaning.  In addition the graph owns `offsets` [E_cap, 3] and `cell_offsets` [E_cap, 3];
        phantom edges get zero rows in both (the phantom nodes sit on pairwise distinct lattice points: no zero-length edge).
        into: a padded periodic graph of the same capacity and structure count, refilled in place and returned.  Raises
        GraphDoesNotFit before anything of `into` is written."""
        return EdgeGraph._build_padded(_SEARCH_PBC, plan, capacity, into, z)

    # ---- a GIVEN periodic edge list (csrc/graph.hip eqf_edges_pbc_count / eqf_edges_pbc_fill; by-source view: eqf_csr_by_source_multi)
    @staticmethod
    def edges_pbc_plan(pos, cell, batch, edge_index, cell_offsets, neighbors, num_graphs=None):
        """The edge list an ocpmodels batch carries -- edge_index [2, E_in] = (neighbour, centre), integer cell_offsets [E_in, 3],
        neighbors [B] = edges per structure, cell [B, 3, 3]; int64 or int32, read as they are -- through the count kernel
        (Cartesian offsets, zero-length edges dropped: get_pbc_distances), the scans and the one host read-back: kept edges,
        nodes of the largest structure, the sum of `neighbors` and the kernel's status word.  Nothing of an earlier graph is
        touched.  Raises ValueError when `neighbors` does not sum to E_in or an edge names a node outside its structure."""
        if not pos.is_cuda:
            raise ops.HipOnlyError("graph construction runs on the GPU only")
        p = EdgesPbcPlan()
        p.pos = pos.detach().to(torch.float32).contiguous()
        p.cell = cell.detach().to(device=p.pos.device, dtype=torch.float32).contiguous().view(-1, 3, 3)
        p.N = int(p.pos.shape[0])
        p.num_graphs = int(p.cell.shape[0]) if num_graphs is None else int(num_graphs)
        dev = p.pos.device
        ints = (torch.int64, torch.int32)
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype not in ints:
            raise ValueError("edge_index must be a [2, E] int64 or int32 tensor, got %s %s" % (tuple(edge_index.shape), edge_index.dtype))
        p.E_in = int(edge_index.shape[1])
        if tuple(cell_offsets.shape) != (p.E_in, 3) or cell_offsets.dtype not in ints:
            raise ValueError("cell_offsets must be a [%d, 3] int64 or int32 tensor, got %s %s"
                             % (p.E_in, tuple(cell_offsets.shape), cell_offsets.dtype))
        if neighbors.numel() != p.num_graphs or p.cell.shape[0] != p.num_graphs:
            raise ValueError("neighbors has %d entries and cell %d, the batch has %d structures"
                             % (neighbors.numel(), p.cell.shape[0], p.num_graphs))
        # (no pass over the edges here: `.to` / `.contiguous()` of a contiguous device tensor return it as it is)
        p.edge_index = edge_index.detach().to(dev).contiguous()
        p.cell_offsets = cell_offsets.detach().to(dev).contiguous()
        p.index64, p.offsets64 = int(edge_index.dtype == torch.int64), int(cell_offsets.dtype == torch.int64)
        p.b32 = _i32(batch)
        nb32 = neighbors.detach().to(device=dev, dtype=torch.int32).reshape(-1).contiguous()  # ([B]: not a per-edge pass)
        st = _stream()
        stats = torch.empty(4, dtype=torch.int32, device=dev)  # [E, nodes of the largest structure, sum of neighbors, status]
        p.mol_ptr = torch.empty(p.num_graphs + 2, dtype=torch.int32, device=dev)  # (+ 1 entry: a phantom structure's end)
        call("eqf_segment_ptr", _P(p.b32), p.N, p.num_graphs, _P(p.mol_ptr), _P(stats, 4), st)
        p.nbr_ptr = torch.empty(p.num_graphs + 1, dtype=torch.int32, device=dev)
        call("eqf_exclusive_scan_i32", _P(nb32), p.num_graphs, _P(p.nbr_ptr), _P(stats, 8), st)
        p.keep = torch.empty(p.E_in, dtype=torch.uint8, device=dev)
        p.off = torch.empty((p.E_in, 3), dtype=torch.float32, device=dev)
        deg = torch.empty(p.N, dtype=torch.int32, device=dev)
        call("eqf_edges_pbc_count", _P(p.pos), _P(p.cell), _P(p.mol_ptr), _P(p.nbr_ptr), p.num_graphs, p.N, _P(p.edge_index),
             p.index64, _P(p.cell_offsets), p.offsets64, p.E_in, _P(p.keep), _P(p.off), _P(deg), _P(stats, 12), st)
        p.row_ptr = torch.empty(p.N + 1, dtype=torch.int32, device=dev)
        call("eqf_exclusive_scan_i32", _P(deg), p.N, _P(p.row_ptr), _P(stats), st)
        p.E, p.max_mol_nodes, total, status = stats.tolist()  # the one host sync
        if total != p.E_in:
            raise ValueError("data.neighbors sums to %d, data.edge_index has %d edges" % (total, p.E_in))
        if status:
            raise ValueError("data.edge_index has an edge whose neighbour or centre lies outside the structure that data.neighbors "
                             "assigns it to (status %d)" % status)
        if p.max_mol_nodes > CSR_MAX_NODES:
            raise ops.HipOnlyError("graphs from a given edge list need structures of at most %d nodes" % CSR_MAX_NODES)
        return p

    @staticmethod
    def _edges_pbc_fill(plan, g):
        """The E kept edges of `plan` into the head of g's per-edge tensors (row_ptr of the plan: real rows only)."""
        call("eqf_edges_pbc_fill", _P(plan.mol_ptr), _P(plan.nbr_ptr), plan.num_graphs, int(plan.max_mol_nodes),
             _P(plan.edge_index), plan.index64, _P(plan.cell_offsets), plan.offsets64, plan.E_in, _P(plan.keep), _P(plan.off),
             _P(plan.row_ptr), plan.E, _P(g.src), _P(g.dst), _P(g.cell_offsets), _P(g.offsets), _P(g.order), _stream())

    @staticmethod
    def from_edges_pbc_plan(plan, capacity=None, into=None, z=None):
        """Second half: the dst-sorted graph of the plan's kept edges, stable in input order.  Beside the index tensors the graph
        owns `offsets` [E, 3] (fp32 Cartesian), `cell_offsets` [E, 3] (int32) and `order` [E] (int32: the input index of the edge in
        each slot, for further per-edge data of the caller), and carries `_pbc = _radius_static = True`: every tensor is refilled
        in place by enqueue-only kernels.

        capacity=None: an exact-shape graph; `into` (a graph of this builder with the same node, structure and kept-edge counts)
        is REWRITTEN in place and returned, with other counts the result is fresh and `into` is marked as abandoned.
        capacity=(N_cap, E_cap): padded with one phantom structure exactly as `from_radius_pbc_plan` pads (the same padded
        inputs, masks and host integers; `_padded`); phantom edges get zero rows in `offsets` / `cell_offsets` and -1 in `order`;
        `into` is a padded graph of this builder with the same capacity and structure count.  Raises GraphDoesNotFit before
        anything of `into` is written."""
        if capacity is None:
            return EdgeGraph._build_exact(_GIVEN_PBC, plan, into)
        return EdgeGraph._build_padded(_GIVEN_PBC, plan, capacity, into, z)

    @staticmethod
    def from_edges_pbc(pos, cell, batch, edge_index, cell_offsets, neighbors, num_graphs=None, into=None, capacity=None, z=None):
        """`edges_pbc_plan` + `from_edges_pbc_plan`: returns (graph, offsets [E, 3] Cartesian, cell_offsets [E, 3] int32), the
        conventions of `from_radius_pbc` for a batch that brings its own edge list (OC20 with otf_graph=False)."""
        plan = EdgeGraph.edges_pbc_plan(pos, cell, batch, edge_index, cell_offsets, neighbors, num_graphs)
        g = EdgeGraph.from_edges_pbc_plan(plan, capacity, into=into, z=z)
        return g, g.offsets, g.cell_offsets

    @staticmethod
    def from_edges(edge_src, edge_dst, N, batch=None, num_graphs=None):
        """Arbitrary edge list (e.g. periodic-boundary edges computed upstream); sorted by dst here.
        Returns (graph, order) with order = permutation applied to the caller's per-edge data."""
        order = torch.argsort(edge_dst.to(torch.int64), stable=True)
        src = _i32(edge_src[order])
        dst = _i32(edge_dst[order])
        row_ptr = _ptr_from_counts(torch.bincount(dst.to(torch.int64), minlength=N))
        return EdgeGraph(N, src, dst, row_ptr, batch, num_graphs), order


_PBC_EDGE = (("offsets", (3,), torch.float32, 0), ("cell_offsets", (3,), torch.int32, 0))
_PBC_TOO_LARGE = "padded periodic graphs need structures (the phantom one included) of at most %d nodes"
_SEARCH = _Source(EdgeGraph._radius_fill, (), "eqf_csr_by_source", False, False, False,
                  "padded radius graphs need molecules (the phantom one included) of at most %d nodes")
_SEARCH_PBC = _Source(EdgeGraph._pbc_fill, _PBC_EDGE, "eqf_csr_by_source_multi", True, False, False, _PBC_TOO_LARGE)
_GIVEN_PBC = _Source(EdgeGraph._edges_pbc_fill, _PBC_EDGE + (("order", (), torch.int32, -1),), "eqf_csr_by_source_multi", True,
                     True, True, _PBC_TOO_LARGE)
