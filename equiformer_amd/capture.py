"""A train step captured in a HIP graph: forward + loss + backward + fused AdamW replayed as ONE graph launch.

Every entry point of include/equiformer_hip.h only enqueues work on the caller's stream (no allocation, no synchronisation),
so the ~280 launches of a QM9 step are legal inside a stream capture (tests/test_gpu_capture.py); replaying them removes the
host's launch path from the step -- ~0.4 ms of gaps at the head of an eager 10-ms step (profiles/r05/r05_fin_step_timeline.txt).
[ref: the train loop, engine.py:58-92; SURVEY.md 8d "HIP-graph captured where possible"]

What stays OUTSIDE the graph, and why:
  * the radius graph (EdgeGraph.from_radius; periodic structures: EdgeGraph.from_radius_pbc): its edge count is the one data-dependent size of the step and is read back on
    the host.  The captured launches address the index tensors of the graph object the capture ran on; every later step
    rebuilds the radius graph INTO those tensors (`from_radius(into=...)`, `from_radius_pbc(into=...)`: the graph's flag
    `_radius_static` says "every tensor of it is refilled in place by enqueue-only kernels", whichever builder made it -- the
    by-source view of the periodic graph comes from eqf_csr_by_source_multi, not from a device sort).  `CapturedTrainStep` keys its graphs on the exact
    (nodes, edges): a step whose counts differ runs eagerly (and, from `min_eager` eager steps of a shape on, gets a graph of
    its own).  Batches of a real loader change both counts nearly every step: `BucketedTrainStep` (below) pads each batch to
    the capacity of a shape bucket with one phantom molecule and keeps one graph per bucket, so almost every step replays.
  * three numbers the captured launches read from device words instead of frozen by-value arguments: the seed offset of
    the attention dropout (a fresh draw per replay: eqf_attn_aggregate_*_dseed) and {lr, 1 - b1^t, sqrt(1 - b2^t)} of AdamW
    (eqf_adamw_step_dev); the host writes them (pinned buffer, asynchronous copy) before it launches the graph.
  * per-graph stochastic depth (`drop_path_rate > 0`) likewise: the step classes run every step, eager or captured, inside
    `droppath.device_draws(word)`, so GraphDropPath draws its keep mask in the kernel (eqf_segment_droppath) from a second
    device word that holds `droppath.step_seed(drop_path_seed, k)` during step k of the instance -- a fresh mask per replay, the
    same masks as an eager loop under `device_draws(step_seed(drop_path_seed, k))`, padded or not (the draw of a graph does not
    depend on the number of graphs).  `drop_path_seed=None` draws the base seed from torch's CPU generator when the first
    GraphDropPath runs; a model without stochastic depth consumes nothing.
  * the equivariant dropouts (`out_drop`, `proj_drop`: equiformer_amd/dropout.py) draw in the same scope from the same word:
    `drop_path_seed` seeds both streams, which the kernels keep apart by stream tag (32 and 33) and the scope by two call
    counters.  A step drops the entries `dropout.keep_mask(step_seed(drop_path_seed, k), call, rows, irreps, p)` names, on the
    real rows of a padded batch as on the unpadded batch (the draw of a row does not depend on the number of rows).

The MD17 force-loss step (forces by a create_graph backward inside the forward, then a second-order backward) is captured the
same way (tests/test_gpu_capture.py; bench.py --workload md17_l2: 463 -> 619 frames/s, md17_l3: 218 -> 254).  The OC20 step on
periodic structures (`model(data, graph=g, offsets=g.offsets)`) is captured exact-shape and bucketed alike
(tests/test_gpu_periodic_capture.py, tools/bench_varying_oc20.py).

Limits: one process / one GPU (a data-parallel reducer's collectives stay eager: `CapturedTrainStep` refuses a reducer),
attention dropout together with a create_graph backward (no model of the reference combines them), graphs built by the enqueue-only
builders only -- from positions (`from_radius`, `from_radius_pbc`) or from the periodic edge list an OC20 batch carries
(`from_edges_pbc`: otf_graph=False; the step classes take it with `edges="batch"`); an arbitrary edge list without the
`neighbors` / `cell_offsets` contract still goes through EdgeGraph.from_edges and its device sort: eager --, structures of at most
`graph.CSR_MAX_NODES` nodes, inputs other than the graph at fixed addresses (`forward_loss` reads the same tensors every step;
copy a new batch into them).

How the classes are put together: `_CapturingStep` holds the capture protocol (record, file the record, words out, first replay)
and the replay, with the optimizer's share of both left out where there is no optimizer; `_TrainStep` adds what a train step
is made of (the eager step that is also what a capture records, the dropout seed word, the stochastic-depth word);
`_BucketedStep` adds the bucket records and the one `step` of the bucketed classes, which BucketedTrainStep and
evaluate.BucketedEvalStep complete with `_run`, their pre-checks, the words they send and how a record's outputs are returned.
`_DeviceWord` is the pinned host word + device word + asynchronous copy that every such number travels through."""
import collections
import contextlib
import functools

import torch

from . import droppath, ops
from .droppath import step_seed
from .graph import EdgeGraph, min_phantom_nodes


class _DeviceWord:
    """One int64 that captured launches read from device memory (`.dev`), written by the host through a pinned word (`.host`) and
    an asynchronous copy.  (The graph build's host read-back follows every write and waits for it: the pinned word is free
    again when the next step writes it.)"""

    def __init__(self, device):
        self.dev = torch.zeros(1, dtype=torch.int64, device=device)
        self.host = torch.zeros(1, dtype=torch.int64).pin_memory()

    def write(self, v):
        self.host[0] = v
        self.dev.copy_(self.host, non_blocking=True)


def _draw_seed(word):
    """a fresh seed offset of the attention dropout into its device word"""
    word.write(int(torch.randint(0, 2 ** 62, (1,)).item()))  # CPU generator, as the eager layers draw theirs


class _DropPathWord(_DeviceWord):
    """The stochastic-depth seed of a step class: a device word that holds `step_seed(seed, k)` during step k (k counts the
    steps of the instance from 0).  seed None: the word holds `step_seed(0, k)` and the base seed travels by value (a
    constant: a capture may freeze it), drawn from torch's CPU generator by the first GraphDropPath (or equivariant dropout:
    the same scope seeds both) that really runs under the instance -- a model without stochastic depth and dropout consumes
    nothing."""

    def __init__(self, seed, device):
        super().__init__(device)
        self.seed = None if seed is None else int(seed)
        self.k = 0
        self._drawn = None

    def base(self):
        if self._drawn is None:
            self._drawn = int(torch.randint(0, 2 ** 62, (1,)).item())  # CPU generator, as the eager layers draw theirs
        return self._drawn

    def advance(self):
        """the word of the next step goes out"""
        v = step_seed(self.seed or 0, self.k)
        self.k += 1
        self.write(v - (1 << 64) if v >= (1 << 63) else v)  # the same 64 bits inside int64's signed range

    def scope(self):
        return droppath.device_draws(self.dev, base=0 if self.seed is not None else self.base)


def _advance(word):
    if word is not None:
        word.advance()


def _scope(word):
    return word.scope() if word is not None else contextlib.nullcontext()


def _refuse_reducer(optimizer, name):
    if getattr(optimizer, "_reducer", None) is not None:
        raise ValueError("%s: data-parallel steps stay eager (the reducer's collectives are not captured)" % name)


class _CapturingStep:
    """The capture protocol of the step classes, written once.  A train step has `opt` (a FlatAdamW, whose device words and
    step count the protocol looks after) and `_seed` (the _DeviceWord of the attention dropout's seed offset); an evaluation
    step has neither, and the optimizer's share of the protocol is left out."""

    opt = _seed = None

    def _capture(self, run, store, **kept):
        """Record run() in a HIP graph, hand the record -- dict(graph=the CUDAGraph, out=what run returned, **kept) -- to `store`,
        which files it, and replay the graph once: capturing enqueued nothing.  The launches record the addresses of the
        EdgeGraph's tensors, of the inputs run() reads and of the gradients / activations / outputs the graph's private pool
        hands out.  Returns what run returned."""
        train = self.opt is not None
        if train:
            self.opt.device_hyper(True)
        graph = torch.cuda.CUDAGraph()
        with ops.dropout_seed_offset(self._seed.dev) if train else contextlib.nullcontext(), ops._arena.capture_scope():
            step_before = self.opt._step if train else None
            with torch.cuda.graph(graph):
                out = run()
            if train:
                self.opt._step = step_before  # (the step count advances with the replays)
        store(dict(graph=graph, out=out, **kept))
        if train:
            _draw_seed(self._seed)
        self._replay(graph)
        return out

    def _replay(self, graph):
        if self.opt is not None:
            self.opt.advance_captured()
        graph.replay()
        self.replays += 1


class _TrainStep(_CapturingStep):
    """What the two train steps are made of: optimizer, forward_loss, the two device words and the eager step."""

    _drop_path = None  # the _DropPathWord the constructor makes (an instance built without it draws on the host, as before)

    def _init_train(self, optimizer, forward_loss, drop_path_seed):
        self.opt, self.forward_loss = optimizer, forward_loss
        dev = optimizer.flat_p.device
        self._seed = _DeviceWord(dev)
        self._drop_path = _DropPathWord(drop_path_seed, dev)

    def _run(self, g, *view):
        """one eager step (also what a captured graph records)"""
        with _scope(self._drop_path):  # (eager steps and the capture alike: one sequence of stochastic-depth masks)
            self.opt.zero_grad(set_to_none=True)
            loss = self.forward_loss(g, *view)
            loss.backward()
            self.opt.step()
        # detached: a caller that keeps the loss of an EAGER step must not keep that step's autograd graph alive into a later
        # capture (hipStreamEndCapture crashed with one alive, round 6)
        return loss.detach()


class CapturedTrainStep(_TrainStep):
    """cs = CapturedTrainStep(model_params_owner_optimizer, forward_loss)
       loss = cs.step(build_graph)          # every train step

    forward_loss(graph) -> scalar loss, reading the batch from tensors that keep their addresses; build_graph(into) -> the
    EdgeGraph of this step's batch (`EdgeGraph.from_radius(pos, batch, r, into=into)`, or for periodic structures
    `EdgeGraph.from_radius_pbc(pos, cell, batch, r, k, into=into)[0]`, whose `.offsets` forward_loss passes on), called OUTSIDE
    the capture.
    optimizer: a FlatAdamW without a reducer.  drop_path_seed: the seed of stochastic depth and of the equivariant dropouts
    (module docstring; None: drawn)."""

    def __init__(self, optimizer, forward_loss, min_eager=3, max_graphs=4, drop_path_seed=None):
        _refuse_reducer(optimizer, "CapturedTrainStep")
        self._init_train(optimizer, forward_loss, drop_path_seed)
        self.min_eager, self.max_graphs = int(min_eager), int(max_graphs)
        self._graphs = {}   # (N, E) -> dict(graph=CUDAGraph, out=the loss, sg=EdgeGraph)
        self._seen = {}     # (N, E) -> eager steps so far (counts only: an EdgeGraph kept here would never be freed)
        self.replays = self.eager_steps = 0

    def step(self, build_graph):
        _advance(self._drop_path)
        # the radius graph of this batch: into the tensors of a captured shape when one fits (tried most recent first)
        g = None
        for key, rec in reversed(list(self._graphs.items())):
            if not rec["sg"]._radius_static:  # (abandoned by a build that found another edge count)
                del self._graphs[key]
                continue
            _draw_seed(self._seed)  # (the device words go out BEFORE the graph build's host read-back: they overlap it)
            g = build_graph(rec["sg"])
            if g is rec["sg"]:
                self._replay(rec["graph"])
                return rec["out"]
            del self._graphs[key]  # its tensors were overwritten by the build of another shape: the graph is gone
            break  # (one rebuild attempt per step: a second one would repeat the neighbour search)
        if g is None:
            g = build_graph(None)
        key = (g.N, g.E)
        n = self._seen.get(key, 0)
        if n < self.min_eager or len(self._graphs) >= self.max_graphs or not g._radius_static:
            self._seen[key] = n + 1
            self.eager_steps += 1
            return self._run(g)
        return self._capture(lambda: self._run(g), functools.partial(self._graphs.__setitem__, key), sg=g)


# ---------------------------------------------------------------------------------------------------------------------------------
# Batches whose node / edge counts change from step to step (a real loader): one graph per shape BUCKET, not per exact shape.
DEFAULT_NODE_STEP = 64     # QM9 bench batch (N = 2 304, E ~ 25 354): (33 reserved + 32 mean round-up) / 2 304 = 2.8 % padded nodes,
DEFAULT_EDGE_STEP = 1024   # 512 / 25 354 = 2.0 % padded edges on average, 4.0 % at most
_SEEN_MAX = 4096           # bucket keys the eager-step counter remembers


def bucket_of(B, N, E, node_step=DEFAULT_NODE_STEP, edge_step=DEFAULT_EDGE_STEP):
    """(B, N_cap, E_cap) of a batch of B molecules, N nodes, E edges.  E_cap: E rounded up to a multiple of edge_step, so at most
    edge_step - 1 phantom edges; N_cap: N plus the phantom nodes that many edges can need (`min_phantom_nodes(edge_step - 1)`,
    reserved whatever E is, so that the bucket depends on N and E separately), rounded up to a multiple of node_step.  A pure
    host function of its arguments."""
    node_step, edge_step = int(node_step), int(edge_step)
    if node_step < 1 or edge_step < 1:
        raise ValueError("bucket steps must be positive")
    e_cap = -(-int(E) // edge_step) * edge_step
    n_cap = -(-(int(N) + min_phantom_nodes(edge_step - 1)) // node_step) * node_step
    return int(B), n_cap, e_cap


def bucket_corner(key, node_step=DEFAULT_NODE_STEP, edge_step=DEFAULT_EDGE_STEP):
    """The largest real (N, E) that `bucket_of` maps to the bucket `key`."""
    return key[1] - min_phantom_nodes(int(edge_step) - 1), key[2]


GIVEN_EDGE_FIELDS = ("edge_index", "cell_offsets", "neighbors", "cell")


def given_edge_fields(batch):
    """The fields a batch must carry for `edges="batch"`, the ocpmodels contract of otf_graph=False: `edge_index` [2, E]
    (neighbour, centre), `cell_offsets` [E, 3] (integer images), `neighbors` [B] (edges per structure), `cell` [B, 3, 3].  Raises
    ValueError naming every missing one (a non-periodic batch has no `cell`); returns the names.  batch: a mapping or an object
    with attributes.  A pure host function."""
    has = (lambda n: n in batch and batch[n] is not None) if hasattr(batch, "keys") else (lambda n: getattr(batch, n, None) is not None)
    missing = [n for n in GIVEN_EDGE_FIELDS if not has(n)]
    if missing:
        raise ValueError("edges=\"batch\" needs the batch's own periodic edge list: %s missing (needed: %s)"
                         % (", ".join(missing), ", ".join(GIVEN_EDGE_FIELDS)))
    return GIVEN_EDGE_FIELDS


class PaddedBatch:
    """What `forward_loss(graph, view)` of a BucketedTrainStep reads: the padded inputs `pos` [N_cap, 3], `z` [N_cap], `batch`
    [N_cap], the masks `node_mask` [N_cap] / `graph_mask` [B + 1] (1.0 real, 0.0 phantom), `B` (real molecules: constant per
    bucket, the only count that may be used as a Python number) and every target under its own name, padded with zero rows to
    B + 1 (per molecule) or N_cap (per node).  Periodic batches: also `offsets` [E_cap, 3] / `cell_offsets` [E_cap, 3] (zero rows
    for phantom edges) and `atomic_numbers` (= `z`), so that the view itself is the `data` of the OC20 model:
    `model(view, graph=graph, offsets=view.offsets)` with "tags" among the node targets."""


class _BucketedStep(_CapturingStep):
    """What BucketedTrainStep and equiformer_amd.evaluate.BucketedEvalStep share: the bucket records with their LRU order and
    counters, the padded view of a bucket's graph, its target buffers, the plan of the batch's graph (the one host read-back) with
    its bucket key, and `step` itself.  A subclass supplies `_run(g, view)` (one eager step, also what a capture records) and,
    where it has any, `_check` (its pre-checks), `_words_out` (the device words of the step) and `_returned` (how the outputs
    of a run or of a record are handed to the caller)."""

    def _init_buckets(self, radius, graph_targets, node_targets, min_eager, max_graphs, node_step, edge_step, max_num_neighbors,
                      edges="search"):
        if edges not in ("search", "batch"):
            raise ValueError("edges must be \"search\" (neighbours found on the GPU) or \"batch\" (the batch's own edge list), got %r"
                             % (edges,))
        self.edges = edges  # ("batch": radius and max_num_neighbors do not enter the graph)
        self.radius, self.max_num_neighbors = float(radius), int(max_num_neighbors)
        self.graph_targets, self.node_targets = tuple(graph_targets), tuple(node_targets)
        self.min_eager, self.max_graphs = int(min_eager), max(1, int(max_graphs))
        self.node_step, self.edge_step = int(node_step), int(edge_step)
        self._graphs = collections.OrderedDict()  # bucket key -> the record of a captured bucket, least recently used first
        self._seen = collections.OrderedDict()    # bucket key -> eager steps so far (counts only, at most _SEEN_MAX keys)
        self.replays = self.eager_steps = self.captures = self.evictions = 0
        self.real_edges = self.padded_edges = self.real_nodes = self.padded_nodes = 0
        self.captures_of = {}  # bucket key -> captures (a key captured twice was evicted in between)
        self._periodic = None  # set by the first batch

    def live_graphs(self):
        return list(self._graphs)

    def _view(self, g, B):
        v = PaddedBatch()
        # (detached aliases: a model that marks `pos` as requiring grad -- the MD17 force pass -- must not mark the graph's buffer)
        v.pos, v.z, v.batch = g.pos.detach(), g.z, g.batch
        v.node_mask, v.graph_mask, v.B = g.node_mask, g.graph_mask, B
        if g._pbc:
            v.offsets, v.cell_offsets, v.atomic_numbers = g.offsets, g.cell_offsets, g.z
        return v

    def _fill_targets(self, view, batch, g, B, fresh):
        with torch.no_grad():
            for names, rows, real in ((self.graph_targets, B + 1, B), (self.node_targets, g.N, g.n_real)):
                for name in names:
                    t = batch[name]
                    if t.shape[0] != real:
                        raise ValueError("target %r has %d rows, the batch has %d" % (name, t.shape[0], real))
                    if fresh:
                        setattr(view, name, torch.zeros((rows,) + tuple(t.shape[1:]), dtype=t.dtype, device=g.src.device))
                    buf = getattr(view, name)
                    buf[:real].copy_(t, non_blocking=True)
                    if not fresh:
                        buf[real:].zero_()

    def _plan(self, batch):
        """(B, z, plan, build, key) of a batch: the graph plan (its host read-back happens here) and the bucket it falls into"""
        b = batch["batch"]
        B = int(batch["num_graphs"]) if "num_graphs" in batch else int(b[-1].item()) + 1
        z = batch["z"] if "z" in batch else batch.get("atomic_numbers")
        if self.edges == "batch":
            plan = EdgeGraph.edges_pbc_plan(batch["pos"], batch["cell"], b, batch["edge_index"], batch["cell_offsets"],
                                            batch["neighbors"], B)
            build = EdgeGraph.from_edges_pbc_plan
        elif self._periodic:
            plan = EdgeGraph.radius_pbc_plan(batch["pos"], batch["cell"], b, self.radius, self.max_num_neighbors, B)
            build = EdgeGraph.from_radius_pbc_plan
        else:
            plan = EdgeGraph.radius_plan(batch["pos"], b, self.radius, self.max_num_neighbors, B)
            build = EdgeGraph.from_radius_plan
        key = bucket_of(B, plan.N, plan.E, self.node_step, self.edge_step)
        self.real_nodes += plan.N
        self.real_edges += plan.E
        self.padded_nodes += key[1]
        self.padded_edges += key[2]
        return B, z, plan, build, key

    def _check_periodic(self, batch):
        if self.edges == "batch":
            given_edge_fields(batch)  # (a non-periodic batch lacks `cell`: refused here)
        periodic = "cell" in batch
        if self._periodic is None:
            self._periodic = periodic
        elif self._periodic != periodic:
            raise ValueError("%s: one instance serves periodic or non-periodic batches, not both" % type(self).__name__)

    def _count_eager(self, key):
        """True while the bucket `key` still runs eagerly (its first `min_eager` steps); counts the step then"""
        n = self._seen.get(key, 0)
        if n >= self.min_eager:
            return False
        self._seen[key] = n + 1
        self._seen.move_to_end(key)
        while len(self._seen) > _SEEN_MAX:
            self._seen.popitem(last=False)
        self.eager_steps += 1
        return True

    def _make_room(self):
        while len(self._graphs) >= self.max_graphs:  # least recently used out; its bucket earns a graph again
            old, _ = self._graphs.popitem(last=False)
            self._seen.pop(old, None)
            self.evictions += 1

    def _captured(self, key, rec):
        self._graphs[key] = rec
        self.captures += 1
        self.captures_of[key] = self.captures_of.get(key, 0) + 1

    def _check(self, batch):
        self._check_periodic(batch)

    def _words_out(self):
        pass

    def _returned(self, out, B, n_real):
        return out

    def step(self, batch):
        self._check(batch)  # (before the batch is touched)
        self._words_out()   # (the device words go out BEFORE the graph build's host read-back: they overlap it)
        B, z, plan, build, key = self._plan(batch)
        rec = self._graphs.get(key)
        if rec is not None:
            self._graphs.move_to_end(key)
            build(plan, key[1:], into=rec["sg"], z=z)
            self._fill_targets(rec["view"], batch, rec["sg"], B, fresh=False)
            self._replay(rec["graph"])
            return self._returned(rec["out"], B, plan.N)
        g = build(plan, key[1:], z=z)
        view = self._view(g, B)
        self._fill_targets(view, batch, g, B, fresh=True)
        if self._count_eager(key):
            return self._returned(self._run(g, view), B, plan.N)
        self._make_room()
        # capture this bucket: beside what every capture records (_capture), the launches hold the addresses of the view's
        # buffers; they see N_cap, E_cap and B + 1 only
        out = self._capture(lambda: self._run(g, view), functools.partial(self._captured, key), sg=g, view=view)
        return self._returned(out, B, plan.N)


class BucketedTrainStep(_TrainStep, _BucketedStep):
    """bs = BucketedTrainStep(optimizer, forward_loss, radius, graph_targets=("y",), node_targets=())
       loss = bs.step(batch)        # batch: mapping with pos [N, 3], z [N], batch [N] (ascending) and the targets; N, E vary

    A batch with `cell` [B, 3, 3] is periodic: the graph is the periodic one (EdgeGraph.radius_pbc_plan / from_radius_pbc_plan,
    `radius` and `max_num_neighbors` of the constructor), `atomic_numbers` is accepted for `z`, and per-node INPUTS such as the
    OC20 `tags` travel through `node_targets` (a zero row is a valid tag).  One instance serves periodic or non-periodic
    batches, not both.  edges="batch": the periodic batch brings its own edge list (`given_edge_fields`: edge_index, cell_offsets,
    neighbors, cell -- what an OC20 LMDB delivers, the reference's otf_graph=False); the graph is EdgeGraph.edges_pbc_plan /
    from_edges_pbc_plan, no neighbour search runs, and `radius` / `max_num_neighbors` do not enter it.

    Every batch is padded to the capacity of its bucket (`bucket_of`) with one phantom molecule (EdgeGraph.from_radius(...,
    capacity=)), the unchanged kernels run on the padded shape, and one HIP graph per BUCKET replays forward + loss + backward +
    AdamW.  The phantom molecule shares no edge with a real one; layer norm is per node, softmax per destination, pooling per
    molecule: real rows are what the unpadded step computes.  forward_loss(graph, view) -> scalar loss must keep the phantom rows
    out of the loss: reduce per-molecule outputs over `[:view.B]`, per-node outputs with `view.node_mask` -- never with the real
    node or edge count, which a capture would freeze.  The phantom rows then get a zero upstream gradient and add exact zeros to
    every parameter gradient.  With drop_path_rate > 0 the phantom molecule is graph B with a draw of its own (droppath.py): the
    real molecules keep the draws of the unpadded step.

    Records are looked up by the step's own bucket key and live side by side; `max_graphs` is honoured by evicting the least
    recently used one (its bucket has to be seen `min_eager` times again).  Each record owns its static inputs (the padded graph
    and target buffers of its bucket), so a batch of another bucket never invalidates a graph.  Eager steps (the first `min_eager`
    of a bucket) run on the same padded inputs as the replays.  Dropout seed word, stochastic-depth seed word (`drop_path_seed`)
    and AdamW device words as CapturedTrainStep; a reducer is refused likewise."""

    def __init__(self, optimizer, forward_loss, radius, graph_targets=("y",), node_targets=(), min_eager=3, max_graphs=16,
                 node_step=DEFAULT_NODE_STEP, edge_step=DEFAULT_EDGE_STEP, max_num_neighbors=1000, drop_path_seed=None,
                 edges="search"):
        _refuse_reducer(optimizer, "BucketedTrainStep")
        self._init_buckets(radius, graph_targets, node_targets, min_eager, max_graphs, node_step, edge_step, max_num_neighbors,
                           edges)
        self._init_train(optimizer, forward_loss, drop_path_seed)

    def _words_out(self):
        _draw_seed(self._seed)
        _advance(self._drop_path)


class _MirrorsBucketed:
    """the counters of the BucketedTrainStep a task step (dens.py, is2rs.py) wraps as `.bucketed`"""
    eager_steps = property(lambda self: self.bucketed.eager_steps)
    captures = property(lambda self: self.bucketed.captures)
    replays = property(lambda self: self.bucketed.replays)
