"""Event-order trace of the step classes -- capture.CapturedTrainStep, capture.BucketedTrainStep, evaluate.BucketedEvalStep --
taken on the CPU.  Replaced while a sequence runs, here and nowhere else: `torch.Tensor.pin_memory` (identity),
`torch.cuda.CUDAGraph` and `torch.cuda.graph` (stubs that record capture enter / exit and replay and run the body),
`ops._arena.capture_scope`, `ops.dropout_seed_offset` and `droppath.device_draws` (record), the plan / build statics of EdgeGraph
(stubs that return objects with the chosen counts and tiny CPU tensors and record `build(into=...)`), and the optimizer (a stub
that records zero_grad, step, device_hyper, advance_captured and every read and write of `_step`).  A TorchFunctionMode adds the
torch calls the steps themselves issue: `randint` (a draw from the CPU generator), `zeros` (a new buffer), `copy_` and `zero_`
with destination and source, and the value a copy puts into the stochastic-depth word.

Tensors are named by the storage they lie in: `graph#k.field` (a stub graph), `batch#i.field` (the batch of step i),
`drop_path_word`, `seed_word` (what `dropout_seed_offset` was handed), `fresh#k` otherwise (numbered by first appearance) --
followed by the byte offset and the shape.  After every step the trace holds what the step returned and the counters.

`trace_all()` returns {sequence: [event, ...]}; tests/golden/step_trace.json holds what it returned when the capture protocol
was written once per class (python tests/step_trace.py PATH writes such a file)."""
import contextlib
import json
import os
import sys

import torch
from torch.overrides import TorchFunctionMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from equiformer_amd import capture, droppath, evaluate, ops  # noqa: E402
from equiformer_amd.graph import EdgeGraph  # noqa: E402

B = 2
NODE_STEP, EDGE_STEP = 16, 8
SHAPES = {"A": [(5, 6), (4, 7)], "B": [(5, 12)]}  # (N, E) of the batches of a bucket: A -> (2, 16, 8), B -> (2, 16, 16)
KEYS = "AAAABBBA"
COUNTERS = ("replays", "eager_steps", "captures", "evictions", "real_nodes", "real_edges", "padded_nodes", "padded_edges")
PLANS = {"radius_plan": "from_radius_plan", "radius_pbc_plan": "from_radius_pbc_plan", "edges_pbc_plan": "from_edges_pbc_plan"}


class _Recorder(TorchFunctionMode):
    def __init__(self):
        super().__init__()
        self.events = []
        self.stores = {}   # base address -> storage (kept alive: no address is handed out twice during a sequence)
        self.names = {}    # base address -> name
        self.drop_path_word = None

    def add(self, *event):
        self.events.append(list(event))

    def register(self, t):
        if torch.is_tensor(t) and t.numel():
            stor = t.untyped_storage()
            self.stores.setdefault(stor.data_ptr(), stor)
        elif isinstance(t, (tuple, list)):
            for x in t:
                self.register(x)

    def name(self, owner, fields):
        for field, t in sorted(fields.items()):
            if torch.is_tensor(t) and t.numel():
                self.register(t)
                self.names.setdefault(t.untyped_storage().data_ptr(), "%s.%s" % (owner, field) if field else owner)

    def ref(self, t):
        if not torch.is_tensor(t):
            return t
        self.register(t)
        base = t.untyped_storage().data_ptr()
        return ("ref", base, t.data_ptr() - base, list(t.shape))

    def __torch_function__(self, func, types_, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        for a in args:
            self.register(a)
        out = func(*args, **kwargs)
        self.register(out)
        if name == "randint":
            self.add("randint")
        elif name == "zeros":
            self.add("zeros", self.ref(out), str(out.dtype))
        elif name == "zero_":
            self.add("zero_", self.ref(args[0]))
        elif name == "copy_":
            e = ["copy_", self.ref(args[0]), self.ref(args[1]), {"non_blocking": bool(kwargs.get("non_blocking", False))}]
            if self.drop_path_word is not None and args[0].data_ptr() == self.drop_path_word.data_ptr():
                e.append({"value": int(args[1][0]) % (1 << 64)})
            self.events.append(e)
        return out

    def resolved(self):
        names, fresh = dict(self.names), {}

        def res(v):
            if isinstance(v, tuple) and v and v[0] == "ref":
                if v[1] not in names:
                    names[v[1]] = fresh[v[1]] = "fresh#%d" % len(fresh)
                return [names[v[1]]] + list(v[2:])
            if isinstance(v, (list, tuple)):
                return [res(x) for x in v]
            if isinstance(v, dict):
                return {str(k): res(x) for k, x in v.items()}
            return v
        return [res(e) for e in self.events]


# ------------------------------------------------------------------------------------------------- stubs
class _Opt:
    """the optimizer of a train step: every use is an event"""

    def __init__(self, rec):
        self.rec, self.flat_p, self._count = rec, torch.zeros(1), 0

    @property
    def _step(self):
        self.rec.add("opt._step read", self._count)
        return self._count

    @_step.setter
    def _step(self, v):
        self.rec.add("opt._step write", v)
        self._count = v

    def zero_grad(self, set_to_none=False):
        self.rec.add("opt.zero_grad", {"set_to_none": set_to_none})

    def step(self):
        self._count += 1
        self.rec.add("opt.step")

    def device_hyper(self, on):
        self.rec.add("opt.device_hyper", on)

    def advance_captured(self):
        self.rec.add("opt.advance_captured")


class _Graph:
    """what a builder returns: the counts, the flags and tiny tensors at fixed addresses"""
    order = capacity = None

    def __init__(self, rec, k, N, E, n_real=None, pbc=False, static=True, padded=True):
        self.name = "graph#%d" % k
        self.N, self.E, self.n_real = N, E, n_real
        self._padded, self._pbc, self._radius_static = padded, pbc, static
        self.pos, self.z, self.batch = torch.empty(N, 3), torch.empty(N, dtype=torch.int64), torch.empty(N, dtype=torch.int32)
        self.node_mask, self.graph_mask, self.src = torch.empty(N), torch.empty(B + 1), torch.empty(E, dtype=torch.int32)
        self.offsets = torch.empty(E, 3) if pbc else None
        self.cell_offsets = torch.empty(E, 3, dtype=torch.int32) if pbc else None
        rec.name(self.name, vars(self))


class _CudaGraph:
    def __init__(self, rec):
        self.rec, self.name = rec, "cudagraph#%d" % rec.cuda_graphs
        rec.cuda_graphs += 1
        rec.add("CUDAGraph()", self.name)

    def replay(self):
        self.rec.add("replay", self.name)


@contextlib.contextmanager
def _span(rec, what, *args):
    rec.add(what + " enter", *args)
    try:
        yield
    finally:
        rec.add(what + " exit")


@contextlib.contextmanager
def _patched(rec):
    """the replacements of the module docstring, undone on the way out"""
    rec.cuda_graphs = 0
    saved = []

    def put(obj, name, value):
        saved.append((obj, name, vars(obj).get(name, saved)))  # (`saved` itself: the name is inherited, not the object's own)
        setattr(obj, name, value)

    def seed_offset(t):
        rec.name("seed_word", {"": t})
        return _span(rec, "dropout_seed_offset", rec.ref(t))

    def device_draws(seed, base=0):
        return _span(rec, "device_draws", rec.ref(seed), "base drawn lazily" if callable(base) else base)
    put(torch.Tensor, "pin_memory", lambda self: self)
    put(torch.cuda, "CUDAGraph", lambda: _CudaGraph(rec))
    put(torch.cuda, "graph", lambda g: _span(rec, "capture", g.name))
    put(ops._arena, "capture_scope", lambda: _span(rec, "capture_scope"))
    put(ops, "dropout_seed_offset", seed_offset)
    put(droppath, "device_draws", device_draws)
    graphs = []

    def plan_stub(name):
        def plan(pos, *rest):
            p = type("Plan", (), {})()
            p.N, p.E, p.kind = int(pos.shape[0]), rec.next_E, name
            rec.add(name, p.N, p.E)
            return p
        return plan

    def build_stub(name, plan_name):
        def build(plan, capacity=None, into=None, z=None):
            assert plan.kind == plan_name
            rec.add(name, list(capacity), None if into is None else into.name, "z" if z is not None else None)
            g = into
            if g is None:
                g = _Graph(rec, len(graphs), capacity[0], capacity[1], pbc=plan_name != "radius_plan")
                graphs.append(g)
            g.n_real, g.e_real = plan.N, plan.E
            return g
        return build
    for plan_name, build_name in PLANS.items():
        put(EdgeGraph, plan_name, staticmethod(plan_stub(plan_name)))
        put(EdgeGraph, build_name, staticmethod(build_stub(build_name, plan_name)))
    try:
        yield
    finally:
        for obj, name, value in reversed(saved):
            if value is saved:
                delattr(obj, name)
            else:
                setattr(obj, name, value)


def _batch(rec, i, N, mode):
    d = {"pos": torch.ones(N, 3), "z": torch.ones(N, dtype=torch.int64), "batch": torch.zeros(N, dtype=torch.int32), "num_graphs": B,
         "y": torch.ones(B), "dy": torch.ones(N, 3)}
    if mode != "search":
        d["cell"] = torch.ones(B, 3, 3)
    if mode == "batch":
        d.update(edge_index=torch.zeros(2, 3, dtype=torch.int64), cell_offsets=torch.zeros(3, 3, dtype=torch.int64),
                 neighbors=torch.tensor([2, 1]))
    rec.name("batch#%d" % i, d)
    return d


def _raises(rec, f):
    try:
        f()
    except Exception as e:  # noqa: BLE001  (the type and the text are the record)
        rec.add("raised", type(e).__name__, str(e))
    else:
        rec.add("did not raise")


# ------------------------------------------------------------------------------------------------- sequences
def _bucketed(kind, mode):
    """keys A A A A B B B A through a bucketed step with min_eager=2, max_graphs=1, then a batch of the other periodicity"""
    rec = _Recorder()
    weight = torch.ones(1, requires_grad=True)
    weight.register_hook(lambda grad: rec.add("backward"))
    kw = dict(graph_targets=("y",), node_targets=("dy",), min_eager=2, max_graphs=1, node_step=NODE_STEP, edge_step=EDGE_STEP,
              max_num_neighbors=16, edges="batch" if mode == "batch" else "search")

    def forward_loss(g, view):
        rec.add("forward_loss", g.name, sorted(vars(view)))
        return (weight * 2.0).sum()

    def predict(g, view):
        rec.add("predict", g.name, sorted(vars(view)), {"grad": torch.is_grad_enabled()})
        return torch.ones(B + 1, requires_grad=True) * 2.0, torch.ones(g.N, 3, requires_grad=True) * 2.0

    class Meter:
        @staticmethod
        def update(energy, y, n_graphs, forces, dy, node_mask):
            rec.add("meter.update", rec.ref(energy), rec.ref(y), n_graphs, rec.ref(forces), rec.ref(dy), rec.ref(node_mask),
                    {"detached": not (energy.requires_grad or forces.requires_grad)})
    with _patched(rec):
        if kind == "train":
            step = capture.BucketedTrainStep(_Opt(rec), forward_loss, 5.0, drop_path_seed=7, **kw)
            rec.drop_path_word = step._drop_path.dev
            rec.name("drop_path_word", {"": rec.drop_path_word})
        else:
            step = evaluate.BucketedEvalStep(predict, 5.0, Meter, **kw)
        taken = {k: 0 for k in SHAPES}
        for i, key in enumerate(KEYS):
            N, rec.next_E = SHAPES[key][taken[key] % len(SHAPES[key])]
            taken[key] += 1
            rec.add("step", i, key)
            d = _batch(rec, i, N, mode)
            with rec:
                out = step.step(d)
            rec.add("returned", [rec.ref(o) for o in out] if isinstance(out, tuple) else rec.ref(out))
            rec.add("counters", {c: getattr(step, c) for c in COUNTERS}, [list(k) for k in step.live_graphs()],
                    sorted([list(k), v] for k, v in step.captures_of.items()), sorted([list(k), v] for k, v in step._seen.items()))
        rec.add("step", len(KEYS), "the other periodicity")
        other = _batch(rec, len(KEYS), 5, "search" if mode != "search" else "pbc")
        with rec:
            _raises(rec, lambda: step.step(other))
        if mode == "batch":
            rec.add("step", len(KEYS) + 1, "edge fields missing")
            d = _batch(rec, len(KEYS) + 1, 5, mode)
            del d["neighbors"]
            with rec:
                _raises(rec, lambda: step.step(d))
    return rec.resolved()


def _eval_checks():
    """the pre-checks of BucketedEvalStep come before the batch is touched: no plan event between `step` and `raised`"""
    rec = _Recorder()
    model = torch.nn.Linear(1, 1)
    with _patched(rec):
        step = evaluate.BucketedEvalStep(lambda g, v: None, 5.0, model=model, min_eager=2, max_graphs=1)
        rec.next_E = 6
        rec.add("step", 0, "a model in training mode")
        d = _batch(rec, 0, 5, "search")
        with rec:
            _raises(rec, lambda: step.step(d))
        model.eval()
        step.device = torch.device("cuda", 0)
        rec.add("step", 1, "a batch on another device")
        with rec:
            _raises(rec, lambda: step.step(d))
        _raises(rec, lambda: evaluate.BucketedEvalStep(lambda g, v: None, 5.0, device="cpu"))
    return rec.resolved()


def _captured():
    """CapturedTrainStep with min_eager=2, max_graphs=2: S1 S1 S1 S1, S2 (the build returns another graph: the record goes, one
    rebuild attempt), S2 S2, S1, then three times a graph that is not refillable in place"""
    rec = _Recorder()
    weight = torch.ones(1, requires_grad=True)
    weight.register_hook(lambda grad: rec.add("backward"))
    shapes = {"S1": (5, 6), "S2": (5, 8), "sorted": (5, 9)}
    made = []

    def forward_loss(g):
        rec.add("forward_loss", g.name)
        return (weight * 2.0).sum()

    def build_graph(into):
        N, E = shapes[rec.shape]
        static = rec.shape != "sorted"
        rec.add("build_graph", rec.shape, None if into is None else into.name)
        if into is not None and (into.N, into.E) == (N, E) and static:
            return into
        if into is not None:
            into._radius_static = False  # (what the builders do to a graph whose counts they did not find)
        made.append(_Graph(rec, len(made), N, E, static=static, padded=False))
        return made[-1]
    with _patched(rec):
        step = capture.CapturedTrainStep(_Opt(rec), forward_loss, min_eager=2, max_graphs=2, drop_path_seed=7)
        rec.drop_path_word = step._drop_path.dev
        rec.name("drop_path_word", {"": rec.drop_path_word})
        for i, rec.shape in enumerate(["S1"] * 4 + ["S2"] * 3 + ["S1"] + ["sorted"] * 3):
            rec.add("step", i, rec.shape)
            with rec:
                out = step.step(build_graph)
            rec.add("returned", rec.ref(out))
            rec.add("counters", {"replays": step.replays, "eager_steps": step.eager_steps}, [list(k) for k in step._graphs],
                    sorted([list(k), v] for k, v in step._seen.items()))
    return rec.resolved()


SEQUENCES = {"captured train": _captured, "eval pre-checks": _eval_checks}
for _kind in ("train", "eval"):
    for _mode in ("search", "pbc", "batch"):
        SEQUENCES["bucketed %s %s" % (_kind, _mode)] = (lambda k=_kind, m=_mode: _bucketed(k, m))


def trace(name):
    torch.manual_seed(0)
    return SEQUENCES[name]()


def trace_all():
    return {name: trace(name) for name in sorted(SEQUENCES)}


def dump(traces, path):
    """one event per line"""
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join("%s: [\n%s\n]" % (json.dumps(k), ",\n".join(json.dumps(e, sort_keys=True) for e in v))
                                   for k, v in sorted(traces.items())) + "\n}\n")


if __name__ == "__main__":
    dump(trace_all(), sys.argv[1])
