"""Launch and write trace of the graph builders of equiformer_amd/graph.py, taken on CPU tensors in the manner of
tests/ops_trace.py: `graph.call` and `graph._stream` are replaced, every tensor answers `is_cuda` with True while a case runs,
and the builders run on the three sources -- the neighbour search ("radius"), the periodic search ("pbc") and a given periodic
edge list ("edges") -- exact-shape and padded, fresh and into an earlier graph.

What is recorded, in the order in which the builder issues it:
  * every entry point of the C ABI with its scalar arguments as they are and its pointer arguments resolved by ADDRESS to
    [owner.field, byte offset]; the owner is `input` (a tensor of the caller), `into` (the graph handed in), `plan` (where the
    case holds the plan object), `g` (the result) or `fresh#k` (memory none of them keeps, numbered by first appearance);
  * every in-place write and copy the builder issues through torch -- `copy_`, `zero_`, `fill_`, `clone` -- with destination and
    source as [owner.field, byte offset, shape] (a TorchFunctionMode sees them);
  * {"mark": "build"} between the two halves where the case runs them itself, {"raised": [type, text]} where a call raises.
The kernels whose results the host reads back get them from the case: the fake `eqf_segment_ptr` writes the largest molecule,
`eqf_exclusive_scan_i32` the totals in the order of the scans (edges; periodic search: edges, candidates; given edges: sum of
`neighbors`, kept edges) and `eqf_edges_pbc_count` its status word, each through the pointer it was handed; the fill kernels
zero `src` / `dst`, which the device-sort fallback reads.

After each step the result's state is recorded as it READS: `N, E, num_graphs, n_real, e_real, num_real_graphs, capacity`
(None where the graph has none), `_padded, _pbc, _radius_static` (False where it has none), the tensors it owns with shape and
dtype, whether it `is into`, and `into._radius_static` afterwards.

`trace_all()` returns {case: [step record, ...]}; tests/golden/graph_trace.json holds what it returned when each builder still
carried its own copy of the padding and refill code (python tests/graph_trace.py PATH writes such a file)."""
import ctypes
import json
import os
import sys
import types

import torch
from torch.overrides import TorchFunctionMode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from equiformer_amd import graph as graph_module  # noqa: E402
from equiformer_amd.graph import CSR_MAX_NODES, EdgeGraph  # noqa: E402

SOURCES = ("radius", "pbc", "edges")
B, N, E, CAPACITY = 2, 5, 6, (8, 12)  # 6 phantom edges need exactly the 3 phantom nodes the capacity leaves
E_IN = 7                              # given edges: one of the 7 input edges is dropped
R, K = 5.0, 16
NUMBERS = ("N", "E", "num_graphs", "n_real", "e_real", "num_real_graphs", "capacity")
FLAGS = ("_padded", "_pbc", "_radius_static")
WRITES = ("copy_", "zero_", "fill_", "clone")
_STREAM = ctypes.c_void_p(0)
_SRC_DST = {"eqf_radius_graph_fill": (6, 7), "eqf_radius_graph_pbc_fill": (9, 10)}


class _Recorder(TorchFunctionMode):
    """stands in for graph.call and watches the torch calls of the builders while a case runs"""

    def __init__(self):
        super().__init__()
        self.events = []
        self.stores = {}   # base address -> storage (kept alive: no address is handed out twice during a case)
        self.readback = None

    def register(self, t):
        if torch.is_tensor(t) and t.numel():
            stor = t.untyped_storage()
            self.stores.setdefault(stor.data_ptr(), stor)
        elif isinstance(t, (tuple, list)):
            for x in t:
                self.register(x)

    def tensor_ref(self, t):
        self.register(t)
        base = t.untyped_storage().data_ptr()
        return ("ref", base, t.data_ptr() - base, list(t.shape))

    def pointer_ref(self, addr):
        for base, stor in self.stores.items():
            if base <= addr < base + stor.nbytes():
                return ("ref", base, addr - base)
        raise LookupError("address %#x lies in no tensor of the case" % addr)

    def __torch_function__(self, func, types_, args=(), kwargs=None):
        kwargs = kwargs or {}
        name = getattr(func, "__name__", "")
        if name == "__get__" and getattr(func, "__self__", None) is torch.Tensor.is_cuda:
            return True
        for a in args:
            self.register(a)
        out = func(*args, **kwargs)
        self.register(out)
        if name in WRITES and args and torch.is_tensor(args[0]):
            if name == "clone":
                dst, src = out, args[0]
            else:
                dst, src = args[0], (args[1] if len(args) > 1 else None)
            src = self.tensor_ref(src) if torch.is_tensor(src) else src
            self.events.append({"write": name, "dst": self.tensor_ref(dst), "src": src})
        return out

    # ---- graph.call ---------------------------------------------------------------------------------------------------------
    def value(self, a):
        if a is _STREAM:
            return "stream"
        if isinstance(a, ctypes.c_void_p):
            return self.pointer_ref(a.value)
        if a is None or isinstance(a, (int, float)):
            return a
        raise TypeError("unexpected argument %r" % (a,))

    @staticmethod
    def _poke(ptr, v):
        ctypes.c_int32.from_address(ptr.value).value = int(v)

    def call(self, name, *args):
        self.events.append({"call": name, "args": [self.value(a) for a in args]})
        rb = self.readback
        if name == "eqf_segment_ptr":
            self._poke(args[4], rb["largest"])
        elif name == "eqf_exclusive_scan_i32":
            self._poke(args[3], rb["scans"].pop(0))
        elif name == "eqf_edges_pbc_count":
            self._poke(args[14], rb["status"])
        elif name in _SRC_DST:
            for i in _SRC_DST[name]:
                ctypes.memset(args[i].value, 0, 4 * rb["E"])

    # ---- names ----------------------------------------------------------------------------------------------------------------
    def resolved(self, events, owners):
        """events with every ("ref", base, offset[, shape]) written as [owner.field or fresh#k, offset[, shape]]"""
        names, fresh = {}, {}
        for owner, fields in owners:
            for field, t in sorted(fields.items()):
                if torch.is_tensor(t) and t.numel():
                    names.setdefault(t.untyped_storage().data_ptr(), "%s.%s" % (owner, field))

        def res(v):
            if isinstance(v, tuple) and v and v[0] == "ref":
                if v[1] not in names:
                    names[v[1]] = fresh[v[1]] = "fresh#%d" % len(fresh)
                return [names[v[1]]] + list(v[2:])
            if isinstance(v, list):
                return [res(x) for x in v]
            if isinstance(v, dict):
                return {k: res(x) for k, x in v.items()}
            return v
        return [res(e) for e in events]


def _fields(obj):
    if obj is None:
        return {}
    if hasattr(obj, "__slots__"):
        return {k: getattr(obj, k) for k in obj.__slots__ if hasattr(obj, k)}
    return dict(vars(obj))


def _inputs(source, ints=torch.int32, n=N):
    t = types.SimpleNamespace(pos=torch.linspace(0.0, 1.0, 3 * n).view(n, 3), batch=torch.tensor([0, 0, 0, 1, 1][:n], dtype=torch.int32),
                              z=torch.arange(1, n + 1, dtype=torch.int64))
    if source != "radius":
        t.cell = (4.0 * torch.eye(3)).repeat(B, 1, 1)
    if source == "edges":
        t.edge_index = torch.tensor([[1, 2, 0, 2, 4, 3, 3], [0, 0, 1, 1, 3, 4, 3]], dtype=ints).clamp(max=n - 1)
        t.cell_offsets = torch.zeros((E_IN, 3), dtype=ints)
        t.neighbors = torch.tensor([4, 3], dtype=ints)
    return t


def _state(g):
    out = {k: getattr(g, k, None) for k in NUMBERS}
    out.update({k: bool(getattr(g, k, False)) for k in FLAGS})
    out["capacity"] = None if out["capacity"] is None else list(out["capacity"])
    out["tensors"] = {k: [list(v.shape), str(v.dtype)] for k, v in sorted(vars(g).items()) if torch.is_tensor(v)}
    return out


def _step(rec, source, prev, inp, E=E, largest=3, cand=9, nsum=E_IN, status=0, capacity=None, into=False, z=False, via="plan"):
    """one build.  via="call": the one-call form (from_radius / from_radius_pbc / from_edges_pbc); via="plan": the two halves,
    with {"mark": "build"} between them (the search sources have no exact-shape second half: capacity=None runs the one-call
    form whatever `via` says)."""
    rec.readback = {"largest": largest, "status": status, "E": E,
                    "scans": {"radius": [E], "pbc": [E, cand], "edges": [nsum, E]}[source]}
    rec.events = []
    into_g = prev if into else None
    zz = inp.z if z else None
    plan = ret = None
    if capacity is None and source != "edges":
        via = "call"
    try:
        if via == "call":
            if source == "radius":
                ret = EdgeGraph.from_radius(inp.pos, inp.batch, R, K, B, into=into_g, capacity=capacity, z=zz)
            elif source == "pbc":
                ret = EdgeGraph.from_radius_pbc(inp.pos, inp.cell, inp.batch, R, K, B, into=into_g, capacity=capacity, z=zz)
            else:
                ret = EdgeGraph.from_edges_pbc(inp.pos, inp.cell, inp.batch, inp.edge_index, inp.cell_offsets, inp.neighbors, B,
                                               into=into_g, capacity=capacity, z=zz)
        else:
            if source == "radius":
                plan = EdgeGraph.radius_plan(inp.pos, inp.batch, R, K, B)
            elif source == "pbc":
                plan = EdgeGraph.radius_pbc_plan(inp.pos, inp.cell, inp.batch, R, K, B)
            else:
                plan = EdgeGraph.edges_pbc_plan(inp.pos, inp.cell, inp.batch, inp.edge_index, inp.cell_offsets, inp.neighbors, B)
            rec.events.append({"mark": "build"})
            build = {"radius": EdgeGraph.from_radius_plan, "pbc": EdgeGraph.from_radius_pbc_plan,
                     "edges": EdgeGraph.from_edges_pbc_plan}[source]
            ret = build(plan, capacity, into=into_g, z=zz)
    except Exception as e:  # noqa: BLE001  (the type and the text are the record)
        rec.events.append({"raised": [type(e).__name__, str(e)]})
    g = ret[0] if isinstance(ret, tuple) else ret
    owners = [("input", vars(inp)), ("into", _fields(into_g)), ("plan", _fields(plan))]
    if g is not None and g is not into_g:
        owners.append(("g", _fields(g)))
    out = {"events": rec.resolved(rec.events, owners), "is_into": g is not None and g is into_g,
           "result": None if g is None else _state(g),
           "into_static": None if into_g is None else bool(getattr(into_g, "_radius_static", False))}
    if isinstance(ret, tuple):
        out["returns_its_offsets"] = ret[1] is g.offsets and ret[2] is g.cell_offsets
    return out, g


# ------------------------------------------------------------------------------------------------- cases
# A case is a list of steps; a step is the keyword arguments of `_step`, plus "same_inputs" (the tensors of the step before,
# not fresh ones: `batch` then already is the graph's), "n" (nodes: 4 leaves the second structure one atom, and the fourth
# phantom node that 8 phantom edges need) and "ints" (the integer type of a given edge list).  `into=True` hands
# the result of the step before to the builder.
PAD = dict(capacity=CAPACITY)


def _cases():
    cases = {}
    for s in SOURCES:
        c = {
            "1 exact fresh": [dict(via="call")],
            "2 exact into equal counts": [dict(), dict(into=True), dict(into=True, same_inputs=True)],
            "3 exact into another E": [dict(), dict(into=True, E=5)],
            "4 padded fresh with z": [dict(PAD, z=True, via="call")],
            "4 padded fresh without z": [dict(PAD)],
            "5 padded into fewer then more edges": [dict(PAD, z=True), dict(PAD, z=True, into=True, E=4, n=4),
                                                   dict(PAD, z=True, into=True, E=7)],
            "6 padded into z presence differs": [dict(PAD, z=True), dict(PAD, into=True), dict(PAD, z=True, into=True)],
            "7 does not fit E above": [dict(PAD), dict(PAD, into=True, E=13)],
            "7 does not fit N above": [dict(PAD), dict(capacity=(4, 12), into=True)],
            "7 does not fit Q 7 P 3": [dict(PAD), dict(PAD, into=True, E=5)],
            "7 does not fit through the one-call form": [dict(PAD), dict(PAD, into=True, E=13, via="call")],
            "8 largest molecule padded": [dict(PAD, largest=CSR_MAX_NODES + 1)],
            "8 largest molecule exact": [dict(largest=CSR_MAX_NODES + 1), dict(into=True, largest=CSR_MAX_NODES + 1)],
        }
        cases.update({"%s: %s" % (s, k): (s, v) for k, v in c.items()})
    cases.update({
        "edges: 9 int64 input": ("edges", [dict(ints=torch.int64), dict(PAD, ints=torch.int64)]),
        "edges: 9 mixed input": ("edges", [dict(ints=torch.int64, offsets_ints=torch.int32)]),
        "edges: 9 wrong neighbour sum": ("edges", [dict(nsum=E_IN - 1), dict(PAD, nsum=E_IN + 1, via="call")]),
        "edges: 9 status": ("edges", [dict(status=3), dict(PAD, status=1, via="call")]),
        "edges: 1 exact fresh in two halves": ("edges", [dict()]),
    })
    return cases


CASES = _cases()


def trace(case):
    source, steps = CASES[case]
    rec = _Recorder()
    saved = graph_module.call, graph_module._stream
    graph_module.call, graph_module._stream = rec.call, lambda: _STREAM
    out, prev, inp = [], None, None
    try:
        for spec in steps:
            spec = dict(spec)
            ints, off_ints = spec.pop("ints", torch.int32), spec.pop("offsets_ints", None)
            if not spec.pop("same_inputs", False):
                inp = _inputs(source, ints, spec.pop("n", N))
                if off_ints is not None:
                    inp.cell_offsets = inp.cell_offsets.to(off_ints)
                rec.register(list(vars(inp).values()))
            with rec:
                record, g = _step(rec, source, prev, inp, **spec)
            out.append(record)
            prev = g if g is not None else prev
    finally:
        graph_module.call, graph_module._stream = saved
    return out


def trace_all():
    return {case: trace(case) for case in sorted(CASES)}


def dump(traces, path):
    """one case per line: a change shows up as the lines of the cases it touches"""
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in sorted(traces.items()))
                + "\n}\n")


if __name__ == "__main__":
    dump(trace_all(), sys.argv[1])
