"""Descriptor trace of the linear operators of equiformer_amd/ops.py, taken on CPU tensors.

The host logic of `irreps_linear`, `irreps_linear_pair`, `dense_linear` and `grouped_linear` is plain Python: with the device
checks, the stream, the capture query and the C ABI (`ops.call`) replaced, the four PUBLIC operators run on CPU tensors and every
launch they would issue is recorded: the entry point, the chunk of GEMM descriptors behind it (decoded from the ctypes array the
real `_gemm_group` builds, so chunking and the matrix mode are part of the record) and every other call with its arguments.
Device pointers are written as (name of the tensor of the case whose memory they point into, element offset); memory that
belongs to no tensor of the case is "fresh#k", numbered in order of first appearance.

`trace_all()` returns {case: {pass: record}}; tests/golden/linear_trace.json holds what it returned before the operators were
merged into one Function triple (python tests/linear_trace.py PATH writes such a file)."""
import ctypes
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from equiformer_amd import ops  # noqa: E402
from equiformer_amd.layout import RowLayout  # noqa: E402
from equiformer_amd.lib import EqfGemmDesc, EqfRows  # noqa: E402

ROWS = 5
PASSES = ("backward_deferred", "backward_immediate", "grad_params", "backward_twice", "force", "force_create_graph",
          "create_graph", "create_graph_params")


class _Recorder:
    """stands in for ops.call and wraps ops._p while a pass runs"""

    def __init__(self):
        self.events = []
        self.base_of = {}   # address handed to the C ABI -> base address of the storage it lies in
        self.keep = []      # storages stay alive: no address is handed out twice during a pass
        self._p = ops._p

    def p(self, t, off=0):
        if t is not None:
            stor = t.untyped_storage()
            self.keep.append(stor)
            self.base_of[t.data_ptr() + 4 * off] = stor.data_ptr()
        return self._p(t, off)

    def ref(self, addr):
        if addr is None:
            return None
        return (self.base_of[addr], addr)

    def value(self, a):
        if isinstance(a, ctypes.c_void_p):
            return self.ref(a.value)
        if isinstance(a, EqfRows):
            return [a.d, a.ld, a.inner]
        if a is None or isinstance(a, (int, float)):
            return a
        raise TypeError("unexpected argument %r" % (a,))

    def call(self, name, *args):
        if name in ("eqf_gemm_group", "eqf_gemmx_group"):
            arr, n = args[0], args[1]
            assert len(arr) == n
            descs = []
            for i in range(n):
                d = arr[i]
                assert isinstance(d, EqfGemmDesc)
                descs.append({"kind": d.kind, "M": d.M, "N": d.N, "K": d.K, "ldb": d.ldb, "accumulate": d.accumulate,
                              "ra": [d.ra.d, d.ra.ld, d.ra.inner], "rc": [d.rc.d, d.rc.ld, d.rc.inner],
                              "A": self.ref(d.A), "B": self.ref(d.B), "C": self.ref(d.C), "bias": self.ref(d.bias)})
            self.events.append({"call": name, "args": [self.value(a) for a in args[2:]], "descs": descs})
        else:
            self.events.append({"call": name, "args": [self.value(a) for a in args]})

    def resolved(self, named):
        """events with every (storage, address) written as [tensor name or fresh#k, element offset]"""
        names, fresh = {0: "null"}, {}
        for name, t in named:
            if t is not None:
                names.setdefault(t.untyped_storage().data_ptr(), name)

        def res(v):
            if isinstance(v, tuple):
                base, addr = v
                if base not in names:
                    names[base] = fresh[base] = "fresh#%d" % len(fresh)
                assert (addr - base) % 4 == 0
                return [names[base], (addr - base) // 4]
            return v

        out = []
        for e in self.events:
            e = dict(e, args=[res(a) for a in e["args"]])
            if "descs" in e:
                e["descs"] = [{k: res(v) for k, v in d.items()} for d in e["descs"]]
            out.append(e)
        return out


def _rand(*shape, grad=False):
    return torch.randn(*shape).requires_grad_(grad)


# ------------------------------------------------------------------------------------------------- cases
# A case is a function that returns (named, x_leaf, params, run): the named tensors of the case, the leaf behind the operator's
# input, the trainable parameters, and run() -> (outputs, was_tuple, output gradients with None for "no gradient arrives").
def _per_degree(irr_in, irr_out, bias=True, frozen_w=False, nonleaf_bias=False, n=ROWS):
    def make():
        li = irr_in if not isinstance(irr_in, str) else RowLayout(irr_in)
        spec = ops.LinearSpec(li, RowLayout(irr_out))
        x = _rand(n, li.dim, grad=True)
        w = _rand(spec.weight_numel, grad=not frozen_w)
        named, params, b = [("x", x), ("w", w)], ([] if frozen_w else [w]), None
        if bias:
            if nonleaf_bias:  # what LinearRS._bias() hands over: an element of a parameter list / a row of a parameter
                b_raw = _rand(1, spec.bias_dim, grad=True)
                named.append(("b_raw", b_raw))
                params.append(b_raw)
            else:
                b = _rand(spec.bias_dim, grad=True)
                named.append(("b", b))
                params.append(b)

        def run():
            y = ops.irreps_linear(x, w, b_raw[0] if (bias and nonleaf_bias) else b, spec)
            return [y], False, [_rand(*y.shape)]
        return named, x, params, run
    return make


_UNSIMPLIFIED = types.SimpleNamespace(segs=[(4, 0), (4, 0), (4, 1)], par=[1, 1, 1], offsets=[0, 4, 8], dim=20)


def _pair(none_second=False, bias_second=True):
    def make():
        li = RowLayout("8x0e+4x1e+4x2e")
        s1, s2 = ops.LinearSpec(li, RowLayout("8x0e+4x1e+4x2e")), ops.LinearSpec(li, RowLayout("8x0e+4x1e"))
        x = _rand(ROWS, li.dim, grad=True)
        w1, w2 = _rand(s1.weight_numel, grad=True), _rand(s2.weight_numel, grad=True)
        b1 = _rand(s1.bias_dim, grad=True)
        b2 = _rand(s2.bias_dim, grad=True) if bias_second else None
        named = [("x", x), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2)]

        def run():
            out = ops.irreps_linear_pair(x, w1, b1, s1, w2, b2, s2)
            ys = list(out)
            return ys, isinstance(out, tuple), [_rand(*ys[0].shape), None if none_second else _rand(*ys[1].shape)]
        return named, x, [p for p in (w1, b1, w2, b2) if p is not None], run
    return make


def _dense(block=None, bias=True, frozen_w=False):
    def make():
        K, N = 8, 12
        W = _rand(N, K, grad=not frozen_w)
        b = _rand(N, grad=True) if bias else None
        if block is None:
            x_leaf = _rand(ROWS, K, grad=True)
            named = [("x", x_leaf)]
        else:  # x is the column block [4, 4 + K) of a [ROWS, block] tensor
            x_leaf = _rand(ROWS, block, grad=True)
            named = [("x_wide", x_leaf)]
        named += [("W", W), ("b", b)]

        def run():
            x = x_leaf if block is None else x_leaf[:, 4:4 + K]
            y = ops.dense_linear(x, W, b)
            return [y], False, [_rand(*y.shape)]
        return named, x_leaf, [p for p in (None if frozen_w else W, b) if p is not None], run
    return make


def _grouped(wide, Ns, has_b, none_dy=()):
    def make():
        K, G = 4, len(Ns)
        x = _rand(ROWS, G * K, grad=True)
        Ws = [_rand(n, K, grad=True) for n in Ns]
        bs = [(_rand(n, grad=True) if hb else None) for n, hb in zip(Ns, has_b)]
        named = [("x", x)] + [("W%d" % g, W) for g, W in enumerate(Ws)] + [("b%d" % g, b) for g, b in enumerate(bs)]

        def run():
            out = ops.grouped_linear(x, K, Ws, bs, wide)
            ys = list(out) if isinstance(out, tuple) else [out]
            return ys, isinstance(out, tuple), [None if g in none_dy else _rand(*y.shape) for g, y in enumerate(ys)]
        return named, x, Ws + [b for b in bs if b is not None], run
    return make


_FULL = "8x0e+4x1e+4x2e"
CASES = {
    "per_degree_bias": _per_degree(_FULL, _FULL),
    "per_degree_no_bias": _per_degree(_FULL, _FULL, bias=False),
    "per_degree_unsimplified_input": _per_degree(_UNSIMPLIFIED, "8x0e+4x1e"),
    "per_degree_uncovered_output": _per_degree("8x0e+4x1e", _FULL),
    "per_degree_uncovered_input": _per_degree(_FULL, "8x0e+4x1e"),
    "per_degree_e3": _per_degree("8x0e+4x0o+4x1e+4x1o", "8x0e+4x0o+4x1e+4x1o"),
    "per_degree_frozen_weight": _per_degree(_FULL, _FULL, frozen_w=True),
    "per_degree_nonleaf_bias": _per_degree(_FULL, _FULL, nonleaf_bias=True),
    "per_degree_no_rows": _per_degree(_FULL, _FULL, n=0),
    "pair_both": _pair(),
    "pair_one_none": _pair(none_second=True),
    "pair_bias_one_side": _pair(bias_second=False),
    "dense_contiguous": _dense(),
    "dense_block_in_place": _dense(block=16),
    "dense_block_copied": _dense(block=15),
    "dense_no_bias": _dense(bias=False),
    "dense_frozen_weight": _dense(frozen_w=True),
    "grouped_wide": _grouped(True, [8, 8, 8], [True, True, True]),
    "grouped_separate": _grouped(False, [8, 4, 12], [True, False, True], none_dy=(1,)),
}
FP32_CASES = ("per_degree_bias", "pair_both", "dense_contiguous", "grouped_wide")  # once more in the matrix mode fp32


# ------------------------------------------------------------------------------------------------- passes
def _one_pass(make, which):
    torch.manual_seed(0)
    named, x_leaf, params, run = make()
    named = list(named)
    shapes = {}

    def note(name, t):
        named.append((name, t))
        shapes[name] = None if t is None else [list(t.shape), list(t.stride())]

    def forward(tag=""):
        ys, was_tuple, dys = run()
        if which.startswith("create_graph"):
            dys = [None if d is None else d.requires_grad_(True) for d in dys]
        for i, (y, d) in enumerate(zip(ys, dys)):
            note("y%d%s" % (i, tag), y)
            note("dy%d%s" % (i, tag), d)
        shapes["outputs_are_a_tuple"] = was_tuple
        roots = [y for y, d in zip(ys, dys) if d is not None]
        return roots, [d for d in dys if d is not None]

    def note_grads(tag=""):
        note("x.grad" + tag, x_leaf.grad)
        for name, t in list(named):
            if any(t is p for p in params):
                note(name + ".grad" + tag, t.grad)

    def pnames():
        return [name for p in params for name, t in named if t is p]

    if which in ("backward_deferred", "backward_immediate", "backward_twice"):
        roots, dys = forward()
        torch.autograd.backward(roots, dys)
        note_grads()
        if which == "backward_twice":
            roots, dys = forward("'")
            torch.autograd.backward(roots, dys)
            note_grads("'")
    elif which == "grad_params":
        roots, dys = forward()
        if params:
            for name, g in zip(pnames(), torch.autograd.grad(roots, params, dys, allow_unused=True)):
                note("d" + name, g)
    elif which in ("force", "force_create_graph"):
        roots, dys = forward()
        with ops.input_grads_only():
            (g,) = torch.autograd.grad(roots, [x_leaf], dys, create_graph=which == "force_create_graph")
        note("dx", g)
    else:
        roots, dys = forward()
        wrt = [x_leaf] + (params if which == "create_graph_params" else [])
        gs = torch.autograd.grad(roots, wrt, dys, create_graph=True, allow_unused=True)
        second, cots = [], []
        for name, g in zip(["x"] + pnames(), gs):
            note("d" + name, g)
            if g is not None and g.requires_grad:
                c = _rand(*g.shape)
                note("c_d" + name, c)
                second.append(g)
                cots.append(c)
        torch.autograd.backward(second, cots)
        note_grads()
        for i, d in enumerate(dys):
            note("dy%d.grad" % i, d.grad)
    return named, shapes


def trace(case, which, mode="split"):
    """{"events": [...], "tensors": {name: [shape, stride] or None}} of one case under one kind of pass"""
    rec = _Recorder()
    saved = {k: getattr(ops, k) for k in ("_chk", "_stream", "_capturing", "call", "_p")}
    prev_defer = ops.set_deferred_weight_gradients(which != "backward_immediate")
    prev_mode = ops.set_matrix_mode(mode)
    ops._chk = lambda *ts: None
    ops._stream = lambda: None
    ops._capturing = lambda: False
    ops.call = rec.call
    ops._p = rec.p
    try:
        named, shapes = _one_pass(CASES[case], which)
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        ops.set_deferred_weight_gradients(prev_defer)
        ops.set_matrix_mode(prev_mode)
    return {"events": rec.resolved(named), "tensors": shapes}


def trace_all():
    out = {}
    for case in CASES:
        out[case] = {which: trace(case, which) for which in PASSES}
    for case in FP32_CASES:
        out[case + "@fp32"] = {which: trace(case, which, "fp32") for which in PASSES}
    return json.loads(json.dumps(out))  # (plain lists, as the recorded file holds them)


# ------------------------------------------------------------------------------------------------- the recorded file
# Most launches recur from pass to pass, so the file holds every distinct descriptor, event and tensor table once, one per line,
# and a trace as indices into them.
_DESC_KEYS = ("kind", "M", "N", "K", "ldb", "accumulate", "ra", "rc", "A", "B", "C", "bias")


def _index(table, item):
    key = json.dumps(item, sort_keys=True)
    return table.setdefault(key, len(table))


def pack(traces):
    descs, events, tensors, out = {}, {}, {}, {}
    for case in sorted(traces):
        out[case] = {}
        for which in PASSES:
            rec = traces[case][which]
            ev = [_index(events, [e["call"], e["args"]] + ([[_index(descs, [d[k] for k in _DESC_KEYS]) for d in e["descs"]]]
                                                           if "descs" in e else [])) for e in rec["events"]]
            out[case][which] = [_index(tensors, rec["tensors"]), ev]
    return {"descs": [json.loads(k) for k in descs], "events": [json.loads(k) for k in events],
            "tensors": [json.loads(k) for k in tensors], "traces": out}


def unpack(packed):
    descs = [dict(zip(_DESC_KEYS, d)) for d in packed["descs"]]
    events = [dict({"call": e[0], "args": e[1]}, **({"descs": [descs[i] for i in e[2]]} if len(e) > 2 else {}))
              for e in packed["events"]]
    return {case: {which: {"events": [events[i] for i in ev], "tensors": packed["tensors"][t]}
                   for which, (t, ev) in passes.items()} for case, passes in packed["traces"].items()}


def dump(packed, f):
    def line(x):
        return json.dumps(x, sort_keys=True, separators=(",", ":"))
    f.write("{")
    for key in ("descs", "events", "tensors"):
        f.write('"%s":[\n%s\n],\n' % (key, ",\n".join(line(x) for x in packed[key])))
    rows = ['"%s":{\n%s\n}' % (case, ",\n".join('"%s":%s' % (w, line(packed["traces"][case][w])) for w in PASSES))
            for case in sorted(packed["traces"])]
    f.write('"traces":{\n%s\n}}\n' % ",\n".join(rows))


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        dump(pack(trace_all()), f)
