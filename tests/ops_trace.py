"""Launch trace of every public operator of equiformer_amd/ops.py but the four linears (tests/linear_trace.py holds those),
taken on CPU tensors in the manner of that file: device checks, stream, capture query and the C ABI are replaced, the operators
run forward, backward and double backward, and every call they would issue is recorded with its arguments.

What the linear trace does not meet is named here too:
  * a raw device pointer (`ctypes.c_void_p(t.data_ptr())`: bf16 planes, the graph-norm workspace, byte masks, the metric
    accumulator) and the entries of a `c_void_p * 8` pointer array are found by ADDRESS among the storages of the pass -- the
    tensors of the case, everything handed to `ops._p` and everything `ops` allocates (its `torch` is wrapped for the pass) --
    and written as [name, offset]; the offset counts 4-byte elements, or bytes ([name, n, "B"]) where the elements are not 4 wide;
  * `EqfLnWgradDesc` arrays are decoded field by field;
  * structs (`EqfGateIn`, the `c_ref` irreps / path / edge-degree tables) are recorded by content;
  * `SfcSpec.x_mask` / `SfcSpec.packed_numel` are replaced for the pass (the case chooses the mask), so the split-precision
    branches run without the shared library;
  * a pass that raises (double backward of a first-order operator, a guarded gradient) ends with the event
    {"call": "raised", "args": [type]}.

`trace_all()` returns {case: {pass: record}}; tests/golden/ops_trace.json holds what it returned before the launch sequences
of ops.py were gathered into one helper per kernel (python tests/ops_trace.py PATH writes such a file)."""
import ctypes
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from equiformer_amd import lib, ops  # noqa: E402
from equiformer_amd.layout import DtpTable, RowLayout  # noqa: E402
from linear_trace import PASSES, _Recorder, _index  # noqa: E402

_BYREF = type(ctypes.byref(ctypes.c_int()))


def _struct(s):
    """a ctypes struct by content (trailing zeros of its arrays dropped)"""
    out = {"struct": type(s).__name__}
    for name, _ in s._fields_:
        v = getattr(s, name)
        if isinstance(v, ctypes.Array):
            v = list(v)
            while v and v[-1] == 0:
                v.pop()
        out[name] = v
    return out


class _OpsRecorder(_Recorder):
    def __init__(self):
        super().__init__()
        self.stores = {}  # base address -> (bytes, element size)

    def register(self, t):
        if t is not None and t.numel():
            stor = t.untyped_storage()
            self.keep.append(stor)
            self.stores.setdefault(stor.data_ptr(), (stor.nbytes(), t.element_size()))
        return t

    def p(self, t, off=0):
        self.register(t)
        return self._p(t, off)

    def ref(self, addr):
        if not addr:
            return None
        for base, (nbytes, _) in self.stores.items():
            if base <= addr < base + nbytes:
                return (base, addr)
        raise LookupError("address %#x lies in no tensor of the pass" % addr)

    def value(self, a):
        if isinstance(a, _BYREF):
            return _struct(a._obj)
        if isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p:
            return {"ptrs": [self.ref(v) for v in a]}
        if isinstance(a, ctypes.Array) and a._type_ is lib.EqfLnWgradDesc:
            return {"ln_descs": [{"x": self.ref(d.x), "dy": self.ref(d.dy), "rstd": self.ref(d.rstd), "mean0": self.ref(d.mean0),
                                  "d_weight": self.ref(d.d_weight), "d_bias": self.ref(d.d_bias), "rows": d.rows,
                                  "irreps": _struct(d.irreps.contents)} for d in a]}
        return super().value(a)

    def resolved(self, named):
        names, fresh = {}, {}
        for name, t in named:
            if t is not None and t.numel():
                names.setdefault(t.untyped_storage().data_ptr(), name)

        def res(v):
            if isinstance(v, tuple):
                base, addr = v
                if base not in names:
                    names[base] = fresh[base] = "fresh#%d" % len(fresh)
                size = self.stores[base][1]
                if size == 4:
                    assert (addr - base) % 4 == 0
                    return [names[base], (addr - base) // 4]
                return [names[base], addr - base, "B"]
            if isinstance(v, list):
                return [res(x) for x in v]
            if isinstance(v, dict):
                return {k: res(x) for k, x in v.items()}
            return v
        return [res(e) for e in self.events]


class _TorchOfThePass:
    """`torch` as ops.py sees it during a pass: what the module allocates is known to the recorder by address"""

    def __init__(self, rec):
        for name in ("empty", "empty_like", "zeros", "zeros_like"):
            setattr(self, name, lambda *a, _f=getattr(torch, name), **k: rec.register(_f(*a, **k)))

    def __getattr__(self, name):
        return getattr(torch, name)


class _OnDevice(torch.Tensor):
    """a CPU tensor that answers is_cuda with True: the few host checks that ask the tensor itself (masks, tags, the metric
    accumulator), not ops._chk"""
    is_cuda = property(lambda self: True)


def _dev(t):
    return t.as_subclass(_OnDevice)


def _rand(*shape, grad=False):
    return torch.randn(shape).requires_grad_(grad)


def _i32(*v):
    return torch.tensor(v, dtype=torch.int32)


# ------------------------------------------------------------------------------------------------- cases
# A case is (make, options).  make() returns (named, x_leaf, params, run) as in linear_trace.py: the named tensors, the leaf
# behind the operator's first differentiable input (None: no gradient at all), the other leaves that take a gradient, and
# run() -> (outputs, was_tuple, output gradients with None for "no gradient arrives").  options: the matrix mode and the
# x_mask of the fused SeparableFCTP.
N, E = 3, 5  # nodes, edges (= rows of the edge operators)
_LN = "8x0e+4x1e"


def _graph():
    g = types.SimpleNamespace(N=N, E=E, num_graphs=2, src=_i32(1, 2, 0, 2, 0), dst=_i32(0, 0, 1, 1, 2), row_ptr=_i32(0, 2, 4, 5),
                              src_ptr=_i32(0, 2, 3, 5), src_perm=_i32(2, 4, 0, 1, 3), batch=_i32(0, 0, 1), mol_ptr=_i32(0, 2, 3))
    return g, [("g." + k, v) for k, v in vars(g).items() if torch.is_tensor(v)]


def _op(build):
    """build() -> (dict of named tensors, names of the differentiable leaves (first = x), f() -> outputs, pattern of dys or None)"""
    def make():
        tensors, leaves, f, pattern = build()
        named = list(tensors.items())

        def run():
            out = f()
            ys = list(out) if isinstance(out, tuple) else [out]
            pat = pattern if pattern is not None else [True] * len(ys)
            return ys, isinstance(out, tuple), [_rand(*y.shape) if (keep and y.dtype == torch.float32) else None
                                                for y, keep in zip(ys, pat)]
        x = tensors[leaves[0]] if leaves else None
        return named, x, [tensors[k] for k in leaves[1:]], run
    return make


def _layer_norm(add=False, pattern=None):
    def build():
        lay = RowLayout(_LN)
        t = {"x": _rand(E, lay.dim, grad=True), "w": _rand(12, grad=True), "b": _rand(8, grad=True)}
        if add:
            t["r"] = _rand(E, lay.dim, grad=True)
            return t, ["x", "r", "w", "b"], lambda: ops.add_layer_norm(t["x"], t["r"], t["w"], t["b"], lay), pattern
        return t, ["x", "w", "b"], lambda: ops.layer_norm(t["x"], t["w"], t["b"], lay), None
    return _op(build)


def _graph_norm(add=False, shift=True, pattern=None):
    def build():
        lay = RowLayout(_LN)
        g, gt = _graph()
        t = {"x": _rand(N, lay.dim, grad=True), "w": _rand(12, grad=True), "b": _rand(8, grad=True)}
        leaves = ["x", "w", "b"]
        if shift:
            t["ms"] = _rand(8, grad=True)
            leaves.append("ms")
        t.update(gt)
        if add:
            t["r"] = _rand(N, lay.dim, grad=True)
            return t, leaves + ["r"], lambda: ops.add_graph_norm(t["x"], t["r"], t.get("ms"), t["w"], t["b"], lay, g), pattern
        return t, leaves, lambda: ops.graph_norm(t["x"], t.get("ms"), t["w"], t["b"], lay, g), None
    return _op(build)


def _gate():
    def build():
        lay = RowLayout("4x1e")
        t = {"x": _rand(E, 8 + 4 + lay.dim, grad=True)}
        return t, ["x"], lambda: ops.gate(t["x"], 8, lay, 1.5, 0.5), None
    return _op(build)


def _silu():
    def build():
        t = {"x": _rand(E, 8, grad=True)}
        return t, ["x"], lambda: ops.scaled_silu(t["x"], 1.5), None
    return _op(build)


def _ln_silu(groups):
    def build():
        t = {"x": _rand(E, 8, grad=True), "gamma": _rand(8, grad=True), "beta": _rand(8, grad=True)}
        return t, ["x", "gamma", "beta"], lambda: ops.ln_silu(t["x"], t["gamma"], t["beta"], 1e-5, groups), None
    return _op(build)


def _fold_weight():
    def build():
        t = {"W": _rand(12, grad=True), "w": _rand(2, grad=True), "row_start": _i32(0, 4, 8, 12), "w_of_row": _i32(0, 1, 0)}
        return t, ["W", "w"], lambda: ops.fold_weight(t["W"], t["w"], t["row_start"], t["w_of_row"]), None
    return _op(build)


def _embed(bias=True):
    def build():
        t = {"types": _i32(0, 2, 1, 1, 0), "W": _rand(3, 4, grad=True), "b": _rand(4, grad=True) if bias else None}
        return t, ["W"] + (["b"] if bias else []), lambda: ops.embed(t["types"], t["W"], t["b"], 8), None
    return _op(build)


def _edgedeg_spec():
    table = DtpTable("4x0e", "1x0e+1x1e", "4x0e+4x1e")
    return ops.EdgeDegSpec(table, ops.LinearSpec(table.layout_out, RowLayout("4x0e+4x1e")), 4)


def _edgedeg_fold(expb=True, pattern=None):
    def build():
        spec = _edgedeg_spec()
        c = spec.c
        t = {"W3": _rand(c.w_numel, c.H, grad=True), "offset": _rand(c.w_numel, grad=True), "expw": _rand(c.C, grad=True),
             "expb": _rand(c.C, grad=True) if expb else None, "W": _rand(c.pw_numel, grad=True)}
        leaves = ["W3", "offset", "expw", "W"] + (["expb"] if expb else [])
        return t, leaves, lambda: ops.edgedeg_fold(t["W3"], t["offset"], t["expw"], t["expb"], t["W"], spec), pattern
    return _op(build)


def _edgedeg_scatter(bias=True):
    def build():
        spec = _edgedeg_spec()
        g, gt = _graph()
        t = {"z": _rand(E, spec.c.Z, grad=True), "coupling": _rand(E, spec.c.m_numel),
             "bias": _rand(spec.blocks[0]["N"], grad=True) if bias else None}
        t.update(gt)
        return t, ["z"] + (["bias"] if bias else []), lambda: ops.edgedeg_scatter(t["z"], t["coupling"], t["bias"], g, spec, 0.5), None
    return _op(build)


def _gather_add(b=True, b_grad=True):
    def build():
        g, gt = _graph()
        t = {"a": _rand(N, 8, grad=True), "b": _rand(N, 8, grad=b_grad) if b else None}
        t.update(gt)
        return t, ["a"] + (["b"] if b and b_grad else []), lambda: ops.gather_add(t["a"], t["b"], g), None
    return _op(build)


def _segment(scale_op=False):
    def build():
        t = {"x": _rand(E, 8, grad=True), "ptr": _i32(0, 2, 5), "seg_of": _i32(0, 0, 1, 1, 1), "s": _rand(2)}
        if scale_op:
            return t, ["x"], lambda: ops.segment_scale(t["x"], t["s"], t["seg_of"]), None
        return t, ["x"], lambda: ops.segment_sum(t["x"], t["ptr"], t["seg_of"], 2, 0.5), None
    return _op(build)


def _edge_geometry(offsets, pattern=None):
    def build():
        g, gt = _graph()
        t = {"pos": _rand(N, 3, grad=True), "offsets": _rand(E, 3) if offsets else None}
        t.update(gt)
        return t, ["pos"], lambda: ops.edge_geometry(t["pos"], t["offsets"], g, 1), pattern or [False, True, True]
    return _op(build)


def _vec_sh(keep):
    def build():
        t = {"vec": _rand(E, 3), "keep": _dev(torch.tensor([1, 0, 1, 1, 0], dtype=torch.uint8)) if keep else None}
        return t, [], lambda: ops.vec_sh(t["vec"], t["keep"], 1, 0.5), [False]
    return _op(build)


def _rbf(kind, length_grad=True):
    def build():
        t = {"length": _rand(E, grad=length_grad)}
        first = ["length"] if length_grad else []
        if kind == "gaussian":
            t.update(mean=_rand(4, grad=True), std=_rand(4, grad=True), weight=_rand(1, grad=True), bias=_rand(1, grad=True))
            return t, first + ["mean", "std", "weight", "bias"], \
                lambda: ops.rbf_gaussian(t["length"], t["mean"], t["std"], t["weight"], t["bias"], 5.0), None
        if kind == "expnorm":
            t.update(means=_rand(4), betas=_rand(4))
            return t, first, lambda: ops.rbf_expnorm(t["length"], t["means"], t["betas"], 1.0, 5.0), None
        t.update(freq=_rand(4, grad=True))
        return t, first + ["freq"], lambda: ops.rbf_bessel(t["length"], t["freq"], 5.0), None
    return _op(build)


def _table(mul):
    irr = "%dx0e+%dx1e" % (mul, mul)
    return DtpTable(irr, "1x0e+1x1e", irr), irr


def _coupling():
    def build():
        table, _ = _table(4)
        t = {"sh": _rand(E, 4, grad=True), "cg": table.cg(torch.device("cpu"))}
        return t, ["sh"], lambda: ops.dtp_coupling(t["sh"], table), None
    return _op(build)


def _dtp_inputs(table, w, rows):
    t = {"x": _rand(rows, table.layout_in.dim, grad=True), "coupling": _rand(rows, table.m_numel, grad=True),
         "w": _rand(rows, table.weight_numel, grad=True) if w else None}
    return t, ["x", "coupling"] + (["w"] if w else [])


def _dtp(w):
    def build():
        table, _ = _table(4)
        t, leaves = _dtp_inputs(table, w, E)
        return t, leaves, lambda: ops.dtp(t["x"], t["coupling"], t["w"], table), None
    return _op(build)


def _dtp_linear(w=True, bias=True):
    def build():
        table, irr = _table(32)
        spec = ops.DtpLinearSpec.make(table, RowLayout(irr))
        t, leaves = _dtp_inputs(table, w, N)
        t.update(weight=_rand(spec.weight_numel, grad=True), bias=_rand(spec.bias_dim, grad=True) if bias else None)
        return t, leaves + ["weight"] + (["bias"] if bias else []), \
            lambda: ops.dtp_linear(t["x"], t["coupling"], t["w"], t["weight"], t["bias"], spec), None
    return _op(build)


def _sep_fctp(n2=32, bias=True, bias2=True, w=True, frozen=False, pattern=None):
    def build():
        table, irr = _table(32)
        spec = ops.SfcSpec(table, RowLayout(irr), n2)
        assert spec.supported
        t, leaves = _dtp_inputs(table, w, N)
        t.update(weight=_rand(spec.weight_numel, grad=not frozen), bias=_rand(32, grad=True) if bias else None,
                 weight2=_rand(spec.weight2_numel, grad=not frozen) if n2 else None,
                 bias2=_rand(n2, grad=True) if (n2 and bias2) else None)
        leaves += [k for k in ("weight", "bias", "weight2", "bias2") if t[k] is not None and t[k].requires_grad]
        return t, leaves, lambda: ops.sep_fctp(t["x"], t["coupling"], t["w"], t["weight"], t["bias"], spec, t["weight2"],
                                               t["bias2"]), pattern
    return _op(build)


def _sep_fctp_gated(bias=True, w=True, frozen=False):
    def build():
        table, irr = _table(32)
        spec = ops.SfcSpec(table, RowLayout(irr))
        gated = RowLayout("32x1e")
        t = {"x_raw": _rand(N, 32 + 32 + gated.dim, grad=True), "coupling": _rand(N, table.m_numel, grad=True),
             "w": _rand(N, table.weight_numel, grad=True) if w else None, "weight": _rand(spec.weight_numel, grad=not frozen),
             "bias": _rand(32, grad=True) if bias else None}
        leaves = ["x_raw", "coupling"] + [k for k in ("w", "weight", "bias") if t[k] is not None and t[k].requires_grad]
        return t, leaves, lambda: ops.sep_fctp_gated(t["x_raw"], t["coupling"], t["w"], t["weight"], t["bias"], spec,
                                                     (32, gated, 1.5, 0.5)), None
    return _op(build)


def _alpha():
    def build():
        t = {"a": _rand(E, 8, grad=True), "alpha_dot": _rand(2, 4, grad=True)}
        return t, ["a", "alpha_dot"], lambda: ops.alpha_logits(t["a"], t["alpha_dot"], 2, 4, 0.5), None
    return _op(build)


def _attn(drop_p=0.0, seed_offset=False):
    def build():
        lay = RowLayout(_LN)
        g, gt = _graph()
        t = {"logit": _rand(E, 2, grad=True), "value": _rand(E, lay.dim, grad=True),
             "seed_off": torch.zeros(1, dtype=torch.int64) if seed_offset else None}
        t.update(gt)

        def f():
            with ops.dropout_seed_offset(t["seed_off"]):
                return ops.attn_aggregate(t["logit"], t["value"], g, 2, lay, drop_p, 7)
        return t, ["logit", "value"], f, None
    return _op(build)


def _kv_split(pattern=None):
    def build():
        lay = RowLayout(_LN)
        t = {"kv": _rand(E, 2 * lay.dim, grad=True)}
        return t, ["kv"], lambda: ops.kv_split(t["kv"], 2, lay), pattern
    return _op(build)


def _dp_logits(k_grad=True):
    def build():
        lay = RowLayout(_LN)
        g, gt = _graph()
        t = {"q": _rand(N, lay.dim, grad=True), "k": _rand(E, lay.dim, grad=k_grad)}
        t.update(gt)
        return t, ["q"] + (["k"] if k_grad else []), lambda: ops.dp_logits(t["q"], t["k"], g, 2, lay), None
    return _op(build)


def _dens_corrupt(ratio=None):
    def build():
        t = {"pos": _rand(N, 3), "dy": _rand(N, 3), "batch": _i32(0, 0, 1)}
        return t, [], lambda: ops.dens_corrupt(t["pos"], t["dy"], t["batch"], 0.1, 0.5, ratio, seed=3), [False] * 5
    return _op(build)


def _dens_loss(extras=False):
    def build():
        t = {"pred_y": _rand(2, grad=True), "pred_dy": _rand(N, 3, grad=True), "y": _rand(2), "dy": _rand(N, 3),
             "noise_vec": _rand(N, 3), "noise_mask": _dev(torch.tensor([True, False, True])), "weights": _rand(3),
             "row_mask": torch.ones(N) if extras else None, "stats": torch.zeros(8) if extras else None}
        return t, ["pred_y", "pred_dy"], lambda: ops.dens_loss(t["pred_y"], t["pred_dy"], t["y"], t["dy"], t["noise_vec"],
                                                                t["noise_mask"], t["weights"], 0.5, 2.0, 0.1, t["row_mask"],
                                                                t["stats"]), None
    return _op(build)


def _is2rs_perturb(int64):
    def build():
        t = {"pos": _rand(N, 3), "pos_relaxed": _rand(N, 3), "batch": _i32(0, 0, 1),
             "tags": _dev(torch.tensor([0, 1, 2], dtype=torch.int64 if int64 else torch.int32))}
        return t, [], lambda: ops.is2rs_perturb(t["pos"], t["pos_relaxed"], t["tags"], t["batch"], seed=3), [False] * 4
    return _op(build)


def _is2rs_loss(extras=False):
    def build():
        t = {"pred_y": _rand(2, grad=True), "pred_pos_wide": _rand(N, 4, grad=True), "y": _rand(2), "pos": _rand(N, 3),
             "pos_relaxed": _rand(N, 3), "tags": _dev(torch.tensor([0, 1, 2], dtype=torch.int64 if extras else torch.int32)),
             "weights": _rand(2), "row_mask": torch.ones(N) if extras else None, "stats": torch.zeros(8) if extras else None}
        return t, ["pred_y", "pred_pos_wide"], \
            lambda: ops.is2rs_loss(t["pred_y"], t["pred_pos_wide"][:, 1:], t["y"], t["pos"], t["pos_relaxed"], t["tags"],
                                   t["weights"], 0.5, 2.0, 0.0, (1.0, 2.0, 3.0) if extras else 1.5, 0.02, t["row_mask"],
                                   t["stats"]), None
    return _op(build)


def _metrics(forces):
    def build():
        t = {"acc": _dev(torch.zeros(ops.METRICS_SUMS, dtype=torch.float64)), "pred_y": _rand(4), "y": _rand(4),
             "pred_dy": _rand(N, 3) if forces else None, "dy": _rand(N, 3) if forces else None,
             "node_mask": torch.ones(N) if forces else None}

        def f():
            ops.metrics_accumulate(t["acc"], t["pred_y"], t["y"], 2, 0.5, 2.0, 0.02, t["pred_dy"], t["dy"], t["node_mask"])
            return t["acc"]
        return t, [], f, [False]
    return _op(build)


_FP32, _NO_DGRAD, _NO_WGRAD, _NO_FWD = ({"mode": "fp32"}, {"mask": 5}, {"mask": 3}, {"mask": 6})
CASES = {
    "layer_norm": (_layer_norm(), {}),
    "add_layer_norm": (_layer_norm(add=True), {}),
    "add_layer_norm_dy_none": (_layer_norm(add=True, pattern=[True, False]), {}),
    "add_layer_norm_ds_none": (_layer_norm(add=True, pattern=[False, True]), {}),
    "graph_norm": (_graph_norm(), {}),
    "instance_norm": (_graph_norm(shift=False), {}),
    "add_graph_norm": (_graph_norm(add=True), {}),
    "add_instance_norm": (_graph_norm(add=True, shift=False), {}),
    "add_graph_norm_dy_none": (_graph_norm(add=True, pattern=[True, False]), {}),
    "add_graph_norm_ds_none": (_graph_norm(add=True, pattern=[False, True]), {}),
    "gate": (_gate(), {}),
    "scaled_silu": (_silu(), {}),
    "ln_silu": (_ln_silu(1), {}),
    "ln_silu_groups": (_ln_silu(2), {}),
    "fold_weight": (_fold_weight(), {}),
    "embed": (_embed(), {}),
    "embed_no_bias": (_embed(bias=False), {}),
    "edgedeg_fold": (_edgedeg_fold(), {}),
    "edgedeg_fold_no_expb_da_none": (_edgedeg_fold(expb=False, pattern=[True, False]), {}),
    "edgedeg_scatter": (_edgedeg_scatter(), {}),
    "edgedeg_scatter_no_bias": (_edgedeg_scatter(bias=False), {}),
    "gather_add": (_gather_add(), {}),
    "gather_add_no_b": (_gather_add(b=False), {}),
    "gather_add_b_constant": (_gather_add(b_grad=False), {}),
    "segment_sum": (_segment(), {}),
    "segment_scale": (_segment(scale_op=True), {}),
    "edge_geometry": (_edge_geometry(False), {}),
    "edge_geometry_offsets": (_edge_geometry(True), {}),
    "edge_geometry_length_only": (_edge_geometry(False, pattern=[False, True, False]), {}),
    "vec_sh": (_vec_sh(True), {}),
    "vec_sh_no_mask": (_vec_sh(False), {}),
    "rbf_gaussian": (_rbf("gaussian"), {}),
    "rbf_gaussian_length_constant": (_rbf("gaussian", length_grad=False), {}),
    "rbf_expnorm": (_rbf("expnorm"), {}),
    "rbf_bessel": (_rbf("bessel"), {}),
    "rbf_bessel_length_constant": (_rbf("bessel", length_grad=False), {}),
    "dtp_coupling": (_coupling(), {}),
    "dtp": (_dtp(True), {}),
    "dtp_no_w": (_dtp(False), {}),
    "dtp_linear": (_dtp_linear(), {}),
    "dtp_linear_no_w_no_bias": (_dtp_linear(w=False, bias=False), {}),
    "sep_fctp": (_sep_fctp(), {}),
    "sep_fctp_fp32": (_sep_fctp(), _FP32),
    "sep_fctp_d2_none": (_sep_fctp(pattern=[True, False]), {}),
    "sep_fctp_d1_none_fp32": (_sep_fctp(pattern=[False, True]), _FP32),
    "sep_fctp_exact_dgrad": (_sep_fctp(), _NO_DGRAD),
    "sep_fctp_exact_wgrad": (_sep_fctp(), _NO_WGRAD),
    "sep_fctp_exact_fwd": (_sep_fctp(), _NO_FWD),
    "sep_fctp_one_consumer": (_sep_fctp(n2=0), {}),
    "sep_fctp_one_consumer_fp32": (_sep_fctp(n2=0), _FP32),
    "sep_fctp_one_consumer_no_bias": (_sep_fctp(n2=0, bias=False), {}),
    "sep_fctp_bias_only_first": (_sep_fctp(bias2=False), {}),
    "sep_fctp_bias_only_second": (_sep_fctp(bias=False), {}),
    "sep_fctp_bias_only_second_fp32": (_sep_fctp(bias=False), _FP32),
    "sep_fctp_no_bias": (_sep_fctp(bias=False, bias2=False), {}),
    "sep_fctp_no_w": (_sep_fctp(w=False), {}),
    "sep_fctp_no_w_fp32": (_sep_fctp(w=False), _FP32),
    "sep_fctp_frozen_weight": (_sep_fctp(frozen=True), {}),
    "sep_fctp_frozen_weight_exact_wgrad": (_sep_fctp(frozen=True), _NO_WGRAD),
    "sep_fctp_gated": (_sep_fctp_gated(), {}),
    "sep_fctp_gated_no_bias_no_w": (_sep_fctp_gated(bias=False, w=False), {}),
    "sep_fctp_gated_frozen_weight": (_sep_fctp_gated(frozen=True), {}),
    "alpha_logits": (_alpha(), {}),
    "attn_aggregate": (_attn(), {}),
    "attn_aggregate_dropout": (_attn(0.25), {}),
    "attn_aggregate_dropout_seed_offset": (_attn(0.25, seed_offset=True), {}),
    "attn_aggregate_seed_offset_no_dropout": (_attn(0.0, seed_offset=True), {}),
    "kv_split": (_kv_split(), {}),
    "kv_split_dv_none": (_kv_split(pattern=[True, False]), {}),
    "dp_logits": (_dp_logits(), {}),
    "dp_logits_k_constant": (_dp_logits(k_grad=False), {}),
    "dens_corrupt": (_dens_corrupt(), {}),
    "dens_corrupt_ratio": (_dens_corrupt(0.5), {}),
    "dens_loss": (_dens_loss(), {}),
    "dens_loss_row_mask_stats": (_dens_loss(extras=True), {}),
    "is2rs_perturb": (_is2rs_perturb(False), {}),
    "is2rs_perturb_int64_tags": (_is2rs_perturb(True), {}),
    "is2rs_loss": (_is2rs_loss(), {}),
    "is2rs_loss_row_mask_stats": (_is2rs_loss(extras=True), {}),
    "metrics_accumulate": (_metrics(True), {}),
    "metrics_accumulate_energy_only": (_metrics(False), {}),
}


# ------------------------------------------------------------------------------------------------- passes
def _one_pass(make, which, rec, shapes):
    """the passes of linear_trace.py for operators with any number of outputs and leaves; fills `shapes`, returns the named
    tensors"""
    torch.manual_seed(0)
    named, x_leaf, params, run = make()
    named = list(named)
    for _, t in named:
        rec.register(t)

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
        pairs = [(y, d) for y, d in zip(ys, dys) if d is not None and y.requires_grad]
        return [y for y, _ in pairs], [d for _, d in pairs]

    leaves = ([x_leaf] if x_leaf is not None else []) + params

    def name_of(p):
        return next(name for name, t in named if t is p)

    def note_grads(tag=""):
        for p in leaves:
            note(name_of(p) + ".grad" + tag, p.grad)

    try:
        roots, dys = forward()
        if not roots or not leaves:
            return named
        if which in ("backward_deferred", "backward_immediate", "backward_twice"):
            torch.autograd.backward(roots, dys)
            note_grads()
            if which == "backward_twice":
                roots, dys = forward("'")
                torch.autograd.backward(roots, dys)
                note_grads("'")
        elif which == "grad_params":
            if params:
                for p, g in zip(params, torch.autograd.grad(roots, params, dys, allow_unused=True)):
                    note("d" + name_of(p), g)
        elif which in ("force", "force_create_graph"):
            if x_leaf is not None:
                with ops.input_grads_only():
                    (g,) = torch.autograd.grad(roots, [x_leaf], dys, create_graph=which == "force_create_graph",
                                               allow_unused=True)
                note("dx", g)
        else:
            wrt = leaves if which == "create_graph_params" else leaves[:1]
            gs = torch.autograd.grad(roots, wrt, dys, create_graph=True, allow_unused=True)
            second, cots = [], []
            for p, g in zip(wrt, gs):
                note("d" + name_of(p), g)
                if g is not None and g.requires_grad:
                    c = _rand(*g.shape)
                    note("c_d" + name_of(p), c)
                    second.append(g)
                    cots.append(c)
            if second:
                torch.autograd.backward(second, cots)
            note_grads()
            for i, d in enumerate(dys):
                note("dy%d.grad" % i, d.grad)
    except (NotImplementedError, RuntimeError, ops.HipOnlyError) as e:
        rec.events.append({"call": "raised", "args": [type(e).__name__]})
    return named


def trace(case, which):
    """{"events": [...], "tensors": {name: [shape, stride] or None}} of one case under one kind of pass"""
    make, opts = CASES[case]
    rec = _OpsRecorder()
    saved = {k: getattr(ops, k) for k in ("_chk", "_stream", "_capturing", "call", "_p", "torch")}
    saved_spec = (ops.SfcSpec.x_mask, ops.SfcSpec.packed_numel)
    prev_defer = ops.set_deferred_weight_gradients(which != "backward_immediate")
    prev_mode = ops.set_matrix_mode(opts.get("mode", "split"))
    ops._chk = lambda *ts: None
    ops._stream = lambda: None
    ops._capturing = lambda: False
    ops.call = rec.call
    ops._p = rec.p
    ops.torch = _TorchOfThePass(rec)
    ops.SfcSpec.x_mask = lambda self, mode, E=None: opts.get("mask", 7)
    ops.SfcSpec.packed_numel = lambda self, mode: 64
    shapes = {}
    try:
        named = _one_pass(make, which, rec, shapes)
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        ops.SfcSpec.x_mask, ops.SfcSpec.packed_numel = saved_spec
        ops.set_deferred_weight_gradients(prev_defer)
        ops.set_matrix_mode(prev_mode)
    return {"events": rec.resolved(named), "tensors": shapes}


def trace_all():
    out = {case: {which: trace(case, which) for which in PASSES} for case in CASES}
    return json.loads(json.dumps(out))  # (plain lists, as the recorded file holds them)


# ------------------------------------------------------------------------------------------------- the recorded file
# The packed form of linear_trace.py: every distinct struct, event and tensor table once, one per line, a trace as indices.
def pack(traces):
    structs, events, tensors, out = {}, {}, {}, {}

    def fold(v):  # structs by index
        if isinstance(v, dict):
            v = {k: fold(x) for k, x in v.items()}
            return {"struct#": _index(structs, v)} if "struct" in v else v
        return [fold(x) for x in v] if isinstance(v, list) else v

    for case in sorted(traces):
        out[case] = {which: [_index(tensors, traces[case][which]["tensors"]),
                             [_index(events, fold(e)) for e in traces[case][which]["events"]]] for which in PASSES}
    return {"structs": [json.loads(k) for k in structs], "events": [json.loads(k) for k in events],
            "tensors": [json.loads(k) for k in tensors], "traces": out}


def unpack(packed):
    def unfold(v):
        if isinstance(v, dict):
            return unfold(packed["structs"][v["struct#"]]) if "struct#" in v else {k: unfold(x) for k, x in v.items()}
        return [unfold(x) for x in v] if isinstance(v, list) else v

    events = [unfold(e) for e in packed["events"]]
    return {case: {which: {"events": [events[i] for i in ev], "tensors": packed["tensors"][t]}
                   for which, (t, ev) in passes.items()} for case, passes in packed["traces"].items()}


def dump(packed, f):
    def line(x):
        return json.dumps(x, sort_keys=True, separators=(",", ":"))
    f.write("{")
    for key in ("structs", "events", "tensors"):
        f.write('"%s":[\n%s\n],\n' % (key, ",\n".join(line(x) for x in packed[key])))
    rows = ['"%s":{\n%s\n}' % (case, ",\n".join('"%s":%s' % (w, line(packed["traces"][case][w])) for w in PASSES))
            for case in sorted(packed["traces"])]
    f.write('"traces":{\n%s\n}}\n' % ",\n".join(rows))


if __name__ == "__main__":
    with open(sys.argv[1], "w") as f:
        dump(pack(trace_all()), f)
