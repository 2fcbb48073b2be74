"""Shared by tests/test_gpu_sfc_edges.py (GPU) and tests/test_sfc_edge_cases.py (CPU): the SE(3) cases of the fused
SeparableFCTP kernels (csrc/sfcx.hip, sfcy.hip, sfcw.hip, sfc.hip), the edge counts at which their tiles and their host
dispatch change, guarded buffers, the float64 reference with its float32 yardstick, and the comparison with its bounds
(TEST INFRASTRUCTURE, importable without a GPU; nothing here launches a kernel).

Edge counts.  E_TILE lies around the 32-edge tiles of sfcx.hip and of sfc.hip (B_TE, W_SUB), the 64-edge F_TE of sfc.hip
and the 64-edge minimum weight-gradient chunk, and the 128-edge workgroup tile of sfcy.hip.  The dispatch edges are DERIVED: from the planners (`eqf_sfcx_dev_plan`,
host only: nx, ny, lds, echunk) and from constants parsed out of the .hip sources, so that a retuned threshold moves the
tests with it (tests/test_sfc_edge_cases.py shows both numbers when the table of this tree no longer holds):
  one-wave forward      4 / 2 / 1 waves per item while 4 nx ny, 2 nx ny <= slots (2048; 1024 for degree 3) and the LDS
                        condition of `fwd_split` holds (it rules the 4-way split out for degree 3)
  data gradient         two waves per item (every other path each) while 2 nx ny <= BWD_PSPLIT_SLOTS.  Degree-3 layouts always
                        run their two-wave half-pass kernel: they have NO edge here.  wide_l2's data gradient is served by the
                        exact-fp32 kernel (x_mask == 5): no edge either
  weight gradient       the one-wave chunk grows from XW_MIN_CHUNK (64) to 96 edges at E = 64 ceil(3072 / nitem) + 1
  sfcy launch padding   tile groups in batches of 8 per XCD (operators with per-edge weights): E = 1025 (9 groups), 8193 (65)
  default dispatch      Y_MIN_EDGES, Y_MIN_EDGES_GATED, W_MIN_EDGES, W_MIN_EDGES_PLAIN and the rounds of sfcw.hip at 22 000

Guarded buffers.  Every per-edge tensor of a launch sits in the middle of a [G + rows + G, cols] allocation, G = 128 rows (the
largest tile: an over-read inside a tile stays inside the allocation).  Guard rows of inputs are NaN (a padded row that
reaches a result through a product with a zero mask shows), guard rows of outputs are NaN (overwritten outputs) or a recorded
random sentinel (accumulated outputs: an atomic add into a NaN would leave the NaN); `check_guarded` compares the guard
rows bit for bit with what was put there.  Flat parameter gradients are guarded as [n / 32, 32] rows.  On a GPU the whole
buffer is a `poison.guard_input` copy: bands of tests/poison.py around the guard rows, checked by the `poisoned_ops` fixture
where a test uses it (a store further out than G rows).

Metric and bounds: those of the sibling files (largest error over the largest reference entry of the tensor; split 1e-4,
bf16 3e-2, split6 and exact fp32 max(5e-6, 4 x float32 yardstick on the same inputs), bias gradients 1e-5)."""
import ctypes
import os
import re
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fp64_ops  # noqa: E402
from fp64_tp import blocks as _blocks, reference  # noqa: E402
from equiformer_amd import lib as _lib, ops, so3  # noqa: E402
from equiformer_amd.layout import DtpTable, RowLayout  # noqa: E402
from poison import guard_input  # noqa: E402

G = 128
E_TILE = [1, 31, 32, 33, 63, 65, 127, 129]
MODE_OF = {"split": 0, "bf16": 1, "split6": 2, "fp32": None}
TOL = {"split": 1e-4, "bf16": 3e-2}  # tests/test_gpu_sfcx.py, tests/test_gpu_sfc_e3.py
FP32_FLOOR, YARD_FACTOR = 5e-6, 4.0  # tests/test_gpu_op_edges.py: max(project bound, 4 x float32 yardstick)
BIAS_TOL = 1e-5  # tests/test_gpu_sfcw.py
GATE_S, GATE_G, GATED_IRREPS = 128, 96, "64x1e+32x2e"  # the gate in front of the QM9 sep_value
SH = {1: "1x0e+1x1e", 2: "1x0e+1x1e+1x2e", 3: "1x0e+1x1e+1x2e+1x3e"}
QM9, MD17 = "128x0e+64x1e+32x2e", "128x0e+64x1e+64x2e+32x3e"
# name: irreps in = DTP irreps, lmax of sh, out1, n2, per-edge w, gate folded, multi-wave kernels accept (degrees <= 2)
CASES = {
    "qm9_sep_act": (QM9, 2, "224x0e+64x1e+32x2e", 128, True, False, True),
    "qm9_sep_value": (QM9, 2, QM9, 0, False, False, True),
    "qm9_sep_value_gated": (QM9, 2, QM9, 0, False, True, True),
    "oc20_l1": ("256x0e+128x1e", 1, "256x0e+128x1e", 0, True, False, True),
    "md17_l3": (MD17, 3, MD17, 0, True, False, False),
    "md17_l3_act": (MD17, 3, "224x0e+64x1e+64x2e+32x3e", 128, True, False, False),
    "wide_l2": ("256x0e+128x1e+64x2e", 2, "256x0e+128x1e+64x2e", 0, True, False, True),
}
FWD_CODE = {1: "one-wave x1", 2: "one-wave x2", 4: "one-wave x4", 8: "sfcy"}  # eqf_sfcx_dev_served(0)
BWD_CODE = {0: "exact fp32", 1: "unsplit", 2: "split", 3: "degree-3"}  # (1); 0: the launch went to eqf_sfc_bwd_data
WG_CODE = {1: "one-wave", 2: "sfcw"}  # (2)
QUANTITIES = ["out1", "out2", "dx", "dM", "dw", "dweight", "dweight2", "dbias", "dbias2"]


class Setup:
    """tables and sizes of a case"""

    def __init__(self, name):
        irr, lmax, out, n2, use_w, gated, multi = CASES[name]
        self.name, self.n2, self.use_w, self.gated, self.multi, self.lmax = name, n2, use_w, gated, multi, lmax
        self.table, self.lay = DtpTable(irr, SH[lmax], irr), RowLayout(out)
        self.spec = ops.SfcSpec(self.table, self.lay, n2=n2)
        assert self.spec.supported
        self.gate = (GATE_S, RowLayout(GATED_IRREPS), so3.C_SILU, so3.C_SIGMOID) if gated else None
        self.x_dim = self.table.layout_in.dim + (GATE_G if gated else 0)
        self.deg3 = lmax == 3

    def x_mask(self, mode):
        m = self.spec.x_mask(mode)
        if self.name == "wide_l2":  # 14 input slabs > the 12 of the data gradient's table: that launch is the exact-fp32 kernel's
            assert m == 5, m
        else:
            assert m == 7, (self.name, m)
        return m


_setups = {}


def setup(name):
    if name not in _setups:
        _setups[name] = Setup(name)
    return _setups[name]


# ------------------------------------------------------------------------------------------------- constants and planners
def _src(name):
    return open(os.path.join(ROOT, "equiformer_amd", "csrc", name)).read()


def constants():
    """thresholds of the host dispatch, parsed from the sources"""
    x, w = _src("sfcx.hip"), _src("sfcw.hip")
    c = {}
    for k in ("W_MIN_EDGES", "W_MIN_EDGES_PLAIN", "Y_MIN_EDGES", "Y_MIN_EDGES_GATED", "BWD_PSPLIT_SLOTS", "XB_WAVE1_OFF",
              "XW_MIN_CHUNK"):
        c[k] = int(re.search(r"constexpr int %s = (\d+);" % k, x).group(1))
    m = re.search(r"const long slots = max_deg\(C\) <= 5 \? (\d+) : (\d+);", x)
    c["FWD_SLOTS"], c["FWD_SLOTS_D3"] = int(m.group(1)), int(m.group(2))
    c["XW_WAVES"] = int(re.search(r"int z = eqf_cdiv\((\d+), nitem\);", x).group(1))
    c["W_ROUNDS_EDGES"] = int(re.search(r"const int rounds = C\.E >= (\d+) \?", w).group(1))
    return c


def plan(name, kind, E, mode=0):
    """header of eqf_sfcx_dev_plan as a dict (kind 0 forward, 1 data gradient, 2 one-wave weight gradient, 3 multi-wave weight
    gradient) + its lines; None where the planner refuses the operator"""
    s = setup(name)
    L = _lib.load()
    L.eqf_sfcx_dev_plan.restype = ctypes.c_int
    L.eqf_sfcx_dev_plan.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.c_char_p, ctypes.c_int]
    buf = ctypes.create_string_buffer(1 << 17)
    n = L.eqf_sfcx_dev_plan(kind, ctypes.cast(s.table.c_ref, ctypes.c_void_p), ctypes.cast(s.lay.c_ref, ctypes.c_void_p), s.n2, E,
                            mode, buf, len(buf))
    if n <= 0:
        return None
    lines = [ln.split() for ln in buf.value.decode().splitlines()]
    head = lines[0]
    return dict(zip(head[1::2], (int(v) for v in head[2::2]))), lines


def _x_ctmax(d3):  # csrc/sfcx_common.h
    return 3 if d3 == 1 else (2 if d3 == 3 else 1)


def fwd_waves(name, E):
    """waves per item of the one-wave forward: `fwd_split` of csrc/sfcx.hip on the planner's nx, ny, lds"""
    c = constants()
    head, lines = plan(name, 0, E)
    items = head["nx"] * head["ny"]
    slots = c["FWD_SLOTS_D3"] if setup(name).deg3 else c["FWD_SLOTS"]
    wave_lds = head["lds"] // 4
    accf = max(int(ln[1]) * _x_ctmax(int(ln[1])) * 16 * 64 for ln in lines if ln[0] == "deg")
    for nsp in (4, 2):
        if nsp * items > slots:
            continue
        region = max(wave_lds, accf) if nsp == 2 else wave_lds
        need = 4 * (2 * region if nsp == 2 else nsp * region + accf)
        if need > 64 * 1024:
            continue
        return nsp
    return 1


def bwd_code(name, E, psplit_allowed=True):
    """expected eqf_sfcx_dev_served(1) of the data gradient"""
    s = setup(name)
    if not s.x_mask(0) & 2:
        return 0
    if s.deg3:
        return 3
    c = constants()
    head, _ = plan(name, 1, E)
    split = psplit_allowed and 2 * head["nx"] * head["ny"] <= c["BWD_PSPLIT_SLOTS"] and head["lds"] <= 4 * c["XB_WAVE1_OFF"]
    return 2 if split else 1


def sfcw_accepts(name, mode=0, E=4096):
    """the multi-wave weight-gradient planner's own verdict (kind 3) in a matrix mode: with the three planes of split6 its d_out
    planes do not fit the 80 KB of two workgroups per CU for any case here, and the one-wave kernel serves"""
    return plan(name, 3, E, mode) is not None


def dispatch_edges(name):
    """[(limit, launch family, (E below, E above), (code below, code above))] of the forced one-wave variants; family 0 / 1 / 2 as
    in eqf_sfcx_dev_served; for the weight-gradient chunk the 'codes' are the chunk lengths (the kernel is the one-wave one)"""
    s, c = setup(name), constants()
    out = []
    ny = plan(name, 0, 1)[0]["ny"]
    slots = c["FWD_SLOTS_D3"] if s.deg3 else c["FWD_SLOTS"]
    for nsp, label in ((4, "fwd 4->2"), (2, "fwd 2->1")):
        e = 32 * (slots // (nsp * ny))
        a, b = fwd_waves(name, e), fwd_waves(name, e + 1)
        if a != b:  # (degree 3: the LDS condition leaves no 4-way split, so there is no 4 -> 2 edge)
            out.append((label, 0, (e, e + 1), (a, b)))
    if s.x_mask(0) & 2 and not s.deg3:
        ngrp = plan(name, 1, 1)[0]["ny"]
        e = 32 * (c["BWD_PSPLIT_SLOTS"] // (2 * ngrp))
        out.append(("bwd psplit", 1, (e, e + 1), (bwd_code(name, e), bwd_code(name, e + 1))))
    nitem = plan(name, 2, 1)[0]["ny"]
    e = c["XW_MIN_CHUNK"] * -(-c["XW_WAVES"] // nitem)
    out.append(("wgrad chunk", 2, (e, e + 1), (plan(name, 2, e)[0]["echunk"], plan(name, 2, e + 1)[0]["echunk"])))
    return out


def default_edges(name):
    """[(limit, family, (E below, E above), (code below, code above))] of the automatic choice (variant 0)"""
    s, c = setup(name), constants()
    out = []
    y = c["Y_MIN_EDGES_GATED"] if s.gated else c["Y_MIN_EDGES"]
    out.append(("Y_MIN_EDGES_GATED" if s.gated else "Y_MIN_EDGES", 0, (y - 1, y), (fwd_waves(name, y - 1), 8 if s.multi else fwd_waves(name, y))))
    w = c["W_MIN_EDGES"] if s.use_w else c["W_MIN_EDGES_PLAIN"]
    out.append(("W_MIN_EDGES" if s.use_w else "W_MIN_EDGES_PLAIN", 2, (w - 1, w), (1, 2 if s.multi else 1)))
    if not s.use_w:
        r = c["W_ROUNDS_EDGES"]
        out.append(("sfcw rounds", 2, (r - 1, r), (2, 2)))
    return out


SFCY_PADDING_E = [1025, 8193]  # 9 and 65 groups of 4 x 32 edges: one past a batch of 8, one past 8 batches


def expected_codes(name, E, fwd_variant=0, wg_variant=0, psplit_off=False, mode=0):
    """(forward, data gradient, weight gradient) codes of eqf_sfcx_dev_served the host dispatch must report for a launch of E
    edges under the development switches (key 2, key 4, key 9 of eqf_sfcx_dev_set) in matrix mode `mode` (0 split, 1 bf16, 2 split6)"""
    s, c = setup(name), constants()
    y_min = c["Y_MIN_EDGES_GATED"] if s.gated else c["Y_MIN_EDGES"]
    w_min = c["W_MIN_EDGES"] if s.use_w else c["W_MIN_EDGES_PLAIN"]
    fwd = 8 if (s.multi and (fwd_variant == 2 or (fwd_variant == 0 and E >= y_min))) else fwd_waves(name, E)
    wg = 2 if (s.multi and sfcw_accepts(name, mode, E) and (wg_variant == 2 or (wg_variant == 0 and E >= w_min))) else 1
    return fwd, bwd_code(name, E, not psplit_off), wg


# ------------------------------------------------------------------------------------------------- guarded buffers
class Guarded:
    """buf [G + rows + G, cols]; mid = buf[G : G + rows]; guards: the int32 image of the guard rows as they were filled; prefill:
    what the middle held before the launch (accumulated outputs) or None"""

    def __init__(self, buf, rows, prefill):
        if buf.device.type != "cpu":  # the whole buffer once more between the bands of tests/poison.py: a store further out than G rows
            buf = guard_input(buf)
        self.buf, self.rows, self.prefill = buf, rows, prefill
        self.mid = buf[G:G + rows]
        self.guards = self._guard_bits().clone()

    def _guard_bits(self):
        return torch.cat([self.buf[:G], self.buf[G + self.rows:]]).contiguous().view(torch.int32)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.mid.data_ptr())


def guarded(rows, cols, fill, device="cpu", seed=0):
    """fill: "nan" -- an output the kernel overwrites: NaN everywhere;  "acc" -- an output it adds into: random unit-scale prefill in
    the middle, a random sentinel in the guard rows, both recorded;  a [rows, cols] tensor -- an input: NaN guard rows around it"""
    if isinstance(fill, str) and fill == "nan":
        return Guarded(torch.full((2 * G + rows, cols), float("nan"), device=device), rows, None)
    if isinstance(fill, str) and fill == "acc":
        buf = torch.randn(2 * G + rows, cols, generator=torch.Generator().manual_seed(1000 + seed)).to(device)
        return Guarded(buf, rows, buf[G:G + rows].clone())
    assert tuple(fill.shape) == (rows, cols), (fill.shape, rows, cols)
    buf = torch.full((2 * G + rows, cols), float("nan"), device=device)
    buf[G:G + rows] = fill.to(device)
    return Guarded(buf, rows, None)


def check_guarded(g, what=""):
    """guard rows bit-identical to what was put there (compared as int32); an overwritten output finite in every element of the
    middle; returns what is compared with the reference: the middle, minus the prefill for an accumulated output"""
    now = g._guard_bits()
    if not torch.equal(now, g.guards):
        bad = (now != g.guards).nonzero()
        r = int(bad[0, 0])
        raise AssertionError("%s: %d guard elements changed, first in guard row %d (%s the tensor) column %d" % (
            what, bad.shape[0], r if r < G else r - G, "before" if r < G else "behind", int(bad[0, 1])))
    mid = g.mid.detach().cpu()
    assert torch.isfinite(mid).all(), "%s: %d elements of the result are not finite" % (what, int((~torch.isfinite(mid)).sum()))
    if g.prefill is not None:
        return mid.double() - g.prefill.cpu().double()
    return mid


# ------------------------------------------------------------------------------------------------- inputs and reference
def inputs(name, E):
    """float32 CPU tensors of a launch, deterministic per (case, E)"""
    s = setup(name)
    g = torch.Generator().manual_seed(7919 * sorted(CASES).index(name) + E)
    r = lambda *shape: torch.randn(*shape, generator=g)  # noqa: E731
    t, sp = s.table, s.spec
    d = dict(x=r(E, s.x_dim), M=r(E, t.m_numel), w=r(E, t.weight_numel) if s.use_w else None,
             weight=r(sp.weight_numel) * 0.1, weight2=r(sp.weight2_numel) * 0.1 if s.n2 else None,
             bias=r(s.lay.mul_of(0)), bias2=r(s.n2) if s.n2 else None, d1=r(E, s.lay.dim), d2=r(E, s.n2) if s.n2 else None)
    return d


def evaluate(name, inp, dtype, spec=None):
    """the operator and every gradient in `dtype` on the CPU from the restatement of tests/fp64_tp.py (+ fp64_ops.gate for the gated
    case) and autograd, in the scheme of Case.ref of tests/test_gpu_sfc_e3.py.  spec: another path table (the teeth tests)."""
    s = setup(name)
    spec = spec or s.spec
    f = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(True)  # noqa: E731
    x, M, w = f(inp["x"]), f(inp["M"]), f(inp["w"])
    weight, weight2, bias, bias2 = f(inp["weight"]), f(inp["weight2"]), f(inp["bias"]), f(inp["bias2"])
    xin = fp64_ops.gate(x, *s.gate) if s.gated else x
    o1, o2 = reference(spec, xin, M, w, _blocks(spec, weight), weight2, bias, bias2)
    loss = (o1 * inp["d1"].to(dtype)).sum()
    if o2 is not None:
        loss = loss + (o2 * inp["d2"].to(dtype)).sum()
    wrt = dict(dx=x, dM=M, dw=w, dweight=weight, dweight2=weight2, dbias=bias, dbias2=bias2)
    names = [k for k, v in wrt.items() if v is not None]
    out = dict(zip(names, torch.autograd.grad(loss, [wrt[k] for k in names])))
    out["out1"], out["out2"] = o1.detach(), (o2.detach() if o2 is not None else None)
    return {k: out.get(k) for k in QUANTITIES}


_refs = {}


def ref_and_yard(name, E):
    """(inputs, float64 reference, the same function in float32 on the CPU), cached for the session: the four modes share one
    evaluation.  The large edge counts are kept one at a time."""
    key = (name, E)
    if key not in _refs:
        if E > 256:
            for k in [k for k in _refs if k[1] > 256]:
                del _refs[k]
        inp = inputs(name, E)
        _refs[key] = (inp, evaluate(name, inp, torch.float64), evaluate(name, inp, torch.float32))
    return _refs[key]


# ------------------------------------------------------------------------------------------------- comparison
def rel(got, ref):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def bound_of(mode, quantity, yard):
    if quantity in ("dbias", "dbias2"):
        return BIAS_TOL
    if mode in TOL:
        return TOL[mode]
    return max(FP32_FLOOR, YARD_FACTOR * yard)


class Checker:
    """collects the comparisons of a test item, keeps the worst case of every (launch, quantity), prints the FIG lines and fails
    at the end, so that one run shows every figure"""

    def __init__(self, case, mode):
        self.case, self.mode, self.bad, self.worst = case, mode, [], {}

    def cmp(self, launch, quantity, got, ref, y32, E=None):
        err, yard = rel(got, ref), rel(y32, ref)
        lim = bound_of(self.mode, quantity, yard)
        k = (launch, quantity)
        w = self.worst.get(k)
        if w is None or err / lim > w[0] / w[2]:
            self.worst[k] = (err, yard, lim, E)
        if not err < lim:
            self.bad.append((launch, quantity, E, err, yard, lim))

    def done(self):
        for (launch, quantity), (err, yard, lim, E) in self.worst.items():
            print("FIG %s %s %s %s err=%.2e yard=%.2e bound=%.2e E=%s" % (self.case, self.mode, launch, quantity, err, yard, lim, E))
        assert not self.bad, (self.case, self.mode, self.bad)


def shifted_spec(name, path, by=32):
    """the case's operator with one path's w_off moved by `by` (teeth: the reference built from it must fail the comparison)"""
    s = setup(name)
    paths = [dict(p) for p in s.table.paths]
    paths[path]["w_off"] += by
    table = types.SimpleNamespace(paths=paths, layout_out=s.table.layout_out)
    return types.SimpleNamespace(table=table, degs=s.spec.degs, pars=s.spec.pars, w_offs=s.spec.w_offs, n2=s.spec.n2)
