"""Poisoned, guarded allocations for the operator-level fp64 suites (TEST INFRASTRUCTURE, importable without a GPU; nothing
here launches a HIP kernel of the project).

What the suites could not see.  They compare the values a kernel wrote with a float64 restatement.  They do not see where
else the kernel wrote, what it never wrote, or what it read past the end of a tensor: `equiformer_amd/ops.py` and its
sibling modules allocate results with torch.empty / empty_like / zeros / zeros_like, and the caching allocator serves these
from blocks that an earlier call of the same operator at the same shape has just filled with correct values.

`poisoned(modules=...)` replaces the module-level name `torch` of each named module by a proxy (the precedent is
`tests/ops_trace.py::_TorchOfThePass`) that forwards everything except those four functions.  An intercepted call returns a
tensor of the shape, dtype, device and strides torch would return, placed in the middle of a larger allocation that the
registry keeps alive until `check()`:

    [ front band | the tensor | back band ]

A band holds the bytes of G = 128 rows of the tensor's own last dimension (the G of tests/sfc_edge_cases.py), at least 4 KiB,
rounded up to a multiple of 512 bytes, so that the data pointer keeps the alignment the caching allocator gives (float4 and
16-byte loads rely on it).  The back band begins at the first byte behind the tensor.

Fill, in the convention of `sfc_edge_cases.guarded`:
  empty / empty_like, floating   NaN in the body, NaN in the bands: an element no kernel wrote is a NaN in the result, and the
                                 `_Checker.cmp` of every suite asserts finite-and-within-bound
  zeros / zeros_like, floating   zeros in the body, random finite values in the bands (an atomic add into a NaN would leave the
                                 NaN and go unseen; an add into a finite sentinel changes it)
  integer, bool, byte            the body is ZEROS, never a poison pattern, for empty as for zeros; the bands are random
                                 values.  REASON: these tensors are indices, offsets, counts and masks.  A kernel that reads a
                                 poisoned index before it is written would be sent to a wild address, and such a fault must not
                                 be provoked on a GPU that others share.  A zero index stays inside every tensor.
The band bits are recorded as slices of per-device blocks that are written once and never changed (a NaN block per dtype, a
block of random bytes 0..63: as the top byte of a float16, bfloat16, float32 or float64 these give a finite number below 2);
the bands are filled by the same fill or copied from that block.

CPU and pinned allocations pass through untouched (`cpu=True` intercepts CPU allocations as well: the controls of
tests/test_poison_alloc.py).  Inside a stream capture the proxy raises: captured steps are out of scope.

`check()` compares every band bit for bit with its record, on the device, with ONE reduction and ONE synchronisation for all
allocations of a device, and releases the allocations.  On a mismatch it raises AssertionError naming the allocation's call
site (file:line in the intercepted module), its shape, and whether the first changed element lies before or behind the tensor
and at which offset (in elements, counted away from the tensor: offset 0 is the element that touches it).

`guard_input(t)` returns a contiguous copy of `t` between bands of the same size (NaN for floating tensors, the random block
for index tensors, whose contents stay valid), keeps requires_grad, and registers the copy with the active registry, if there
is one, so that `check()` proves nobody wrote around it.  A load past an input then reads NaN instead of a neighbour.  The
choke points: `fp64_ops.evaluate` on a GPU, `second_order_ref._compare`, `Case.__init__` of tests/test_gpu_sfc_e3.py.

Fixtures `poisoned_ops` (the default modules) and `poisoned_model` (+ equiformer_amd.nets.layers) enter `poisoned()`, yield
the registry, call `check()` after the test body and print `POISON <nodeid> allocations=<n> guarded_bytes=<b>`.  A test module
opts in by importing the fixture and naming it in `pytest.mark.usefixtures`.

ops._zeros.  `ops._ZeroArena` carves float32 accumulators out of 16 MB slabs filled once; inside `poisoned()` every request
counts as too large for a slab (`_arena.MAX_REQ = -1`, restored on exit), so each accumulator is a guarded torch.zeros of its own.

Opted in as whole files (every test): test_gpu_op_edges, test_gpu_graph_norm, test_gpu_graph_edges, test_gpu_second_order_ops,
test_gpu_second_order, test_gpu_dtp_edges, test_gpu_dp_edges, test_gpu_sfc_e3, test_gpu_linear_unified, test_gpu_optim_edges.
Opted in per test, the operator-level tests of files that also hold model passes, captured steps and training loops:
  test_gpu_edge_degree.py   test_operator_against_fp64, test_argument_errors_and_refusals
  test_gpu_trainloss.py     test_grid_against_fp64, test_sums_accumulate_over_three_batches,
                            test_operator_autograd_and_device_weights
  test_gpu_dens_step.py     test_corruption_invariants, test_loss_forward_backward_against_fp64
  test_gpu_is2rs_step.py    test_perturbation_invariants, test_loss_forward_backward_against_fp64
  test_gpu_metrics.py       test_sums_against_fp64_at_every_size, test_nan_and_inf_in_excluded_rows_change_no_bit
  test_gpu_dropout.py       test_operator_is_the_product_with_keep_mask_at_every_order,
                            test_operator_edges_row_count_no_rows_refused_width_and_split_seed
  test_gpu_droppath.py      test_operator_is_segment_scale_of_keep_factors_at_every_order,
                            test_operator_edges_no_rows_refused_width_and_split_seed
  test_gpu_properties.py    test_molecules_without_edges_and_empty_graph (fixture poisoned_model: one eager model pass, E = 0)

EXCLUSIONS.  No test of a whole-file suite is left out.  In the per-test files these stay outside the fixture:
  captures a HIP graph (the proxy raises inside a capture):
    tests/test_gpu_edge_degree.py::test_captured_train_step_with_the_collapsed_embedding
    tests/test_gpu_dens_step.py::test_captured_step_equals_eager_loop
    tests/test_gpu_is2rs_step.py::test_captured_step_equals_eager_loop, ::test_captured_step_variants
    tests/test_gpu_metrics.py::test_update_is_legal_inside_a_stream_capture
    tests/test_gpu_dropout.py::test_captured_step_with_out_drop_equals_eager_loop, ::test_replays_draw_fresh_masks,
      ::test_bucketed_step_on_molecules_with_proj_drop_equals_eager_loop, ::test_default_seed_is_one_draw_taken_by_the_first_dropping_forward
    tests/test_gpu_droppath.py::test_captured_step_with_stochastic_depth_equals_eager_loop, ::test_replays_draw_fresh_masks,
      ::test_bucketed_step_on_molecules_equals_eager_loop, ::test_default_seed_is_drawn_once_and_only_by_a_model_that_drops
  asserts on host synchronisation (torch.cuda.set_sync_debug_mode("error") around the step; check() synchronises):
    tests/test_gpu_dens_step.py::test_no_host_synchronisation, tests/test_gpu_is2rs_step.py::test_no_host_synchronisation
  The remaining tests of those files are whole-model passes against the oracle, statistics of the device draws, padded-batch
  views and refusals that raise before a launch; the operators they run are the ones the tests above hold on poisoned allocations.
  Two tests of whole-file suites launch nothing and therefore report allocations=0: tests/test_gpu_graph_norm.py::
  test_bad_arguments_return_an_error_code (argument errors on pointers that are never dereferenced) and tests/
  test_gpu_second_order_ops.py::test_zz_report_measured_errors (writes the figures the other tests recorded).

The suites that drive the C ABI by hand allocate nothing through the package; their buffers go through `guard_input`:
`sfc_edge_cases.Guarded` (the whole [G + rows + G] buffer once more between bands), `Buf` of tests/test_gpu_trainloss.py, `_gpu` of
tests/test_gpu_optim_edges.py (as an [n, 1] column), `_run` of tests/test_gpu_metrics.py.

FINDINGS on an MI355X (one run of every opted-in file): none.  No guard band changed and no returned tensor held a NaN, at
every shape of these suites: 1 124 poisoned test items, 58 859 guarded allocations.
EXEMPTIONS: none.  No comparison was restricted to a part of a returned tensor.
"""
import contextlib
import importlib
import os
import sys

import pytest
import torch

G = 128
MIN_BAND = 4096
ALIGN = 512
DEFAULT_MODULES = tuple("equiformer_amd." + m for m in
                        ("ops", "graph", "dens", "is2rs", "dropout", "droppath", "evaluate", "train", "optim"))
INTERCEPTED = ("empty", "empty_like", "zeros", "zeros_like")
_EMPTY_OF = {"empty": torch.empty, "empty_like": torch.empty_like, "zeros": torch.empty, "zeros_like": torch.empty_like}
_THIS = os.path.abspath(__file__).rstrip("c")

_active = []  # registries of the `poisoned()` blocks that are open, innermost last


def band_bytes(shape, dtype):
    """bytes of one guard band of a tensor of this shape and dtype"""
    last = int(shape[-1]) if len(shape) else 1
    row = max(last, 1) * torch.empty((), dtype=dtype).element_size()
    return max(MIN_BAND, -(-G * row // ALIGN) * ALIGN)


class _Blocks:
    """the records: per device a block of random bytes 0..63 and per (device, dtype) a block of NaN.  A block is never written
    again; a larger one replaces it for later allocations while earlier records keep theirs."""

    def __init__(self):
        self.rand, self.nan = {}, {}

    def random(self, device, nbytes):
        b = self.rand.get(device)
        if b is None or b.numel() < nbytes:
            g = torch.Generator(device=device)  # (its own generator, drawn on the device: torch's global streams do not move)
            g.manual_seed(20240)
            n = max(1 << 20, 2 * nbytes)
            b = self.rand[device] = torch.randint(0, 64, (n,), generator=g, dtype=torch.uint8, device=device)
        return b[:nbytes]

    def nans(self, device, dtype, nbytes):
        b = self.nan.get((device, dtype))
        if b is None or b.numel() < nbytes:
            n = max(1 << 20, 2 * nbytes)
            b = self.nan[(device, dtype)] = torch.full((n // torch.empty((), dtype=dtype).element_size(),), float("nan"),
                                                       dtype=dtype, device=device).view(torch.uint8)
        return b[:nbytes]


_blocks = _Blocks()


class _Allocation:
    __slots__ = ("buf", "band", "nbytes", "record", "site", "shape", "dtype", "kind")

    def bands(self):
        return self.buf[:self.band], self.buf[self.band + self.nbytes:]


def _call_site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename).rstrip("c") == _THIS:
        f = f.f_back
    return "?" if f is None else "%s:%d" % (f.f_code.co_filename, f.f_lineno)


class Registry:
    """the guarded allocations of one `poisoned()` block"""

    def __init__(self):
        self.live = []
        self.allocations = 0    # since the block was entered, over every check()
        self.guarded_bytes = 0  # bytes of the guarded tensors themselves (bands not counted)

    # ---------------------------------------------------------------------------------------------------- allocation
    def _place(self, like, kind, site):
        """a tensor with the shape, dtype, device and strides of `like` between two bands; kind: "nan" (NaN body and bands, floating
        only), "zero" (zero body, random bands) or "copy" (body left to the caller; NaN bands if floating, else random bands)"""
        dtype, device, shape = like.dtype, like.device, tuple(like.shape)
        item = like.element_size()
        floating = dtype.is_floating_point or dtype.is_complex
        if kind == "nan" and not floating:
            kind = "zero"
        strides = like.stride()  # (torch's own: contiguous, or those of a dense permuted tensor that empty_like preserves)
        a = _Allocation()
        a.band, a.nbytes = band_bytes(shape, dtype), like.numel() * item
        a.site, a.shape, a.dtype, a.kind = site, shape, dtype, kind
        a.buf = torch.empty(2 * a.band + a.nbytes, dtype=torch.uint8, device=device)
        front, back = a.bands()
        if kind == "nan" or (kind == "copy" and floating):
            a.record = _blocks.nans(device, dtype, a.band)
            if kind == "nan":
                a.buf.view(dtype).fill_(float("nan"))
            else:
                front.view(dtype).fill_(float("nan"))
                back.copy_(a.record)  # (its start need not be a multiple of the element size)
        else:
            a.record = _blocks.random(device, a.band)
            front.copy_(a.record)
            back.copy_(a.record)
            if kind == "zero" and a.nbytes:
                a.buf[a.band:a.band + a.nbytes].zero_()
        t = torch.empty(0, dtype=dtype, device=device).set_(a.buf.untyped_storage(), a.band // item, shape, strides)
        self.live.append(a)
        self.allocations += 1
        self.guarded_bytes += a.nbytes
        return t

    def allocate(self, name, args, kwargs, cpu=False):
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("poison: torch.%s inside a stream capture; captured steps are not run on poisoned allocations" % name)
        site = _call_site()
        kw = dict(kwargs)
        requires_grad = kw.pop("requires_grad", False)
        like = _EMPTY_OF[name](*args, **kw)
        if (like.device.type == "cpu" and (not cpu or kw.get("pin_memory"))) or like.layout != torch.strided:
            return getattr(torch, name)(*args, **kwargs)
        t = self._place(like, "zero" if name.startswith("zeros") else "nan", site)
        return t.requires_grad_() if requires_grad else t

    def guard_input(self, t, site=None):
        src = t.detach().contiguous()
        out = self._place(src, "copy", site or _call_site())
        out.copy_(src)
        return out.requires_grad_(t.requires_grad)

    # ---------------------------------------------------------------------------------------------------- check
    def check(self):
        """every band bit-identical to its record: one comparison and one synchronisation per device; releases the allocations"""
        live, self.live = self.live, []
        by_device = {}
        for a in live:
            by_device.setdefault(a.buf.device, []).append(a)
        for device, group in by_device.items():
            now = torch.cat([b for a in group for b in a.bands()])
            rec = torch.cat([a.record for a in group for _ in (0, 1)])
            if not torch.equal(now, rec):
                raise AssertionError(self._describe(group))

    @staticmethod
    def _describe(group):
        lines = []
        for a in group:
            item = torch.empty((), dtype=a.dtype).element_size()
            for side, band in zip(("before", "behind"), a.bands()):
                diff = (band != a.record).nonzero().flatten()
                if diff.numel() == 0:
                    continue
                elems = torch.unique(diff // item)  # (both bands begin at a multiple of the element size)
                off = a.band // item - 1 - int(elems[-1]) if side == "before" else int(elems[0])
                changed = int(elems.numel())
                lines.append("guard band changed %s the tensor allocated at %s, shape %s, %s (%s): %d elements, the nearest at "
                             "offset %d %s it" % (side, a.site, list(a.shape), str(a.dtype).replace("torch.", ""), a.kind, changed,
                                                  off, side))
        return "\n".join(lines[:8] + (["... and %d more" % (len(lines) - 8)] if len(lines) > 8 else []))


class _PoisonedTorch:
    """`torch` as an intercepted module sees it inside `poisoned()`"""

    def __init__(self, registry, cpu):
        for name in INTERCEPTED:
            setattr(self, name, lambda *a, _n=name, **k: registry.allocate(_n, a, k, cpu))

    def __getattr__(self, name):
        return getattr(torch, name)


@contextlib.contextmanager
def poisoned(modules=DEFAULT_MODULES, cpu=False):
    """modules: module objects or dotted names; yields the registry.  The caller calls check()."""
    mods = [importlib.import_module(m) if isinstance(m, str) else m for m in modules]
    reg = Registry()
    proxy = _PoisonedTorch(reg, cpu)
    saved = [(m, m.__dict__["torch"]) for m in mods]
    # ops._zeros carves float32 accumulators out of 16 MB slabs that are zero-filled once (ops._ZeroArena): inside the block every
    # request counts as too large for a slab, so that each accumulator is a guarded torch.zeros of its own
    arenas = [(m._arena, m._arena.MAX_REQ) for m in mods if hasattr(getattr(m, "_arena", None), "MAX_REQ")]
    _active.append(reg)
    try:
        for m in mods:
            m.torch = proxy
        for a, _ in arenas:
            a.MAX_REQ = -1
        yield reg
    finally:
        _active.remove(reg)
        for m, t in saved:
            m.torch = t
        for a, req in arenas:
            del a.MAX_REQ  # (the class attribute shows again)
            assert a.MAX_REQ == req


def guard_input(t):
    """a contiguous copy of `t` between guard bands (see the module docstring); registered with the innermost open registry, or
    with none: the bands then still keep a load past the end from reading a neighbour"""
    reg = _active[-1] if _active else Registry()
    return reg.guard_input(t, _call_site())


def _fixture(extra=()):
    def fix(request):
        with poisoned(DEFAULT_MODULES + tuple(extra)) as reg:
            yield reg
            reg.check()
            print("POISON %s allocations=%d guarded_bytes=%d" % (request.node.nodeid, reg.allocations, reg.guarded_bytes))
    return fix


poisoned_ops = pytest.fixture(_fixture(), name="poisoned_ops")
poisoned_model = pytest.fixture(_fixture(("equiformer_amd.nets.layers",)), name="poisoned_model")
