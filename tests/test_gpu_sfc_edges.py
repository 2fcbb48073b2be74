"""The fused SeparableFCTP kernels on the SE(3) layouts the benchmarks run (QM9 l <= 2, MD17 l <= 3, OC20 l <= 1, with and
without a second consumer, per-edge weights, a folded gate) against the float64 restatement of tests/fp64_tp.py, launched
through the C ABI on GUARDED buffers (tests/sfc_edge_cases.py: cases, edge counts, guard rows, reference, bounds).

(a) tile edges: E = 1, 31, 32, 33, 63, 65, 127, 129 -- forward (one-wave, multi-wave), data gradient (paths split over two
    waves or not, with and without d_coupling), weight gradient (one-wave, multi-wave, with and without the bias gradients),
    in the modes split, bf16, split6 and on the exact-fp32 kernels (eqf_sfc_*: no variants, no gated form).
(b) dispatch edges: the last edge count on one side and the first on the other of every limit of the host dispatch, derived
    from the planners and the constants of the sources (item-count limits under the forced one-wave variants, the launch
    padding of the multi-wave forward, the *_MIN_EDGES limits under the automatic choice).
(c) every comparison asserts which kernel served the launch (eqf_sfcx_dev_served): a forced variant that fell through would
    turn half of the comparisons into repeats of the other half.

Outputs the kernels add into (d_coupling, dweight, dweight2, dbias, dbias2) start from a recorded random prefill; the guard
rows of every tensor must come back bit-identical, and every element of a result must be finite with NaN behind the inputs.

Every item prints "FIG <case> <mode> <launch> <quantity> err=... yard=... bound=... E=..." per worst case (pytest -rA / -s).

Measured on an MI355X: the worst case of each quantity over all cases, edge counts and launches (largest err / bound), from
the FIG lines of one run; err = the kernel, yard = the float32 restatement on the same inputs:
  split    out1 4.1e-6 (qm9_sep_act, E = 3904), out2 3.5e-6, dx 4.9e-6 (qm9_sep_act, E = 65), dM 3.8e-6, dw 4.1e-6 (oc20_l1,
           E = 1), dweight 1.1e-5 (oc20_l1, one-wave, E = 127), dweight2 8.5e-6 (md17_l3_act, E = 32)            bound 1e-4
  bf16     out1 3.8e-3, out2 3.2e-3, dx 4.0e-3 (qm9_sep_value_gated, E = 1), dM 3.1e-3, dw 4.4e-3, dweight 4.4e-3,
           dweight2 4.6e-3 (md17_l3_act, E = 1)                                                                    bound 3e-2
  split6   out1 1.5e-6 (wide_l2, multi-wave forward, E = 1025; yard 4.0e-7), out2 5.4e-7, dx 6.9e-7, dM 5.0e-7, dw 8.6e-7,
           dweight 7.9e-7, dweight2 3.5e-7                                                                         bound 5e-6
  fp32     out1 1.1e-6 (wide_l2, E = 33; yard 4.6e-7), out2 8.6e-7, dx 5.1e-7, dM 4.9e-7, dw 4.9e-7, dweight 1.5e-6
           (md17_l3, E = 127; yard 5.0e-7), dweight2 4.4e-7                                                        bound 5e-6
  bias gradients (split, bf16, split6)   dbias 3.4e-7, dbias2 3.1e-7                                               bound 1e-5
The yardstick stayed <= 5.8e-7 everywhere: 5e-6 was the binding term of every split6 / fp32 bound.  No guard row changed and
no result held a non-finite element.  The multi-wave weight gradient served split and bf16 on the degree <= 2 cases and
never split6 (its planner refuses: three d_out planes exceed its 80 KB of LDS), which the expected codes follow.
The slowest item took 3.3 s (md17_l3, 8 999 edges: the float64 reference on the CPU); the 215 items 49 s.
"""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfc_edge_cases as sc  # noqa: E402
from equiformer_amd import lib as _lib, ops  # noqa: E402
from equiformer_amd.lib import call  # noqa: E402

pytestmark = pytest.mark.gpu

P = lambda g: g.ptr if g is not None else None  # noqa: E731
T = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _served(family):
    return _lib.load().eqf_sfcx_dev_served(family)


class Launches:
    """the three launches of a case at E edges in one mode, every per-edge tensor guarded"""

    def __init__(self, name, E, mode):
        self.s, self.E, self.mode, self.m = sc.setup(name), E, mode, sc.MODE_OF[mode]
        self.inp, self.ref, self.yard = sc.ref_and_yard(name, E)
        s, inp, dev = self.s, self.inp, _dev()
        self.dev = dev
        self.mask = s.x_mask(self.m) if self.m is not None else 0
        gi = lambda k, cols: None if inp[k] is None else sc.guarded(E, cols, inp[k], dev)  # noqa: E731
        self.x, self.M, self.w = gi("x", s.x_dim), gi("M", s.table.m_numel), gi("w", s.table.weight_numel)
        self.d1, self.d2 = gi("d1", s.lay.dim), gi("d2", s.n2)
        d = lambda k: None if inp[k] is None else inp[k].to(dev)  # noqa: E731
        self.weight, self.weight2, self.bias, self.bias2 = d("weight"), d("weight2"), d("bias"), d("bias2")
        self.packed = ops._sfc_pack(self.weight, self.weight2, s.spec, self.m) if self.m is not None else None
        self.gin = _lib.EqfGateIn(sc.GATE_S, sc.GATE_G, float(s.gate[2]), float(s.gate[3])) if s.gated else None
        self.st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        self.L = _lib.load()
        _served(0), _served(1), _served(2)  # (clear the records of earlier launches)

    def _pk(self):
        return ctypes.c_void_p(self.packed.data_ptr())

    def inputs_untouched(self):
        for k in ("x", "M", "w", "d1", "d2"):
            g = getattr(self, k)
            if g is not None:
                assert torch.equal(g._guard_bits(), g.guards) and torch.equal(g.mid.cpu(), self.inp[k]), k

    def forward(self, variant):
        s, E, st = self.s, self.E, self.st
        t, lay, n2 = s.table, s.lay, s.n2
        o1 = sc.guarded(E, lay.dim, "nan", self.dev)
        o2 = sc.guarded(E, n2, "nan", self.dev) if n2 else None
        if self.m is None or not self.mask & 1:
            call("eqf_sfc_fwd", P(self.x), P(self.M), P(self.w), t.c_ref, ops._sfc_Wl(self.weight, s.spec), T(self.bias), T(self.weight2),
                 T(self.bias2), P(o1), lay.c_ref, P(o2), n2, E, st)
        else:
            self.L.eqf_sfcx_dev_set(2, variant)
            try:
                if s.gated:
                    call("eqf_sfcx_fwd_gated", P(self.x), ctypes.byref(self.gin), P(self.M), P(self.w), t.c_ref, self._pk(), T(self.bias),
                         P(o1), lay.c_ref, E, self.m, st)
                else:
                    call("eqf_sfcx_fwd", P(self.x), P(self.M), P(self.w), t.c_ref, self._pk(), T(self.bias), T(self.bias2), P(o1), lay.c_ref,
                         P(o2), n2, E, self.m, st)
                torch.cuda.synchronize()
            finally:
                self.L.eqf_sfcx_dev_set(2, 0)
        torch.cuda.synchronize()
        return _served(0), dict(out1=o1, out2=o2)

    def data_gradient(self, psplit_off, want_dM):
        s, E, st = self.s, self.E, self.st
        t, lay, n2 = s.table, s.lay, s.n2
        dx = sc.guarded(E, s.x_dim, "nan", self.dev)
        dw = sc.guarded(E, t.weight_numel, "nan", self.dev) if s.use_w else None
        dM = sc.guarded(E, t.m_numel, "acc", self.dev, seed=1) if want_dM else None
        if self.m is None or not self.mask & 2:
            call("eqf_sfc_bwd_data", P(self.x), P(self.M), P(self.w), t.c_ref, ops._sfc_Wl(self.weight, s.spec), T(self.weight2),
                 P(self.d1), lay.c_ref, P(self.d2), n2, P(dx), P(dw), P(dM), E, st)
        else:
            self.L.eqf_sfcx_dev_set(9, 1 if psplit_off else 0)
            try:
                if s.gated:
                    call("eqf_sfcx_bwd_data_gated", P(self.x), ctypes.byref(self.gin), P(self.M), P(self.w), t.c_ref, self._pk(),
                         P(self.d1), lay.c_ref, P(dx), P(dw), P(dM), E, self.m, st)
                else:
                    call("eqf_sfcx_bwd_data", P(self.x), P(self.M), P(self.w), t.c_ref, self._pk(), P(self.d1), lay.c_ref, P(self.d2), n2,
                         P(dx), P(dw), P(dM), E, self.m, st)
                torch.cuda.synchronize()
            finally:
                self.L.eqf_sfcx_dev_set(9, 0)
        torch.cuda.synchronize()
        return _served(1), dict(dx=dx, dw=dw, dM=dM)

    def weight_gradient(self, variant, bias):
        s, E, st = self.s, self.E, self.st
        t, lay, n2, sp = s.table, s.lay, s.n2, s.spec
        acc = lambda n, seed: sc.guarded(n // 32, 32, "acc", self.dev, seed=seed) if n else None  # noqa: E731
        dW, dW2 = acc(sp.weight_numel, 2), acc(sp.weight2_numel, 3)
        db, db2 = (acc(lay.mul_of(0), 4), acc(n2, 5)) if bias else (None, None)
        dWl = ops._sfc_Wl(dW.mid, sp)
        if self.m is None or not self.mask & 4:
            assert not bias  # (the exact-fp32 launch does not take the bias gradients along)
            call("eqf_sfc_bwd_weight", P(self.x), P(self.M), P(self.w), t.c_ref, P(self.d1), lay.c_ref, P(self.d2), n2, dWl, P(dW2), E, st)
        else:
            self.L.eqf_sfcx_dev_set(4, variant)
            try:
                if s.gated and bias:
                    call("eqf_sfcx_bwd_weight_gated_bias", P(self.x), ctypes.byref(self.gin), P(self.M), P(self.w), t.c_ref, P(self.d1),
                         lay.c_ref, dWl, P(db), E, self.m, st)
                elif s.gated:
                    call("eqf_sfcx_bwd_weight_gated", P(self.x), ctypes.byref(self.gin), P(self.M), P(self.w), t.c_ref, P(self.d1),
                         lay.c_ref, dWl, E, self.m, st)
                elif bias:
                    call("eqf_sfcx_bwd_weight_bias", P(self.x), P(self.M), P(self.w), t.c_ref, P(self.d1), lay.c_ref, P(self.d2), n2, dWl,
                         P(dW2), P(db), P(db2), E, self.m, st)
                else:
                    call("eqf_sfcx_bwd_weight", P(self.x), P(self.M), P(self.w), t.c_ref, P(self.d1), lay.c_ref, P(self.d2), n2, dWl,
                         P(dW2), E, self.m, st)
                torch.cuda.synchronize()
            finally:
                self.L.eqf_sfcx_dev_set(4, 0)
        torch.cuda.synchronize()
        return _served(2), dict(dweight=dW, dweight2=dW2, dbias=db, dbias2=db2)

    def compare(self, ck, launch, results):
        for q, g in results.items():
            if g is None:
                continue
            got = sc.check_guarded(g, "%s %s %s E=%d %s" % (self.s.name, self.mode, launch, self.E, q))
            ck.cmp(launch, q, got, self.ref[q], self.yard[q], self.E)


def _expect(name, E, launch, family, code, want):
    names = (sc.FWD_CODE, sc.BWD_CODE, sc.WG_CODE)[family]
    print("SERVED %s E=%d %s: %s" % (name, E, launch, names.get(code, code)))
    assert code == want, "%s E=%d %s: served by %s, expected %s" % (name, E, launch, names.get(code, code), names.get(want, want))


def _three_launches(ck, run, name, E, tag, fwd_variant, wg_variant):
    """forward, data gradient (with d_coupling) and weight gradient (with the bias gradients) under the given switches"""
    want = sc.expected_codes(name, E, fwd_variant, wg_variant, mode=run.m)
    code, res = run.forward(fwd_variant)
    _expect(name, E, "fwd " + tag, 0, code, want[0])
    run.compare(ck, "fwd " + tag, res)
    code, res = run.data_gradient(False, True)
    _expect(name, E, "bwd " + tag, 1, code, want[1])
    run.compare(ck, "bwd " + tag, res)
    code, res = run.weight_gradient(wg_variant, True)
    _expect(name, E, "wgrad " + tag, 2, code, want[2])
    run.compare(ck, "wgrad " + tag, res)
    run.inputs_untouched()


# (the exact-fp32 entry points have no gated form: that combination does not exist)
@pytest.mark.parametrize("case,mode", [(c, m) for c in sorted(sc.CASES) for m in ("split", "bf16", "split6", "fp32")
                                       if not (m == "fp32" and sc.CASES[c][5])])
def test_tile_edges(case, mode):
    s = sc.setup(case)
    ck = sc.Checker(case, mode)
    exact = mode == "fp32"
    for E in sc.E_TILE:
        run = Launches(case, E, mode)
        if exact:
            _, res = run.forward(0)
            run.compare(ck, "fwd", res)
            for want_dM in (True, False):
                _, res = run.data_gradient(False, want_dM)
                run.compare(ck, "bwd%s" % ("+dM" if want_dM else ""), res)
            _, res = run.weight_gradient(0, False)
            run.compare(ck, "wgrad", res)
            run.inputs_untouched()
            continue
        # forward: the one-wave kernel and, where its planner accepts the case, the multi-wave one (degree 3 falls through: once)
        for variant in (1, 2):
            if variant == 2 and not s.multi and E != sc.E_TILE[-1]:
                continue
            code, res = run.forward(variant)
            _expect(case, E, "fwd v%d" % variant, 0, code, sc.expected_codes(case, E, fwd_variant=variant)[0])
            run.compare(ck, "fwd v%d" % variant, res)
        for psplit_off in (False, True):
            for want_dM in (True, False):
                launch = "bwd%s%s" % (" nosplit" if psplit_off else "", "+dM" if want_dM else "")
                code, res = run.data_gradient(psplit_off, want_dM)
                _expect(case, E, launch, 1, code, sc.expected_codes(case, E, psplit_off=psplit_off)[1])
                run.compare(ck, launch, res)
        for variant in (1, 2):
            if variant == 2 and not s.multi and E != sc.E_TILE[-1]:
                continue
            for bias in (False, True):
                launch = "wgrad v%d%s" % (variant, "+bias" if bias else "")
                code, res = run.weight_gradient(variant, bias)
                _expect(case, E, launch, 2, code, sc.expected_codes(case, E, wg_variant=variant, mode=run.m)[2])
                run.compare(ck, launch, res)
        run.inputs_untouched()
    ck.done()


def _dispatch_items():
    items = []
    for case in sorted(sc.CASES):
        s = sc.setup(case)
        per_E = {}
        for label, _, es, _ in sc.dispatch_edges(case):
            for E in es:
                per_E.setdefault((E, "onewave"), []).append(label)
        if s.use_w and s.multi:
            for E in sc.SFCY_PADDING_E:
                per_E.setdefault((E, "sfcy"), []).append("sfcy padding")
        for (E, kind), labels in sorted(per_E.items()):
            for mode in ("split", "bf16", "split6"):
                items.append(pytest.param(case, E, kind, mode, id="%s-%d-%s-%s" % (case, E, kind, mode)))
        seen = set()
        for label, _, es, _ in sc.default_edges(case):
            for E in es:
                if E not in seen:
                    seen.add(E)
                    items.append(pytest.param(case, E, "default", "split", id="%s-%d-default-split" % (case, E)))
    return items


@pytest.mark.parametrize("case,E,kind,mode", _dispatch_items())
def test_dispatch_edges(case, E, kind, mode):
    """kind: "onewave" = the forced one-wave variants (item-count limits of the wave split, the path split and the chunk length),
    "sfcy" = the forced multi-wave forward (launch padding), "default" = the automatic choice (*_MIN_EDGES limits)"""
    ck = sc.Checker(case, mode)
    run = Launches(case, E, mode)
    fwd_variant, wg_variant = {"onewave": (1, 1), "sfcy": (2, 1), "default": (0, 0)}[kind]
    _three_launches(ck, run, case, E, kind, fwd_variant, wg_variant)
    ck.done()
