"""Both GEMM back ends -- csrc/gemmx.hip (eqf_gemmx_group, modes split / bf16 / split6) and csrc/gemm.hip (eqf_gemm_group and
the single-problem eqf_gemm_nn / nt / tn_colsum, mode fp32) -- against the float64 restatement of the descriptor ABI in
tests/fp64_gemm.py, on the SAME descriptors, at every tile, tail and group edge the host dispatch distinguishes.

What a case checks
  * every element OUTSIDE the written region (guard bands of 64 floats, gaps between degree rows and after a node's rows,
    columns past N, rows past M, operands) is bit-identical to before the call;
  * every output per row with `fp64_ops.per_row_rel` (weight gradients per row AND per column, column sums per element)
    against `ref_group`, bound = max(project bound, 4 x yardstick):
      mode fp32                  2e-6 (kinds 0, 1) / 5e-6 (kinds 2, 3: gradients), yardstick = the contraction in float32 on the CPU
      mode split                 those x test_gpu_ops.MODE_TOL["split"] (4), yardstick = ref_split("split") against ref_group
      modes split6 / bf16        test_gpu_gemmx.TOL (3e-6 / 2e-2: MODE_TOL has no entry for them), yardstick = ref_split(mode)
      column sums                5e-6 in every mode (they are taken from the fp32 values), yardstick = float32 sums on the CPU
  * `vs_split`: the split modes ALSO against ref_split(mode) itself, at the fp32 bounds above with the yardstick "the same
    plane products summed in float32 on the CPU".  The kernel and ref_split multiply the same bf16 planes (every product is
    exact in fp32) and differ in the order and width of the additions only, which is what the fp32 bound covers.  This is
    the comparison that sees a dropped weight plane or a lost product term (2^-16 = 1.5e-5 of a product in mode split,
    2^-24 in split6: far below the mode's own bound against ref_group, far above 2e-6 against ref_split).
  * input families (fp64_gemm.operands): randn; "scaled" (rows and columns of 10^-3 .. 10^3: only the per-row metric sees a
    swapped or stale small row); "exact" (0/1 selection x asymmetric half-integers, integer-valued C, bias and targets:
    bit-exact in fp32 and split6; asserted in split too, where a 0/1 operand needs one plane); "ties" (operand on bf16 ties at
    1, 2^-100, 2^-108, compared per magnitude group).

Narrow rows.  With at most 16 compared elements in a row (N = 1, 3, 4, 16; the per-column view of an M = 1 gradient; a
column sum, compared per element) the per-row metric is close to a per-element one: a single cancelling sum is divided by
its own small value, not by the largest of many.  Two things then fall outside "4 x yardstick", and both were measured
(first GPU run, before this rule): (a) the CPU's float32 matmul and sum run >= 16 interleaved partial chains (vector lanes
and blocking), the matrix instructions and the column-sum loops ONE chain per element, so the kernel's rounding error is
that of a chain up to 16 x longer, sqrt(16) = 4 x the yardstick's before any safety factor -- measured err / yard: column
sums 4.8 .. 6.9 (fp32, split, split6 alike: they are fp32 sums in every mode), fp32 C with N = 1 5.3 and 5.7; (b) ref_split sums
the plane products in float64, so its distance from ref_group holds NO accumulation error at all: split6 with N = 1 measured
4.6e-5 against a ref_split yardstick of 1.8e-6, while the fp32 kernel on the same data had 5.2e-5.  For such rows, and only
for them, the factor is 4 x 4 = 16 and the yardstick of a split mode is the larger of err(ref_split) and err(float32
restatement).  Rows of more than 16 elements keep factor 4 and the yardsticks as stated above.

Dispatch conditions are written beside each parametrisation; where the library names its choice through the profiler
(gemm_tn_<BM>x<BN>_mem, gemm_rows_<BM>x<BN>_mem_kn|nk) the test asserts it, otherwise the choice is stated by reasoning
from the host code of eqf_gemmx_group / eqf_gemm_group.

Why these tests bite (one-token mutations of the kernels, by reasoning; none is committed):
  * LoaderKC::commit `e < krem` -> `e <= krem` (gemmx.hip): the first element past a K tail is no longer zeroed but keeps
    what the clamped load brought (A[i, K-1] on the scalar path, A[i, 0] on the VEC path), in the A loader and in kind 1's
    B loader alike, so A[i,K-1] B[n,K-1] (or A[i,0] B[n,0]) is counted twice -> test_rows_generic kind 1, every K that is
    no multiple of 32 (K = 1, 3, 4, 29, 36, 65), every mode of gemmx, error O(1 / sqrt(K)) of a row.
  * LoaderKS::issue without the `wrap` term: rows of the next node are read `ld - d * inner` floats early ->
    test_tn_edges d = 3, 5, 7 (every case with lpad or a row wider than the segment), and test_rows_generic kind 0 whenever
    ldb != 0 (B is walked with d = 1, wrap = ldb: every K > 1).
  * csA `nt == 0` -> `true` (gemmx_tn_kernel): the column sums of A are added once per column tile -> test_tn_edges kind 3
    with N > 64 (N = 65, 130, 260) reads 2x .. 5x the bias gradient.
  * `accumulate` ignored in gx_store_tile16: test_rows_generic cases with accumulate = 1 on the 16-byte path (N % 4 == 0,
    c_off = 0, lpad = 0) and every accumulate case of test_rows_wide lose the pre-filled C (error O(1)).
  * LoaderKS::init `kb / R.d` -> `kb / 1` (the one exact division): test_tn_edges R = 773 with d = 3, 5 and R = 257 with
    d = 7, whose second split starts at rows 224 and 160, no multiples of d.
  * gemm_tn_body `row < g.M` dropped, or gx_store_tile16 without `col0 + c4 < N`: the rows / columns behind the matrix
    change -> the bit-identity check of every partial-tile case.
  * flat_problem loop bound GX_MAXP -> GX_MAXP - 1: problem 23 of test_group_24 is never reached (its C keeps the fill).

Measured on an MI355X, one run, the worst FIG line (largest err / bound) per family and mode; C = against ref_group,
vs = against ref_split(mode), cs = column sums; yard as defined above; * = a narrow row (factor 16):
  rows generic   fp32   C 1.26e-05 yard 2.39e-06 bound 3.83e-05 * (M63 N1 K29 scaled); rows wider than 16: 4.9e-07, bound 2e-06
                 split  C 9.01e-06 yard 8.74e-06 bound 3.50e-05 (M66 N33 K29 d3 scaled); vs 6.97e-06 yard 9.31e-07 bound 1.49e-05 *
                 split6 C 5.03e-07 bound 3e-06 (M65 N68 K65); vs 5.42e-06 yard 6.20e-07 bound 9.91e-06 * (M63 N1 K29)
                 bf16   C 5.09e-03 yard 5.09e-03 bound 2.03e-02; vs 2.05e-07 bound 2e-06
  rows wide      fp32   C 6.19e-07 yard 6.36e-07 bound 2.54e-06 (M8257 K64 N200 scaled)
                 split  C 8.72e-06 yard 8.61e-06 bound 3.45e-05 (M8192 K36 N130 scaled); vs 4.54e-07 bound 2e-06
                 split6 C 4.98e-07 bound 3e-06; vs 4.97e-07 bound 2e-06;  bf16 C 5.78e-03 bound 2.31e-02; vs 2.82e-07
                 group of three: split C 6.71e-06 yard 6.67e-06, vs 4.24e-07; M = 8191 generic against wide: inside 2e-06
  tn             fp32   C 5.24e-05 yard 9.15e-06 bound 1.46e-04 * (R256 d5 M260 N1); cs 1.71e-05 yard 2.63e-06 bound 4.21e-05 *
                 split  C 1.17e-05 yard 1.14e-05 bound 4.58e-05 (R257 d3 M65 N65 scaled); vs 1.17e-06 bound 5e-06;
                        cs 2.36e-05 yard 3.42e-06 bound 5.47e-05 * (R33 M65 N130)
                 split6 C 1.28e-06 bound 3e-06 (R257 d7 M33 N260, per column); vs 1.28e-06 bound 5e-06; cs 1.32e-05 bound 5.47e-05 *
                 bf16   C 5.54e-03 bound 2.21e-02; vs 4.37e-07 bound 5e-06; cs 8.97e-06 bound 5.47e-05 *
  launch_tn      fp32   C 7.06e-07 bound 5e-06, cs 1.58e-06 bound 5e-06;  launch_rows fp32 C 4.71e-07 bound 2e-06
  groups         24 of a kind: split C 3.97e-06 yard 3.88e-06, vs 8.16e-07; split6 vs 4.16e-06 yard 3.32e-07 bound 5.32e-06 *
                 (kind 2, N = 3); fp32 C 4.94e-07.  Empty problems + all kinds: fp32 cs 2.00e-05 yard 4.63e-06 bound 7.42e-05 *,
                 split C 5.78e-06 yard 5.64e-06.  Chunking 25 / 49 / 9: split C 1.14e-05 yard 1.11e-05, fp32 C 7.62e-07.
  exact family   err 0 in fp32, split and split6 (bit-equal), all four kinds;  ties: bf16 C 6.08e-03 = its yardstick (2^-108 rows)
Every mode's C figure sits ON its ref_split yardstick (split 9.0e-06 against 8.7e-06): the kernels deliver the arithmetic
they promise, and `vs` (2e-07 .. 1e-06 on rows wider than 16) is the accumulation alone.  test_gpu_gemmx.TOL["split"] stays
2e-5: the worst per-row split figure here is 1.17e-05, and 4 x that is above any tighter value.
Wall time of this file: 102 tests in 5.4 s, in the same run as tests/test_gpu_op_edges.py (123 tests in 6.3 s).
"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_gemm as fg  # noqa: E402
import fp64_ops as fo  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = ("fp32", "split", "bf16", "split6")
MODE_ID = {"split": 0, "bf16": 1, "split6": 2}
BASE = {0: 2e-6, 1: 2e-6, 2: 5e-6, 3: 5e-6}  # the project's fp32 bounds: forward / gradients (tests/test_gpu_ops.py)
CS_BOUND = 5e-6
NARROW, NARROW_FACTOR = 16, 16.0  # rows of at most 16 compared elements: see "Narrow rows" at the head of this file


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _mode_bound(mode, kind):
    if mode == "fp32":
        return BASE[kind]
    if mode == "split":
        from test_gpu_ops import MODE_TOL
        return BASE[kind] * MODE_TOL["split"]
    from test_gpu_gemmx import TOL
    return TOL[mode]


class _Checker:
    """collects every comparison of a test, prints its figures and fails at the end, so that one run shows them all"""

    def __init__(self, case):
        self.case, self.bad, self.worst = case, [], {}

    def cmp(self, name, got, ref, bound, y32=None, y_chain=None):
        """y_chain: the float32 restatement, a second yardstick for NARROW rows only (see the head of this file)"""
        assert torch.isfinite(got).all(), (self.case, name, "not finite")
        err = fo.per_row_rel(got, ref)
        yard = fo.per_row_rel(y32, ref) if y32 is not None else None
        factor = 4.0
        if yard is not None and got.dim() == 2 and got.shape[1] <= NARROW:
            factor = NARROW_FACTOR
            if y_chain is not None:
                yard = max(yard, fo.per_row_rel(y_chain, ref))
        lim = bound if yard is None else max(bound, factor * yard)
        w = self.worst.get(name)
        if w is None or err / lim > w[0] / w[2]:
            self.worst[name] = (err, yard, lim)
        if not err < lim:
            self.bad.append((name, err, yard, lim))

    def done(self):
        for name, (err, yard, lim) in self.worst.items():
            print("FIG %s %s err=%.2e yard=%s bound=%.2e" % (self.case, name, err,
                                                              "-" if yard is None else "%.2e" % yard, lim))
        assert not self.bad, (self.case, self.bad)


def _descs(probs, dev):
    from equiformer_amd import ops
    from equiformer_amd.lib import EqfGemmDesc

    def ptr(h):
        return None if h is None else ops._p(dev[h[0]], h[1])

    return [EqfGemmDesc(ptr(p.A), ptr(p.B), ptr(p.C), ptr(p.bias), ops.rows(*p.ra), ops.rows(*p.rc), p.ldb, p.M, p.N, p.K,
                        p.accumulate, p.kind) for p in probs]


def _launch_group(mode, descs):
    """eqf_gemm_group (at most 8 problems per call) or eqf_gemmx_group (24) on the descriptors as they are"""
    from equiformer_amd import ops
    from equiformer_amd.lib import EqfGemmDesc, call
    cap = 8 if mode == "fp32" else 24
    for i in range(0, len(descs), cap):
        chunk = descs[i:i + cap]
        arr = (EqfGemmDesc * len(chunk))(*chunk)
        if mode == "fp32":
            call("eqf_gemm_group", arr, len(chunk), ops._stream())
        else:
            call("eqf_gemmx_group", arr, len(chunk), MODE_ID[mode], ops._stream())


class _Refs:
    """the references of one set of problems, computed once and shared by the modes"""

    def __init__(self, probs, bufs):
        self.probs, self.bufs = probs, bufs
        self.ref, self.f32 = fg.ref_group(probs, bufs), fg.ref_f32(probs, bufs)
        self._split = {}

    def split(self, mode):
        if mode not in self._split:
            self._split[mode] = (fg.ref_split(self.probs, self.bufs, mode),
                                 fg.ref_split(self.probs, self.bufs, mode, torch.float32))
        return self._split[mode]


def _check(ck, mode, R, got, family="randn", tag=""):
    for name, init in R.bufs.items():  # everything outside the written region: bit-identical
        keep = ~R.ref.written[name]
        same = torch.equal(got[name][keep].view(torch.int32), init[keep].view(torch.int32))
        assert same, (ck.case, mode, name, "changed outside the written region at",
                      (got[name].view(torch.int32) != init.view(torch.int32)).logical_and(keep).nonzero()[:8].flatten().tolist())
    for n, what, name, ix in R.ref.outs:
        kind = R.probs[n].kind
        g, r = got[name][ix], R.ref.exp[name][ix]
        q = "%s%s.k%d.%s" % (tag, mode, kind, what)
        if what == "cs":
            ck.cmp(q, g, r, CS_BOUND, R.f32.exp[name][ix])
            continue
        f32 = R.f32.exp[name][ix]
        if mode == "fp32":
            yard, views = f32, [("", g, r, None)]
        else:
            s64, s32 = R.split(mode)
            yard, views = s64.exp[name][ix], [("", g, r, None), (".vs_split", g, s64.exp[name][ix], s32.exp[name][ix])]
        for suffix, a, b, y in views:
            bound, y, yc = (_mode_bound(mode, kind), yard, f32) if suffix == "" else (BASE[kind], y, None)
            if family == "ties":  # per magnitude group of rows: 1, 2^-100, 2^-108
                for m in range(min(3, a.shape[0])):
                    ck.cmp(q + suffix + ".mag%d" % m, a[m::3], b[m::3], bound, y[m::3], None if yc is None else yc[m::3])
                continue
            ck.cmp(q + suffix, a, b, bound, y, yc)
            if kind >= 2:  # weight gradients: per column too
                ck.cmp(q + suffix + ".T", a.T, b.T, bound, y.T, None if yc is None else yc.T)
        if family == "exact" and mode != "bf16":
            assert torch.equal(g, r.float()), (ck.case, q, "not exact")


def _run(ck, probs, bufs, modes=MODES, family="randn", launch=_launch_group, tag=""):
    dev = _dev()
    R = _Refs(probs, bufs)
    out = {}
    for mode in modes:
        d = {k: v.to(dev) for k, v in bufs.items()}
        launch(mode, _descs(probs, d))
        torch.cuda.synchronize()
        out[mode] = {k: v.cpu() for k, v in d.items()}
        _check(ck, mode, R, out[mode], family, tag)
    return R, out


def _bits(i):
    return (i * 2654435761 >> 7) & 0xFFFF


# ------------------------------------------------------------------------------------------------- rows, generic kernel
# gemmx_rows_kernel<MODE, BKIND, VEC> (eqf_gemmx_group, kinds 0 and 1; M < 8192 keeps the wide kernel out):
#   VEC loaders      K % 4 == 0 and A 16-byte aligned with ld % 4 == inner % 4 == 0 (kind 1: B too) for EVERY problem of the kind
#   16-byte epilogue (C.ld | C.inner | N) % 4 == 0 and the C base 16-byte aligned, per problem; else the scalar epilogue
#   tiles            64 x 64, K steps of 32: M = 63 / 64 / 65 / 129, N = 64 / 68, K = 29 / 32 / 36 / 65 straddle them
# gemm_rows_group_kernel (eqf_gemm_group): <128, 32> tiles when every N of the kind is <= 32, else <64, 64>.
# Both kinds of a case go in ONE call (one launch per kind).
_MS, _NS, _KS = (1, 31, 63, 64, 65, 129), (1, 3, 4, 33, 64, 68), (1, 3, 4, 29, 32, 36, 65)
ROWS_CASES = []
for _i in range(42):  # all 36 (M, N) pairs, all 42 (M, K) pairs, 36 of the 42 (N, K) pairs
    _b = _bits(_i)
    ROWS_CASES.append(dict(M=_MS[_i % 6], N=_NS[(_i // 6 + _i) % 6], K=_KS[(_i + 3 * (_i // 6)) % 7], d=1, c_off=2 * (_b & 1),
                           lpad=2 * (_b >> 1 & 1), ipad=0, bias=bool(_b >> 2 & 1), acc=_b >> 3 & 1,
                           family=("randn", "scaled")[_b >> 4 & 1]))
for _j, (_d, _n) in enumerate((d, n) for d in (3, 5, 7) for n in (13, 22, 43)):  # a tile edge inside a node
    _b = _bits(100 + _j)
    ROWS_CASES.append(dict(M=_n * _d, N=_NS[(_j + 2) % 6], K=_KS[(2 * _j + 1) % 7], d=_d, c_off=2 * (_b & 1), lpad=2 * (_b >> 1 & 1),
                           ipad=(0, 4, 2)[_j % 3], bias=bool(_b >> 2 & 1), acc=_b >> 3 & 1, family=("randn", "scaled")[_j % 2]))
# the fully aligned paths named: VEC loaders + 16-byte stores with a partial last tile, accumulate on and off, d = 1 and 3
ROWS_CASES += [dict(M=65, N=68, K=36, d=1, c_off=0, lpad=0, ipad=0, bias=True, acc=1, family="scaled"),
               dict(M=129, N=64, K=32, d=1, c_off=0, lpad=4, ipad=0, bias=False, acc=0, family="randn"),
               dict(M=3 * 43, N=68, K=36, d=3, c_off=0, lpad=4, ipad=4, bias=True, acc=1, family="scaled"),
               dict(M=3 * 22, N=4, K=4, d=3, c_off=0, lpad=0, ipad=0, bias=True, acc=0, family="randn")]


def _rows_id(c):
    return "M%d-N%d-K%d-d%d-c%d-l%d-i%d-b%d-a%d-%s" % (c["M"], c["N"], c["K"], c["d"], c["c_off"], c["lpad"], c["ipad"], c["bias"],
                                                       c["acc"], c["family"])


@pytest.mark.parametrize("c", ROWS_CASES, ids=_rows_id)
def test_rows_generic(c):
    ar = fg.Arena(1000 + c["M"] + 7 * c["N"] + 31 * c["K"])
    probs = [fg.add_problem(ar, "k%d" % kind, kind, c["M"], c["N"], c["K"], d=c["d"], family=c["family"], c_off=c["c_off"],
                            lpad=c["lpad"], ipad=c["ipad"], bias=c["bias"], accumulate=c["acc"]) for kind in (0, 1)]
    ck = _Checker("rows[%s]" % _rows_id(c))
    _run(ck, probs, ar.bufs, family=c["family"])
    ck.done()


# ------------------------------------------------------------------------------------------------- rows, wide kernel
# gemmx_rows_wide_kernel (eqf_gemmx_group: `wide_ok`): kind 1, K <= 64, K % 4 == 0, A and B 16-byte aligned, M >= 8192,
# N >= 128, for every problem of the kind; grid (max row tiles, 1, problems).  M = 8191 takes gemmx_rows_kernel<., 1, true>.
# Its scalar epilogue: N % 4 != 0 (130) or a C base off by 2 floats; two-level rows: d = 3 (8193 = 3 * 2731); nkt / kv zeroing:
# K = 4, 20, 36.  In mode fp32 the same descriptors run gemm_rows_group_kernel<64, 64>.
WIDE_CASES = [(8191, 4, 128, 1, 0, 0, "randn"), (8192, 20, 130, 1, 0, 1, "scaled"), (8193, 36, 196, 3, 0, 0, "randn"),
              (8257, 64, 200, 1, 0, 1, "scaled"), (8192, 64, 128, 1, 2, 1, "randn"), (8193, 4, 200, 3, 2, 0, "scaled"),
              (8257, 20, 196, 1, 0, 0, "randn"), (8192, 36, 130, 1, 0, 0, "scaled"), (8192, 64, 196, 1, 0, 0, "exact")]


@pytest.mark.parametrize("M,K,N,d,c_off,acc,family", WIDE_CASES)
def test_rows_wide(M, K, N, d, c_off, acc, family):
    ar = fg.Arena(2000 + M + K + N, integer=family == "exact")
    p = fg.add_problem(ar, "w", 1, M, N, K, d=d, family=family, c_off=c_off, bias=True, accumulate=acc)
    ck = _Checker("wide[M%d,K%d,N%d,d%d,c%d,a%d,%s]" % (M, K, N, d, c_off, acc, family))
    _run(ck, [p], ar.bufs, family=family)
    ck.done()


def test_rows_wide_group_and_generic_agree():
    """Three problems of different M on the (max tiles, 1, n) grid of the wide kernel (`if (m0 >= P.M) return`), d = 3 in the
    middle; and the same data at M = 8191 (generic kernel) against rows 0..8190 of M = 8192 (wide kernel): both within the
    bound of the reference, and of each other."""
    ar = fg.Arena(2100)
    probs = [fg.add_problem(ar, "g0", 1, 8192, 128, 64, family="scaled"),
             fg.add_problem(ar, "g1", 1, 12288, 132, 36, d=3, family="randn", accumulate=1),
             fg.add_problem(ar, "g2", 1, 8200, 130, 20, family="scaled", bias=False)]
    ck = _Checker("wide_group")
    _, out = _run(ck, probs, ar.bufs, modes=("split", "split6", "fp32"))
    p = probs[0]
    short = [fg.Prob(1, p.A, p.ra, p.B, p.ldb, p.C, p.rc, p.bias, 8191, p.N, p.K)]
    bufs = {k: ar.bufs[k] for k in ("g0.A", "g0.B", "g0.C", "g0.bias")}
    R, out1 = _run(ck, short, bufs, modes=("split", "split6"), tag="M8191.")
    ix = R.ref.outs[0][3]
    for mode in ("split", "split6"):
        ck.cmp("%s.generic_vs_wide" % mode, out1[mode]["g0.C"][ix], out[mode]["g0.C"][ix].double(), BASE[1])
    ck.done()


# ------------------------------------------------------------------------------------------------- weight gradients
# gemmx_tn_kernel / gemm_tn_group_kernel (kinds 2, 3; K = reduction rows R): 32 rows per step, split over the grid with
# ksplit = min(1024 / tiles, ceil(steps / 8)), steps_per_split = ceil(steps / ksplit):
#   R <= 256 one split (R = 1, 7, 31: under one step; 33: a one-row second step); R = 257: 9 steps, 2 splits of 5 (the second
#   starts at row 160: 160 % 7 = 6, 160 % 3 = 1); R = 8 * 32 * 3 + 5 = 773: 25 steps, 4 splits of 7 (224 % 3 = 2, 224 % 5 = 4).
#   LoaderKS::init divides once at the split start, then the (q, rem) walk wraps every d rows; column sums only where
#   nt == 0 (kind 3: of A) / mt == 0 (kind 2: of B); the targets are pre-filled with randn and ADDED to.
TN_CASES = [(1, 1, 1, 1, True), (7, 3, 32, 33, True), (31, 5, 33, 64, False), (32, 7, 64, 65, True), (33, 1, 65, 130, True),
            (255, 3, 130, 32, True), (256, 5, 260, 1, False), (257, 7, 33, 260, True), (773, 3, 65, 33, True),
            (773, 5, 130, 130, True), (257, 1, 1, 260, True), (773, 1, 64, 64, False), (7, 7, 260, 260, True),
            (257, 3, 65, 65, True)]


@pytest.mark.parametrize("R,d,M,N,cs", TN_CASES)
def test_tn_edges(R, d, M, N, cs):
    j = TN_CASES.index((R, d, M, N, cs))
    family = ("randn", "scaled")[j % 2]
    ar = fg.Arena(3000 + j)
    probs = [fg.add_problem(ar, "k%d" % kind, kind, M, N, R, d=d, family=family, lpad=(0, 4, 2)[j % 3], ipad=(0, 0, 4, 1)[j % 4],
                            c_off=2 * (j & 1), bias=cs) for kind in (2, 3)]
    ck = _Checker("tn[R%d,d%d,M%d,N%d,cs%d,%s]" % (R, d, M, N, cs, family))
    _run(ck, probs, ar.bufs, family=family)
    ck.done()


def _prof(fn, flt="gemm"):
    from equiformer_amd import lib
    lib.prof_enable(flt)
    try:
        fn()
        torch.cuda.synchronize()
        return lib.prof_report()
    finally:
        lib.prof_enable(None)


# launch_tn (csrc/gemm.hip, the single-problem entry): BM = 32 iff M % 64 != 0 and M < 256, the same for BN -> four kernels
@pytest.mark.parametrize("M,N,name", [(64, 300, "gemm_tn_64x64_mem"), (300, 40, "gemm_tn_64x32_mem"),
                                      (40, 64, "gemm_tn_32x64_mem"), (40, 40, "gemm_tn_32x32_mem")])
def test_fp32_launch_tn_tile_variants(M, N, name):
    """eqf_gemm_tn_colsum with BOTH column sums, R = 257 rows of d = 3 (two splits), targets pre-filled; the kernel the host
    chose is read from the profiler"""
    from equiformer_amd import ops
    from equiformer_amd.lib import call
    ar = fg.Arena(3100 + M + N)
    p = fg.add_problem(ar, "t", 2, M, N, 257, d=3, family="scaled", lpad=4, bias=True)
    csA = ("t.csA", ar.alloc("t.csA", M))
    twin = fg.Prob(3, p.A, p.ra, p.B, p.ldb, ("t.C", p.C[1]), p.rc, csA, M, N, 257)  # the same C: reference = C + 2 A^T B
    ck = _Checker("launch_tn[%d,%d]" % (M, N))

    def launch(mode, descs):
        d = descs[0]

        def go():
            for _ in range(2):  # twice into the same target: kind 2 + kind 3 of the reference, and += onto a non-zero C
                call("eqf_gemm_tn_colsum", d.A, d.ra, d.B, d.rc, d.C, d.ldb, M, N, 257, descs[1].bias if _ else None,
                     None if _ else d.bias, ops._stream())
        rep = _prof(go)
        assert list(rep) == [name] and rep[name]["launches"] == 2, rep

    _run(ck, [p, twin], ar.bufs, modes=("fp32",), family="scaled", launch=launch)
    ck.done()


# launch_rows (csrc/gemm.hip): BN = 128 / 64 / 32 by N > 64 / > 32; BM = 64 when BN >= 64 (and fewer than 4096 tiles of 128
# rows: every shape a test can afford), else 128.  The <128, 128> and <128, 64> tiles need 4096 row tiles and stay unlaunched.
@pytest.mark.parametrize("N,name", [(33, "gemm_rows_64x64_mem"), (68, "gemm_rows_64x128_mem"), (4, "gemm_rows_128x32_mem")])
def test_fp32_launch_rows_tile_variants(N, name):
    from equiformer_amd import ops
    from equiformer_amd.lib import call
    ar = fg.Arena(3200 + N)
    probs = [fg.add_problem(ar, "k%d" % kind, kind, 3 * 43, N, 29, d=3, family="scaled", c_off=2, bias=True, accumulate=kind)
             for kind in (0, 1)]
    ck = _Checker("launch_rows[N%d]" % N)

    def launch(mode, descs):
        def go():
            for d, fn in zip(descs, ("eqf_gemm_nn", "eqf_gemm_nt")):
                call(fn, d.A, d.ra, d.B, d.ldb, d.C, d.rc, d.bias, d.M, d.N, d.K, d.accumulate, ops._stream())
        rep = _prof(go)
        assert sorted(rep) == [name + "_kn", name + "_nk"], rep

    _run(ck, probs, ar.bufs, modes=("fp32",), family="scaled", launch=launch)
    ck.done()


# ------------------------------------------------------------------------------------------------- input families
@pytest.mark.parametrize("family", ["exact", "ties"])
def test_exact_and_tie_operands_all_kinds(family):
    """all four kinds in ONE call.  "exact": bit-equal to the reference in fp32, split and split6 (every value an integer or a
    half below 2^24).  "ties": no bias, nothing accumulated, so that `vs_split` is the split's rounding alone, per magnitude."""
    ar = fg.Arena(4000, integer=True)
    ex = family == "exact"
    probs = [fg.add_problem(ar, "a", 0, 65, 33, 36, family=family, bias=ex, accumulate=int(ex)),
             fg.add_problem(ar, "b", 1, 66, 68, 29, d=3, family=family, bias=ex, lpad=4),
             fg.add_problem(ar, "c", 0, 129, 64, 65, family=family, bias=False),
             fg.add_problem(ar, "d", 2, 33, 65, 257, d=7, family=family, bias=ex),
             fg.add_problem(ar, "e", 3, 130, 33, 773, d=3, family=family, bias=ex)]
    if not ex:  # targets of the weight gradients: zero, so that a magnitude group is not swamped by the fill
        for p in probs[3:]:
            ar.bufs[p.C[0]].zero_()
    ck = _Checker("family[%s]" % family)
    _run(ck, probs, ar.bufs, family=family)
    ck.done()


# ------------------------------------------------------------------------------------------------- groups
def _mixed(ar, i, kind, M=None):
    """problem i of a mixed group: small, every shape different"""
    Ms, Ns, Ks, ds = (65, 31, 129, 64, 1, 70), (33, 64, 3, 68, 16), (29, 32, 36, 4, 65, 3, 1), (1, 3, 5, 1, 7)
    d = ds[i % 5]
    m = (Ms[i % 6] // d + 1) * d if M is None else M
    if kind < 2:
        return fg.add_problem(ar, "p%d" % i, kind, m, Ns[i % 5], Ks[i % 7], d=d, family=("randn", "scaled")[i % 2],
                              c_off=2 * (i % 3 == 1), lpad=4 * (i % 2), bias=i % 3 != 0, accumulate=i % 2)
    return fg.add_problem(ar, "p%d" % i, kind, m, Ns[i % 5], 40 * (i % 7) + 7 if M is None or M > 0 else 50, d=d,
                          family=("randn", "scaled")[i % 2], lpad=4 * (i % 2), bias=i % 3 != 0)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_group_24_problems_of_one_kind(kind):
    """exactly GX_MAXP = 24 problems in one launch of eqf_gemmx_group: flat_problem must reach problem 23 (woff[23]); in mode
    fp32 the same list goes in three calls of 8 (MAX_GROUP)"""
    ar = fg.Arena(5000 + kind)
    probs = [_mixed(ar, i, kind) for i in range(24)]
    ck = _Checker("group24[k%d]" % kind)
    _run(ck, probs, ar.bufs, modes=("split", "split6", "fp32"))
    ck.done()


def test_group_with_empty_problems_and_all_kinds():
    """24 descriptors of all four kinds, three of them with M = 0 in the middle (an empty batch), one weight gradient with
    K = 0 rows: skipped on the host, the problems behind them still land in their own buffers"""
    ar = fg.Arena(5100)
    probs = [_mixed(ar, i, i % 4, M=0 if i in (5, 11, 18) else None) for i in range(23)]
    k0 = _mixed(ar, 23, 2)
    k0.K = 0
    ck = _Checker("group_empty")
    R, _ = _run(ck, probs + [k0], ar.bufs)
    for i in (5, 11, 18, 23):
        assert not R.ref.written["p%d.C" % i].any()
    ck.done()


@pytest.mark.parametrize("mode,n", [("split", 25), ("split", 49), ("fp32", 9)])
def test_gemm_group_chunking(mode, n):
    """ops._gemm_group cuts a list into calls of 24 (gemmx) / 8 (fp32): one problem more than one and two full calls"""
    from equiformer_amd import ops
    ar = fg.Arena(5200 + n)
    probs = [_mixed(ar, i, (0, 1, 2)[i % 3]) for i in range(n)]
    ck = _Checker("chunk[%s,%d]" % (mode, n))

    def launch(mode, descs):
        with ops.matrix_mode(mode):
            ops._gemm_group(descs, ops._stream())

    _run(ck, probs, ar.bufs, modes=(mode,), launch=launch)
    ck.done()


@pytest.mark.parametrize("kind", [0, 1])
def test_one_unaligned_problem_makes_the_group_scalar(kind):
    """`vec_ok = 0` for the whole launch when one problem has K % 4 != 0 (K = 29) or an A base off by 2 floats: its aligned
    neighbours (K = 32, 36) then take the scalar loaders too"""
    ar = fg.Arena(5300 + kind)
    probs = [fg.add_problem(ar, "a", kind, 65, 64, 32, family="scaled"),
             fg.add_problem(ar, "b", kind, 66, 33, 29, d=3, family="randn"),
             fg.add_problem(ar, "c", kind, 129, 68, 36, family="scaled", accumulate=1),
             fg.add_problem(ar, "d", kind, 64, 64, 32, family="randn", a_off=2)]
    ck = _Checker("unaligned[k%d]" % kind)
    _run(ck, probs[:3], ar.bufs)
    _run(ck, [probs[0], probs[3], probs[2]], ar.bufs, tag="base.")
    ck.done()


@pytest.mark.parametrize("wide_n", [96, 32])
@pytest.mark.parametrize("kind", [0, 1])
def test_fp32_group_tiles_follow_the_widest_problem(kind, wide_n):
    """eqf_gemm_group takes <64, 64> tiles when ANY problem of the kind has N > 32, else <128, 32>: an N = 16 problem with more
    rows than its neighbour rides on the (max row tiles, max column tiles, n) grid of either"""
    ar = fg.Arena(5400 + kind + wide_n)
    probs = [fg.add_problem(ar, "narrow", kind, 3 * 43, 16, 36, d=3, family="scaled", accumulate=1),
             fg.add_problem(ar, "widest", kind, 31, wide_n, 29, family="randn")]
    ck = _Checker("fp32_tiles[k%d,N%d]" % (kind, wide_n))
    _run(ck, probs, ar.bufs, modes=("fp32", "split"))
    ck.done()


# ------------------------------------------------------------------------------------------------- argument checks
def test_k_below_one_is_refused_before_any_launch():
    """kinds 0 and 1 with K <= 0: EQF_E_BADARG from both back ends and from eqf_gemm_nn / nt, and NOTHING is launched -- the
    valid problem in front of the bad one leaves its C untouched.  (The loaders of gemmx.hip clamp to k = K - 1: with K = 0
    they would read in front of the row.)  M <= 0 and N <= 0 stay empty problems with status 0."""
    from equiformer_amd import ops
    from equiformer_amd.lib import HipLibraryError, call
    ar = fg.Arena(6000)
    good = fg.add_problem(ar, "good", 2, 33, 33, 40)
    good1 = fg.add_problem(ar, "good1", 1, 33, 33, 36)
    bad = fg.add_problem(ar, "bad", 0, 33, 33, 4)
    dev = {k: v.to(_dev()) for k, v in ar.bufs.items()}
    for k in (0, -1):
        bad.K = k
        for kind in (0, 1):
            bad.kind = kind
            descs = _descs([good1, good, bad], dev)
            for mode in MODES:
                with pytest.raises(HipLibraryError):
                    _launch_group(mode, descs)
            d = descs[2]
            with pytest.raises(HipLibraryError):
                call("eqf_gemm_nn" if kind == 0 else "eqf_gemm_nt", d.A, d.ra, d.B, d.ldb, d.C, d.rc, d.bias, d.M, d.N, k, 0,
                     ops._stream())
    bad.K, bad.kind = 4, 0
    for field in ("M", "N"):
        old = getattr(bad, field)
        setattr(bad, field, 0)
        for mode in MODES:
            _launch_group(mode, _descs([bad], dev))
        setattr(bad, field, old)
    torch.cuda.synchronize()
    for name, init in ar.bufs.items():
        assert torch.equal(dev[name].cpu().view(torch.int32), init.view(torch.int32)), name
