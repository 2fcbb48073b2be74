"""Plain float64 restatement of the grouped GEMM ABI (TEST INFRASTRUCTURE, not product code).

`ref_group` executes a list of problems stated in the terms of `eqf_gemm_desc` (include/equiformer_hip.h; the comment block
at the head of csrc/gemmx.hip) on flat CPU buffers and returns what every buffer must hold afterwards, together with the
mask of the elements a kernel may write: everything else -- gaps between degree segments, columns past N up to ld, rows
past M, the guard bands -- must come back bit-identical.

  kind 0:  C[i,n] (=|+=) sum_k A[i,k] B[k,n] (+ bias[n])     A: M two-level rows (ra) x K, B plain [K,N] (ldb), C rows (rc)
  kind 1:  C[i,n] (=|+=) sum_k A[i,k] B[n,k] (+ bias[n])     B plain [N,K] (ldb)
  kind 2:  C[m,n] += sum_{i<K} A[i,m] B[i,n]                  A: K two-level rows (ra) x M, B: K two-level rows (rc) x N,
                                                              C plain [M,N] (ldb); bias[n] += sum_i B[i,n]
  kind 3:  as kind 2, bias[m] += sum_i A[i,m]
  two-level row i of (d, ld, inner) starts at (i // d) * ld + (i % d) * inner; a plain matrix is (1, ld, 0).
  Problems with M <= 0 or N <= 0 (kinds 2, 3: or K <= 0) do nothing; kinds 0, 1 with K <= 0 are an argument error.

`ref_split` is the same contraction in the arithmetic a matrix mode promises (operands split into bf16 planes by round to
nearest even, the product terms `mma_terms<NA, NB>` of csrc/sfcx_common.h keeps: plane pairs (i, j) with
i + j <= max(NA, NB) - 1), products and sums in float64: the yardstick of the split modes, computed from the reference alone.

A buffer is a flat float32 tensor whose first and last GUARD elements are guard bands; offsets count from the start of the
tensor.  `ref_group` asserts that every element a problem reads or writes lies inside the bands, so a case that passes here
cannot send a correct kernel out of bounds.
"""
import torch

GUARD = 64
# bf16 planes (A operand, B operand) per matrix mode: rows kinds = activations x weights, tn kinds = two activations
PLANES_ROWS = {"split": (2, 3), "bf16": (1, 1), "split6": (3, 3)}
PLANES_TN = {"split": (2, 2), "bf16": (1, 1), "split6": (3, 3)}


class Prob:
    """One eqf_gemm_desc.  A, B, C, bias: (buffer name, offset in floats) -- bias may be None; ra, rc: (d, ld, inner)."""

    def __init__(self, kind, A, ra, B, ldb, C, rc, bias, M, N, K, accumulate=0):
        self.kind, self.A, self.ra, self.B, self.ldb, self.C, self.rc = kind, A, tuple(ra), B, ldb, C, tuple(rc)
        self.bias, self.M, self.N, self.K, self.accumulate = bias, M, N, K, accumulate

    def empty(self):
        return self.M <= 0 or self.N <= 0 or (self.kind >= 2 and self.K <= 0)


def rows_index(off, r, nrows, ncols):
    """flat indices [nrows, ncols] of a matrix of two-level rows"""
    d, ld, inner = r
    i = torch.arange(nrows)
    return (off + (i // d) * ld + (i % d) * inner)[:, None] + torch.arange(ncols)[None, :]


def index(p):
    """flat indices of the LOGICAL operands of a problem: a [M,K], b [K,N], c [M,N], cs (column sums / bias) or None"""
    if p.kind < 2:
        a = rows_index(p.A[1], p.ra, p.M, p.K)
        b = rows_index(p.B[1], (1, p.ldb, 0), p.K, p.N) if p.kind == 0 else rows_index(p.B[1], (1, p.ldb, 0), p.N, p.K).T
        c = rows_index(p.C[1], p.rc, p.M, p.N)
        cs = None if p.bias is None else p.bias[1] + torch.arange(p.N)
    else:
        a = rows_index(p.A[1], p.ra, p.K, p.M).T
        b = rows_index(p.B[1], p.rc, p.K, p.N)
        c = rows_index(p.C[1], (1, p.ldb, 0), p.M, p.N)
        cs = None if p.bias is None else p.bias[1] + torch.arange(p.N if p.kind == 2 else p.M)
    return a, b, c, cs


class Ref:
    """exp: buffer name -> expected contents (float64); written: name -> bool mask of what a kernel may write;
    outs: (problem number, "C" | "cs", buffer name, flat indices as a matrix [rows, columns]) per output"""

    def __init__(self, exp, written, outs):
        self.exp, self.written, self.outs = exp, written, outs


def ref_group(probs, bufs, contract=None, f32_sums=False):
    exp = {k: v.double().clone() for k, v in bufs.items()}
    written = {k: torch.zeros(v.numel(), dtype=torch.bool) for k, v in bufs.items()}
    outs = []
    for n, p in enumerate(probs):
        assert 0 <= p.kind <= 3 and p.ra[0] >= 1 and p.rc[0] >= 1
        if p.empty():
            continue
        assert p.K >= 1, "kinds 0, 1 with K <= 0 are an argument error"
        ia, ib, ic, ics = index(p)
        for (name, _), ix in ((p.A, ia), (p.B, ib), (p.C, ic), (p.bias or p.C, ic if ics is None else ics)):
            assert GUARD <= int(ix.min()) and int(ix.max()) < bufs[name].numel() - GUARD, (n, name)
        assert ic.unique().numel() == ic.numel(), (n, "output rows overlap")
        a, b = bufs[p.A[0]][ia].double(), bufs[p.B[0]][ib].double()
        prod = a @ b if contract is None else contract(a, b, p.kind)
        C = exp[p.C[0]]
        if p.kind < 2:
            if ics is not None:
                prod = prod + bufs[p.bias[0]][ics].double()[None, :]
            C[ic] = prod + C[ic] if p.accumulate else prod
        else:
            C[ic] = C[ic] + prod
            if ics is not None:
                if f32_sums:
                    a, b = a.float(), b.float()
                exp[p.bias[0]][ics] += (b.sum(0) if p.kind == 2 else a.sum(1)).double()
                written[p.bias[0]][ics] = True
                outs.append((n, "cs", p.bias[0], ics[:, None]))
        written[p.C[0]][ic] = True
        outs.append((n, "C", p.C[0], ic))
    return Ref(exp, written, outs)


def planes(x, n):
    """x (float32 values) as n bf16 planes, each the round-to-nearest-even bf16 of what the planes before left (the
    subtraction in float32, as where the kernels stage their operands); returned as float32 tensors"""
    r = x.float().clone()
    out = []
    for _ in range(n):
        h = r.bfloat16().float()
        out.append(h)
        r = r - h
    return out


def split_contract(mode, acc=torch.float64):
    """contraction a @ b in the arithmetic of `mode`; acc = float32 sums the kept plane products in float32 instead (the
    yardstick of a comparison against ref_split itself)"""

    def contract(a, b, kind):
        na, nb = (PLANES_ROWS if kind < 2 else PLANES_TN)[mode]
        pa, pb = planes(a, na), planes(b, nb)
        top = max(na, nb) - 1
        out = torch.zeros(a.shape[0], b.shape[1], dtype=acc)
        for s in range(top, -1, -1):
            for i in range(na):
                j = s - i
                if 0 <= j < nb:
                    out = out + pa[i].to(acc) @ pb[j].to(acc)
        return out.double()

    return contract


def ref_split(probs, bufs, mode, acc=torch.float64):
    return ref_group(probs, bufs, split_contract(mode, acc))


def ref_f32(probs, bufs):
    """the contraction in plain float32 on the CPU: the yardstick of the exact-fp32 kernels (and, with its float32 column sums, of the bias
    gradients in every mode)"""
    return ref_group(probs, bufs, lambda a, b, kind: (a.float() @ b.float()).double(), f32_sums=True)


# ------------------------------------------------------------------------------------------------- building problems
class Arena:
    """Flat buffers with guard bands, pre-filled with random values EVERYWHERE (guards, gaps, outputs): a kernel that
    writes outside its region changes a value, one that fails to write leaves a wrong one."""

    def __init__(self, seed, integer=False):
        self.gen = torch.Generator().manual_seed(seed)
        self.integer = integer
        self.bufs = {}

    def randn(self, *shape):
        if self.integer:
            return torch.randint(-8, 9, shape, generator=self.gen).float()
        return torch.randn(*shape, generator=self.gen)

    def alloc(self, name, numel, pad=8):
        """a buffer with `numel` (+ pad) floats between its guard bands; returns the offset of its first inner float"""
        assert name not in self.bufs
        self.bufs[name] = self.randn(GUARD + numel + pad + GUARD)
        return GUARD


def span(r, nrows, ncols):
    """floats a matrix of two-level rows reaches from its base"""
    d, ld, inner = r
    last = max(nrows, 1) - 1
    return (last // d) * ld + (d - 1 if nrows >= d else last) * inner + max(ncols, 1) + ld


FAMILIES = ("randn", "scaled", "exact", "ties")


def operands(family, M, K, N, gen):
    """logical a [M,K], b [K,N] (float32) of an input family:
    randn   plain
    scaled  output row i scaled by 10^(i % 7 - 3) (through a), output column n by 10^(n % 7 - 3) (through b)
    exact   a = rows of a permutation-like 0/1 matrix, b = asymmetric multiples of 1/2 below 256: every product and sum
            is exact in fp32 and in three bf16 planes
    ties    a on bf16 ties (1 + odd * 2^-8) at magnitudes 1, 2^-100 (8e-31) and 2^-108 (3e-33: the smallest at which the
            third plane, 2^-16 of the value, is still a normal number) by row i % 3; b small integers: every kept plane
            product and every sum of them is exact in fp32, so a result shows the rounding of the split and nothing else
    """
    if family == "exact":
        a = torch.zeros(M, K)
        a[torch.arange(M), (torch.arange(M) * 5 + 3) % K] = 1.0
        b = ((torch.arange(K * N).view(K, N) % 97) * 0.5 + (torch.arange(K) % 120).float()[:, None]).float()
        return a, b
    if family == "ties":
        odd = 2 * torch.randint(0, 64, (M, K), generator=gen) + 1
        sign = 1.0 - 2.0 * torch.randint(0, 2, (M, K), generator=gen)
        mag = torch.tensor([1.0, 2.0 ** -100, 2.0 ** -108], dtype=torch.float64)[torch.arange(M) % 3]
        a = (sign.double() * (1.0 + odd.double() * 2.0 ** -8) * mag[:, None]).float()
        b = torch.randint(-3, 4, (K, N), generator=gen).float()
        return a, b
    a, b = torch.randn(M, K, generator=gen), torch.randn(K, N, generator=gen)
    if family == "scaled":
        a = a * (10.0 ** (torch.arange(M) % 7 - 3).double())[:, None].float()
        b = b * (10.0 ** (torch.arange(N) % 7 - 3).double())[None, :].float()
    return a, b


def add_problem(ar, tag, kind, M, N, K, d=1, family="randn", c_off=0, a_off=0, b_off=0, ipad=0, lpad=0, bias=True,
                accumulate=0):
    """Allocates the buffers of one problem in arena `ar` and returns its Prob.
    rows kinds: A rows (d, d * (K + ipad) + lpad, K + ipad), C rows (d, d * (N + ipad) + lpad, N + ipad), B plain with
    ldb = its row length + ipad; tn kinds: A: K rows of (d, ..) x M, B: K rows x N, C plain [M, N + ipad].
    *_off: extra floats before the operand (alignment), lpad / ipad: gaps after a node's rows / between degree rows."""
    a, b = operands(family, max(M, 0), max(K, 0), max(N, 0), ar.gen)
    if kind < 2:
        ra = (d, d * (K + ipad) + lpad, K + ipad if d > 1 else 0)
        rc = (d, d * (N + ipad) + lpad, N + ipad if d > 1 else 0)
        ldb = (N if kind == 0 else K) + ipad
        nb = (K if kind == 0 else N) * ldb
        A = (tag + ".A", ar.alloc(tag + ".A", span(ra, M, K) + a_off) + a_off)
        B = (tag + ".B", ar.alloc(tag + ".B", nb + b_off) + b_off)
        C = (tag + ".C", ar.alloc(tag + ".C", span(rc, M, N) + c_off) + c_off)
        bs = (tag + ".bias", ar.alloc(tag + ".bias", N)) if bias else None
    else:
        ra = (d, d * (M + ipad) + lpad, M + ipad if d > 1 else 0)
        rc = (d, d * (N + ipad) + lpad, N + ipad if d > 1 else 0)
        ldb = N + ipad
        A = (tag + ".A", ar.alloc(tag + ".A", span(ra, K, M) + a_off) + a_off)
        B = (tag + ".B", ar.alloc(tag + ".B", span(rc, K, N) + b_off) + b_off)
        C = (tag + ".C", ar.alloc(tag + ".C", max(M, 0) * ldb + c_off) + c_off)
        bs = (tag + ".bias", ar.alloc(tag + ".bias", N if kind == 2 else M)) if bias else None
    p = Prob(kind, A, ra, B, ldb, C, rc, bs, M, N, K, accumulate)
    if not p.empty() and K > 0:
        ia, ib, _, _ = index(p)
        ar.bufs[A[0]][ia] = a
        ar.bufs[B[0]][ib] = b
    return p
