"""The fused optimizer kernels (csrc/optim.hip) through the C ABI -- eqf_sumsq, eqf_adamw_step, eqf_adamw_step_dev -- at the
sizes FlatAdamW never produces: every parameter there is padded to 64 floats, so the scalar tails of sumsq_kernel and
adamw_kernel (n not a multiple of 4) and, below OC20 size, the grid-stride iterations (more than 1024 x 256 and 4096 x 256
float4 groups) run in no other test.  Reference: oracle.optim (adamw_step, clip_coef, ema_update) in float64 numpy on
float32-rounded inputs.  Bound: the figure of tests/test_optim.py, 2e-6 * max(1, |x|), applied per element to p, m, v and the
EMA, and to the sum of squares.  Elements with a NEGATIVE weight decay are skipped (only their EMA moves): their p, m, v must
be bit-identical afterwards.  Every buffer is a fresh allocation (256-byte aligned: the kernels read float4) and is never
offset.

Measured on an MI355X, the worst figure of one run (profiles/graph_edges/figures.txt):
  sumsq 1.2e-7 (n = 1 049 603, randn; 3.1e-7 on the scaled family in another run: the atomics' order varies);
  AdamW p 2.4e-7, ema 3.0e-7, m 1.7e-8, v 2.2e-10 (n = 4 197 379); skipped elements bit-identical; the _dev entry bit-identical
Wall time of this file on an MI355X, one run each (pytest's figure): 3.9 s at the parent commit, 3.9 s with every allocation
of the opted-in tests poisoned and guarded (tests/poison.py).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import optim as ooptim
from poison import guard_input, poisoned_ops  # noqa: E402,F401  (every buffer of this file sits between guard bands)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("poisoned_ops")]

SMALL_N = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025]
SUMSQ_BIG = 1048576 + 1027     # past the 1024-block cap of eqf_sumsq, with a tail of 3
ADAMW_BIG = 4194304 + 3075     # past the 4096-block cap of eqf_adamw_step, with a tail of 3
BOUND = 2e-6
LR, BETA1, BETA2, EPS, EMA_DECAY = 1e-2, 0.9, 0.999, 1e-8, 0.99


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _f32(x):
    """the float32 rounding of a hyper-parameter, as a Python float (what the C ABI receives)"""
    return float(np.float32(x))


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gpu(a):
    # as an [n, 1] column between NaN guard bands (tests/poison.py; a band of 128 one-element rows, at least 4 KiB): the kernels
    # update p, m, v and the EMA in place, so check() sees a store past either end, and a load past the end reads NaN
    t = guard_input(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(_dev()).unsqueeze(1)).squeeze(1)
    assert t.data_ptr() % 256 == 0
    return t


def _rel(got, ref):
    """max over elements of |got - ref| / max(1, |ref|)"""
    got = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())


def _bits(t):
    return t.detach().cpu().numpy().view(np.int32)


# ------------------------------------------------------------------------------------------------- sum of squares
def _sumsq_input(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "randn":
        g = rng.standard_normal(n)
    elif kind == "const":
        g = np.full(n, 0.75)
    else:  # blocks of 37 elements scaled by 1e+3 / 1e-3 in turn
        g = rng.standard_normal(n) * np.where((np.arange(n) // 37) % 2 == 0, 1e3, 1e-3)
    return g.astype(np.float32)


@pytest.mark.parametrize("kind", ["randn", "const", "scaled"])
@pytest.mark.parametrize("n", SMALL_N + [SUMSQ_BIG])
def test_sumsq_edges(n, kind):
    from equiformer_amd.lib import call
    g = _sumsq_input(kind, n, 600 + n % 1000)
    ref = float((g.astype(np.float64) ** 2).sum())
    gd = _gpu(g)
    out = torch.full((1,), 123.0, device=_dev())  # (the entry point zeroes it)
    call("eqf_sumsq", _P(gd), n, _P(out), _stream())
    err = _rel(out, np.array([ref]))
    print("FIG sumsq[n=%d,%s] sumsq err=%.2e yard=- bound=%.2e" % (n, kind, err, BOUND))
    assert err < BOUND


# ------------------------------------------------------------------------------------------------- AdamW
def _wd(n, shift):
    """zero, positive and NEGATIVE entries in turn (period 3, so every float4 group mixes skipped and live lanes and the tail
    of a size that is no multiple of 4 holds a skipped element for one of the shifts)"""
    k = (np.arange(n) + shift) % 3
    return np.where(k == 0, -1.0, np.where(k == 1, 0.0, 0.05)).astype(np.float32)


def _hyper(step):
    """{lr, bc1, bc2_sqrt} as the by-value entry derives them: double arithmetic on the float32 betas, rounded to float32"""
    b1, b2 = _f32(BETA1), _f32(BETA2)
    return np.array([LR, 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step)], dtype=np.float32)


class _State:
    """p, m, v, ema and wd on the GPU plus the float64 reference of the same state"""

    def __init__(self, n, shift, with_ema, seed):
        rng = np.random.default_rng(seed)
        self.n, self.with_ema = n, with_ema
        self.wd = _wd(n, shift)
        self.skip = self.wd < 0
        p0 = rng.standard_normal(n).astype(np.float32)
        m0, v0 = np.zeros(n, np.float32), np.zeros(n, np.float32)
        m0[self.skip], v0[self.skip] = 0.125, 0.375      # never touched: any value must survive bit for bit
        e0 = (p0 + 0.5).astype(np.float32)
        self.p0, self.m0, self.v0 = p0, m0, v0
        self.p, self.m, self.v, self.e = (x.astype(np.float64) for x in (p0, m0, v0, e0))
        self.dp, self.dm, self.dv, self.dwd = _gpu(p0), _gpu(m0), _gpu(v0), _gpu(self.wd)
        self.de = _gpu(e0) if with_ema else None
        self.rng = rng

    def grad(self):
        return (self.rng.standard_normal(self.n) * 0.3).astype(np.float32)

    def reference_step(self, g, step, clip):
        g64 = g.astype(np.float64)
        coef = ooptim.clip_coef([g64], clip)[0] if clip is not None else 1.0
        live = ~self.skip
        p, m, v = ooptim.adamw_step(self.p[live], g64[live] * coef, self.m[live], self.v[live], step, _f32(LR), _f32(BETA1),
                                    _f32(BETA2), _f32(EPS), self.wd[live].astype(np.float64))
        self.p[live], self.m[live], self.v[live] = p, m, v
        self.e = ooptim.ema_update(self.e, self.p, _f32(EMA_DECAY))
        return coef

    def check(self, tag, worst):
        figs = {"p": _rel(self.dp, self.p), "m": _rel(self.dm, self.m), "v": _rel(self.dv, self.v)}
        if self.with_ema:
            figs["ema"] = _rel(self.de, self.e)
        for k, e in figs.items():
            worst[k] = max(worst.get(k, 0.0), e)
        assert all(e < BOUND for e in figs.values()), (tag, figs)
        s = self.skip
        if s.any():
            assert np.array_equal(_bits(self.dp)[s], self.p0.view(np.int32)[s]), "a skipped element's p changed"
            assert np.array_equal(_bits(self.dm)[s], self.m0.view(np.int32)[s]), "a skipped element's m changed"
            assert np.array_equal(_bits(self.dv)[s], self.v0.view(np.int32)[s]), "a skipped element's v changed"


def _step(st, g, step, sumsq, max_norm, dev_entry):
    from equiformer_amd.lib import call
    gd = _gpu(g)
    if dev_entry:
        hyper = _gpu(_hyper(step))
        call("eqf_adamw_step_dev", _P(st.dp), _P(gd), _P(st.dm), _P(st.dv), _P(st.dwd), _P(st.de), _P(sumsq), st.n, _P(hyper),
             BETA1, BETA2, EPS, max_norm, EMA_DECAY, _stream())
    else:
        call("eqf_adamw_step", _P(st.dp), _P(gd), _P(st.dm), _P(st.dv), _P(st.dwd), _P(st.de), _P(sumsq), st.n, LR, BETA1,
             BETA2, EPS, step, max_norm, EMA_DECAY, _stream())
    torch.cuda.synchronize()


def _three_steps(n, shift, with_ema, clip_kind, seed, dev_entry=False):
    """three consecutive steps (m and v are non-zero from the second on) checked against the oracle after each; clip_kind:
    "none" (sumsq is a null pointer), "active" (max_norm = half the gradient norm), "inactive" (ten times the norm)"""
    st = _State(n, shift, with_ema, seed)
    coefs, worst = [], {}
    tag = "adamw[n=%d,wd%d,ema=%d,clip=%s%s]" % (n, shift, with_ema, clip_kind, ",dev" if dev_entry else "")
    for step in (1, 2, 3):
        g = st.grad()
        norm = math.sqrt(float((g.astype(np.float64) ** 2).sum()))
        clip = {"none": None, "active": 0.5 * norm, "inactive": 10.0 * norm}[clip_kind]
        sumsq = _gpu(np.array([norm * norm])) if clip is not None else None
        _step(st, g, step, sumsq, _f32(clip) if clip is not None else 0.0, dev_entry)
        coefs.append(st.reference_step(g, step, _f32(clip) if clip is not None else None))
        try:
            st.check("%s step %d" % (tag, step), worst)
        finally:
            if step == 3 or any(not e < BOUND for e in worst.values()):  # the worst figure of the three steps, printed once
                for k, e in worst.items():
                    print("FIG %s %s err=%.2e yard=- bound=%.2e" % (tag, k, e, BOUND))
    if clip_kind == "active":
        assert all(c < 0.51 for c in coefs)
    elif clip_kind == "inactive":
        assert all(c == 1.0 for c in coefs)
    return st


@pytest.mark.parametrize("clip_kind", ["none", "active", "inactive"])
@pytest.mark.parametrize("with_ema", [False, True], ids=["noema", "ema"])
@pytest.mark.parametrize("n", SMALL_N)
def test_adamw_edges(n, with_ema, clip_kind):
    """every small size, three placements of the skipped elements (so that the tail holds a skipped and a live one in turn)"""
    for shift in (0, 1, 2):
        _three_steps(n, shift, with_ema, clip_kind, 700 + n + shift)


@pytest.mark.parametrize("with_ema,clip_kind", [(True, "active"), (False, "none")])
def test_adamw_grid_stride(with_ema, clip_kind):
    """4 194 304 + 3075 elements: more float4 groups than 4096 x 256 threads, and a tail of three"""
    _three_steps(ADAMW_BIG, 0, with_ema, clip_kind, 800)


@pytest.mark.parametrize("n", [5, 1025])
def test_adamw_dev_entry_gives_the_same_bits(n):
    """{lr, bc1, bc2_sqrt} read from a device array: the same bits as the by-value entry given the same three floats"""
    a = _three_steps(n, 1, True, "active", 900 + n % 1000, dev_entry=False)
    b = _three_steps(n, 1, True, "active", 900 + n % 1000, dev_entry=True)
    for x, y in ((a.dp, b.dp), (a.dm, b.dm), (a.dv, b.dv), (a.de, b.de)):
        assert np.array_equal(_bits(x), _bits(y))
