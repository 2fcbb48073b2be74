"""Equivariant dropout, the host side (equiformer_amd/dropout.py): `keep_mask` in wrapping numpy arithmetic against the
Python-integer restatement of csrc/rng.h (droppath.rand_uniform) with stream tag 33 and the index (call << 48) | (row << 16) | c,
the range checks, the modules in eval mode / at rate 0 on CPU tensors, the models built with out_drop and proj_drop (same
state_dict keys and parameter order as the zero-rate models), the 100k registration, and the C-ABI entry point in header,
binding table and build -- with its refusals by status, which come back before any launch and need no GPU."""
import ctypes
import math
import os
import re
import struct
import sys

import pytest
import torch

from equiformer_amd import dropout, droppath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
P = 0.4


def _fp32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def _restated(seed, call, rows, n, p, tag=33):
    """the factors one Python integer at a time"""
    inv, p32 = _fp32(1.0 / (1.0 - p)), _fp32(p)
    return torch.tensor([[inv if droppath.rand_uniform(seed, tag, (call << 48) | (r << 16) | c) >= p32 else 0.0
                          for c in range(n)] for r in range(rows)], dtype=torch.float32).view(rows, n)


# -------------------------------------------------------------------------------------------------------------------- keep_mask
def test_keep_mask_pinned_literals():
    """seed 7, call 2, p 0.4, computed from rng.h's formulas with tag 33"""
    m = dropout.keep_mask(7, 2, 37, "12x0e", P)
    assert m.dtype == torch.float32 and m.shape == (37, 12)
    assert int((m > 0).sum()) == 268
    assert (m[0] > 0).int().tolist() == [0, 0, 1, 1, 1, 1, 0, 1, 0, 1, 1, 1]
    assert (dropout.keep_mask(7, 2, 1, "4x0e", P) > 0).int().tolist() == [[0, 0, 1, 1]]
    assert set(m.flatten().tolist()) == {0.0, _fp32(1.0 / (1.0 - P))}
    assert dropout.DROPOUT_TAG == 33 == droppath.DROPPATH_TAG + 1


@pytest.mark.parametrize("seed", [7, 4242, (1 << 64) - 1, 2 ** 62 + 12345])
@pytest.mark.parametrize("rows,irreps", [(37, "12x0e"), (1, "4x0e"), (9, "8x0e+4x1e"), (0, "4x0e")])
def test_keep_mask_equals_the_python_integer_restatement(seed, rows, irreps):
    from equiformer_amd.irreps import Irreps
    n = Irreps(irreps).num_irreps
    for call in (0, 2, (1 << 16) - 1):
        assert torch.equal(dropout.keep_mask(seed, call, rows, irreps, P), _restated(seed, call, rows, n, P)), (seed, call)
    assert torch.equal(dropout.keep_mask(seed + (1 << 64), 2, rows, irreps, P), dropout.keep_mask(seed, 2, rows, irreps, P))


def test_keep_mask_rand_uniform_is_rng_h():
    idx = [0, 1, 5, (2 << 48) | (36 << 16) | 11, (1 << 64) - 1]
    got = dropout.rand_uniform(7, 33, idx).tolist()
    assert got == [droppath.rand_uniform(7, 33, i) for i in idx]


@pytest.mark.parametrize("seed", [7, 4242])
@pytest.mark.parametrize("rows,n", [(37, 12), (64, 192)])
def test_keep_rate(seed, rows, n):
    """|kept / n - (1 - p)| < 3 sqrt(p (1 - p) / n): a binomial share within three standard deviations"""
    m = dropout.keep_mask(seed, 2, rows, "%dx0e" % n, P)
    N = rows * n
    share = float((m > 0).double().mean())
    sd = math.sqrt(P * (1 - P) / N)
    print("seed %d, %d draws: kept %.4f, %.2f standard deviations from %.1f" % (seed, N, share, abs(share - (1 - P)) / sd, 1 - P))
    assert abs(share - (1 - P)) < 3 * sd


def test_keep_mask_depends_on_call_seed_and_tag_but_not_on_the_row_count():
    a = dropout.keep_mask(7, 2, 37, "12x0e", P)
    assert not torch.equal(a, dropout.keep_mask(7, 3, 37, "12x0e", P)), "two calls, one mask"
    assert not torch.equal(a, dropout.keep_mask(8, 2, 37, "12x0e", P)), "two seeds, one mask"
    assert not torch.equal(a, _restated(7, 2, 37, 12, P, tag=32)), "stochastic depth's stream gives the same mask"
    assert torch.equal(dropout.keep_mask(7, 2, 20, "12x0e", P), a[:20]), "the factor of a row depends on the number of rows"
    assert torch.equal(dropout.keep_mask(7, 2, 5, "12x0e", 0.0), torch.ones(5, 12))
    # the channel index counts over all segments: the mask of 8x0e+4x1e is the mask of 12 plain channels
    assert torch.equal(dropout.keep_mask(7, 2, 37, "8x0e+4x1e", P), a)


def test_scalars_only_leaves_every_other_column_at_one():
    irreps = "8x0e+4x0o+4x1e+4x1o"
    full = dropout.keep_mask(7, 2, 37, irreps, P)
    m = dropout.keep_mask(7, 2, 37, irreps, P, scalars_only=True)
    assert torch.equal(m[:, :8], full[:, :8]) and bool((m[:, 8:] == 1.0).all())
    assert bool((full[:, 8:] == 0).any()) and bool((m[:, :8] == 0).any())


def test_expansion_to_rows_in_both_layouts():
    from equiformer_amd.layout import RowLayout
    irreps = "8x0e+4x1e+4x2e"
    lay = RowLayout(irreps)
    m = dropout.keep_mask(7, 2, 9, irreps, P)
    cf = dropout.keep_mask(7, 2, 9, irreps, P, expand="cf")
    e3 = dropout.keep_mask(7, 2, 9, lay, P, expand="e3nn")
    assert cf.shape == e3.shape == (9, lay.dim) and torch.equal(cf, dropout.expand_mask(m, irreps))
    assert torch.equal(cf, e3[:, lay.perm_from_e3nn()])
    # written out: segment s, component k, channel u
    off, c = 0, 0
    for mul, l in lay.segs:
        for k in range(2 * l + 1):
            for u in range(mul):
                assert torch.equal(cf[:, off + k * mul + u], m[:, c + u]) and torch.equal(e3[:, off + u * (2 * l + 1) + k], m[:, c + u])
        off += mul * (2 * l + 1)
        c += mul
    with pytest.raises(ValueError):
        dropout.expand_mask(m, irreps, order="rows")


def test_range_checks():
    for bad in (dict(call=1 << 16), dict(call=-1), dict(p=1.0), dict(p=-0.1), dict(p=1.5), dict(irreps="%dx0e" % (1 << 16))):
        kw = dict(call=0, p=P, irreps="4x0e")
        kw.update(bad)
        with pytest.raises(ValueError):
            dropout.keep_mask(7, kw["call"], 3, kw["irreps"], kw["p"])
        with pytest.raises(ValueError):  # the operator checks its ranges before it looks at the tensor
            dropout.irreps_dropout(torch.zeros(3, 4), kw["irreps"], kw["p"], 7, kw["call"])
    assert dropout.keep_mask(7, (1 << 16) - 1, 1, "%dx0e" % ((1 << 16) - 4), P).shape == (1, (1 << 16) - 4)


def test_cpu_tensor_is_refused():
    from equiformer_amd.ops import HipOnlyError
    with pytest.raises(HipOnlyError):
        dropout.irreps_dropout(torch.zeros(2, 4), "4x0e", P, 7, 0)


# ---------------------------------------------------------------------------------------------------------------------- modules
def test_modules_are_the_identity_in_eval_mode_and_at_rate_zero():
    x = torch.randn(5, 20)
    for cls in (dropout.EquivariantDropout, dropout.EquivariantScalarsDropout):
        m = cls("8x0e+4x1e", P)
        assert not list(m.parameters()) and not list(m.buffers()) and not m.state_dict()
        assert m.eval()(x) is x
        assert cls("8x0e+4x1e", 0.0).train()(x) is x
        assert "drop_prob=0.4" in repr(m) and "8x0e+4x1e" in repr(m)
        with droppath.device_draws(7) as d:
            assert m.eval()(x) is x and d.dropout_calls == 0, "the identity takes no call"
    assert dropout.EquivariantDropout("8x0e+4x1e", P).num_irreps == 12
    assert dropout.EquivariantScalarsDropout.scalars_only and not dropout.EquivariantDropout.scalars_only


def test_modules_take_seed_call_and_word_from_the_scope(monkeypatch):
    """inside `device_draws`: the scope's seed and word, the dropout counter (stochastic depth's stays where it is), nothing from
    the CPU generator; outside: one seed per forward from the CPU generator, call 0, the attention dropout's device word"""
    from equiformer_amd import ops
    calls = []
    monkeypatch.setattr(dropout, "irreps_dropout", lambda x, lay, p, seed, call, word, so: calls.append((p, seed, call, word, so)) or x)
    a, b = dropout.EquivariantDropout("8x0e+4x1e", P).train(), dropout.EquivariantScalarsDropout("8x0e+4x1e", 0.1).train()
    x = torch.ones(3, 20)
    torch.manual_seed(5)
    state = torch.get_rng_state()
    with droppath.device_draws(123) as d:
        d.next_call()
        a(x), b(x), a(x)
        assert (d.calls, d.dropout_calls) == (1, 3)
        with droppath.device_draws(9) as inner:
            b(x)
            assert inner.dropout_calls == 1
        a(x)
    assert torch.equal(torch.get_rng_state(), state)
    assert calls == [(P, 123, 0, None, False), (0.1, 123, 1, None, True), (P, 123, 2, None, False), (0.1, 9, 0, None, True),
                     (P, 123, 3, None, False)]
    del calls[:]
    word = torch.zeros(1, dtype=torch.int64)  # (a CPU stand-in: the module only carries it)
    torch.manual_seed(5)
    with ops.dropout_seed_offset(word):
        a(x)
    b(x)
    state = torch.get_rng_state()
    torch.manual_seed(5)
    s0, s1 = (int(torch.randint(0, 2 ** 62, (1,)).item()) for _ in range(2))
    assert torch.equal(torch.get_rng_state(), state), "one draw per forward"
    assert calls == [(P, s0, 0, word, False), (0.1, s1, 0, None, True)]


def _qm9(cls, cfg, **kw):
    return cls(irreps_in="5x0e", max_radius=5.0, number_of_basis=32, **dict(cfg, **kw))


def _builders():
    import make_golden as mg
    from equiformer_amd.nets import dp_attention_transformer as dp
    from equiformer_amd.nets.equiformer_md17_dens import Equiformer_MD17_DeNS
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    from equiformer_amd.nets.graph_attention_transformer_md17 import GraphAttentionTransformerMD17
    from equiformer_amd.nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20
    md17 = dict(irreps_in="64x0e", max_radius=5.0, number_of_basis=32, basis_type="exp")
    attn = dict(mg.SMALL_L3, irreps_feature=mg.SMALL_L3["irreps_node_embedding"], use_attn_head=True)
    return {
        "qm9": (lambda **kw: _qm9(GraphAttentionTransformer, mg.SMALL_L2, **kw), False),
        "qm9_linear": (lambda **kw: _qm9(GraphAttentionTransformer, dict(mg.SMALL_L2, nonlinear_message=False), **kw), False),
        "qm9_e3": (lambda **kw: _qm9(GraphAttentionTransformer, mg.SMALL_E3_L2, **kw), False),
        "qm9_dp": (lambda **kw: _qm9(dp.DotProductAttentionTransformer, mg.SMALL_DP_L2, **kw), False),
        "md17": (lambda **kw: GraphAttentionTransformerMD17(**dict(md17, **mg.SMALL_L2), **kw), False),
        "md17_attn_head": (lambda **kw: GraphAttentionTransformerMD17(**dict(md17, **attn), **kw), False),
        "md17_dp": (lambda **kw: dp.DotProductAttentionTransformerMD17(**dict(md17, **mg.SMALL_DP_L2), **kw), False),
        "dens": (lambda **kw: Equiformer_MD17_DeNS(**dict(mg.SMALL_DENS, irreps_in="64x0e", max_radius=5.0), **kw), False),
        "oc20": (lambda **kw: GraphAttentionTransformerOC20(None, None, 1, **dict(mg.SMALL_OC20, number_of_basis=32), **kw), True),
        "oc20_aux": (lambda **kw: GraphAttentionTransformerOC20(None, None, 1, use_auxiliary_task=True,
                                                                **dict(mg.SMALL_OC20, number_of_basis=32, irreps_feature="64x0e+32x1e"), **kw), True),
        "oc20_attn": (lambda **kw: GraphAttentionTransformerOC20(None, None, 1, use_attention_head=True, use_auxiliary_task=True,
                                                                 **dict(mg.SMALL_OC20, number_of_basis=32), **kw), True),
        "oc20_dp": (lambda **kw: dp.DotProductAttentionTransformerOC20(None, None, 1, use_auxiliary_task=True,
                                                                      **dict(mg.SMALL_OC20, number_of_basis=32, nonlinear_message=False), **kw), True),
    }


@pytest.mark.parametrize("family", ["qm9", "qm9_linear", "qm9_e3", "qm9_dp", "md17", "md17_attn_head", "md17_dp", "dens", "oc20",
                                    "oc20_aux", "oc20_attn", "oc20_dp"])
def test_models_build_with_both_rates_and_keep_keys_and_parameter_order(family):
    from equiformer_amd.nets import layers
    build, scalars = _builders()[family]
    plain, m = build(), build(out_drop=0.1, proj_drop=0.1)
    assert list(m.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert m.no_weight_decay() == plain.no_weight_decay()
    assert not any(isinstance(x, dropout.EquivariantDropout) for x in plain.modules()) and plain.out_dropout is None
    # out_drop: the scalars variant on the OC20 classes, the per-irrep one elsewhere; sized by the feature
    assert type(m.out_dropout) is (dropout.EquivariantScalarsDropout if scalars else dropout.EquivariantDropout)
    assert m.out_dropout.drop_prob == 0.1 and m.out_dropout.irreps == m.irreps_feature
    # proj_drop: the per-irrep dropout behind the projection of every block's attention and feed-forward network
    for blk in m.blocks:
        for sub in (blk.attention, blk.ffn):
            assert type(sub.proj_drop) is dropout.EquivariantDropout and sub.proj_drop.drop_prob == 0.1
            assert sub.proj_drop.irreps == sub.irreps_node_output
    for blk in plain.blocks:
        assert blk.attention.proj_drop is None and blk.ffn.proj_drop is None
    n = sum(isinstance(x, (layers.GraphAttention, layers.DotProductAttention, layers.FeedForwardNetwork)) and x.proj_drop is not None
            for x in m.modules())
    assert n >= 2 * len(m.blocks)
    if family.startswith("oc20"):  # the OC20 heads are built with proj_drop 0 [ref: graph_attention_transformer_oc20.py:193, :207]
        assert n == 2 * len(m.blocks)


def test_registered_100k_recipe():
    from equiformer_amd import nets
    from equiformer_amd.nets import layers
    assert "oc20_l1_256_nonlinear_aux_100k" in nets.list_models()
    m = nets.model_entrypoint("oc20_l1_256_nonlinear_aux_100k")(num_layers=1)
    assert type(m.out_dropout) is dropout.EquivariantScalarsDropout and m.out_dropout.drop_prob == 0.1
    assert str(m.out_dropout.irreps) == "512x0e+256x1e" and m.use_auxiliary_task
    assert m.alpha_drop == 0.1 and m.blocks[0].ga.alpha_drop == 0.1 and m.auxiliary_head.alpha_drop == 0.1
    assert not any(isinstance(x, layers.GraphDropPath) for x in m.modules())
    assert all(x.proj_drop is None for x in m.modules() if isinstance(x, (layers.GraphAttention, layers.FeedForwardNetwork)))
    base = nets.model_entrypoint("oc20_l1_256_nonlinear_aux")(num_layers=1)
    assert list(m.state_dict()) == list(base.state_dict()) and base.out_dropout is None


# --------------------------------------------------------------------------------------------------------------------- boundary
def test_entry_point_is_declared_bound_and_built():
    from equiformer_amd import build, lib
    header = open(os.path.join(ROOT, "include", "equiformer_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+eqf_irreps_dropout\s*\(([^;{]*?)\)\s*;", text, flags=re.S)
    assert m, "eqf_irreps_dropout is not declared"
    sig = lib.SIGNATURES["eqf_irreps_dropout"]
    assert len([a for a in m.group(1).split(",") if a.strip()]) == len(sig) == 11
    assert sig[3] is lib._P_IRR and sig[7] is lib._u64 and sig[8] is lib.c_fp and sig[9] is lib._u64
    assert "dropout.hip" in build.SOURCES
    before = header[:header.index("int eqf_irreps_dropout(")]
    assert "nets/drop.py:68-108" in before[before.rindex("/*"):]
    # the operator's launch lives in dropout.py: ops.py calls no new entry point
    assert "eqf_irreps_dropout" not in open(os.path.join(ROOT, "equiformer_amd", "ops.py")).read()


def test_refusals_are_return_codes_before_any_launch(hip_lib):
    """every refusal is decided on the host from the descriptor: no GPU is needed to see it (the pointers are never read)"""
    from equiformer_amd import lib
    p, inv = ctypes.c_void_p(256), 1.0 / (1.0 - P)
    ok = lib.make_irreps([(8, 0), (4, 1)])

    def call(x=p, out=p, rows=4, ir=ok, scalars_only=0, c=0):
        return hip_lib.eqf_irreps_dropout(x, out, rows, ctypes.byref(ir) if ir is not None else None, scalars_only, P, inv, 7, None,
                                          c, None)

    assert call(x=None) == call(out=None) == call(ir=None) == -1  # EQF_E_BADARG
    assert call(ir=lib.make_irreps([(6, 0)])) == call(ir=lib.make_irreps([(8, 0), (6, 1)])) == -2  # EQF_E_UNSUPPORTED: mul % 4
    assert call(ir=lib.make_irreps([(6, 1)]), scalars_only=1) == -2, "also on a segment that would only be copied"
    assert call(ir=lib.make_irreps([(1 << 15, 0), (1 << 15, 1)])) == -2  # 2^16 irreps
    assert call(c=1 << 16) == -2
    assert call(rows=0) == call(rows=-3) == 0  # nothing to do: no launch
    assert call(rows=0, ir=lib.make_irreps([(6, 0)])) == -2 and call(rows=0, x=None) == -1, "refusals come before the empty case"
