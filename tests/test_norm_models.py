"""Host side of `norm_layer` in {'layer', 'graph', 'instance', 'fast_layer'} [ref: get_norm_layer,
nets/graph_attention_transformer.py:39-51]: every model family constructs with each of them, parameter names / shapes /
registration order and no_weight_decay() equal what the reference's own classes gave (tests/golden/norms/
param_tables.json, written by tests/golden/make_norm_golden.py), the options that are not built refuse at construction
and an unknown name raises the reference's ValueError.  No GPU needed; runs on the GPU machine as well."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_norm_golden as mng  # noqa: E402

NORM_TYPES = list(mng.NORM_TYPES)


def _families():
    from equiformer_amd.nets.dp_attention_transformer import (DotProductAttentionTransformer,
                                                              DotProductAttentionTransformerMD17,
                                                              DotProductAttentionTransformerOC20)
    from equiformer_amd.nets.equiformer_md17_dens import Equiformer_MD17_DeNS
    from equiformer_amd.nets.graph_attention_transformer import GraphAttentionTransformer
    from equiformer_amd.nets.graph_attention_transformer_md17 import GraphAttentionTransformerMD17
    from equiformer_amd.nets.graph_attention_transformer_oc20 import GraphAttentionTransformerOC20
    md17 = dict(irreps_in="64x0e", max_radius=5.0, number_of_basis=32, basis_type="exp")
    return {"qm9": (GraphAttentionTransformer, mng.QM9_KW),
            "md17": (GraphAttentionTransformerMD17, mng.MD17_KW),
            "oc20": (GraphAttentionTransformerOC20, dict(mg.SMALL_OC20, number_of_basis=32)),
            "dp_qm9": (DotProductAttentionTransformer, dict(irreps_in="5x0e", max_radius=5.0, number_of_basis=32, **mg.SMALL_DP_L2)),
            "dp_md17": (DotProductAttentionTransformerMD17, dict(md17, **mg.SMALL_DP_L2)),
            "dp_oc20": (DotProductAttentionTransformerOC20,
                        {k: v for k, v in dict(mg.SMALL_OC20, number_of_basis=32).items() if k != "nonlinear_message"}),
            "dens": (Equiformer_MD17_DeNS, dict(mg.SMALL_DENS))}


@pytest.mark.parametrize("norm_type", NORM_TYPES)
@pytest.mark.parametrize("family", ["qm9", "md17", "oc20", "dp_qm9", "dp_md17", "dp_oc20", "dens"])
def test_every_family_constructs_with_every_norm_type(family, norm_type):
    from equiformer_amd.nets import layers
    cls, kw = _families()[family]
    m = cls(norm_layer=norm_type, **kw)
    want = {"layer": layers.EquivariantLayerNormV2, "graph": layers.EquivariantGraphNorm,
            "instance": layers.EquivariantInstanceNorm, "fast_layer": layers.EquivariantLayerNormFast}[norm_type]
    norms = [m.norm] + [n for blk in m.blocks for n in (blk.norm_1, blk.norm_2)]
    assert all(type(n) is want for n in norms)
    names = [n for n, _ in m.blocks[0].norm_1.named_parameters()]
    assert names == (["mean_shift"] if norm_type == "graph" else []) + ["affine_weight", "affine_bias"]
    if norm_type == "graph":
        assert float(m.norm.mean_shift.detach().min()) == float(m.norm.mean_shift.detach().max()) == 1.0
        assert m.norm.mean_shift.shape == m.norm.affine_bias.shape
    nwd = m.no_weight_decay()
    assert ("blocks.0.norm_1.affine_weight" in nwd) == (norm_type != "fast_layer")


@pytest.mark.parametrize("norm_type", NORM_TYPES)
@pytest.mark.parametrize("family", ["qm9", "md17"])
def test_parameter_tables_and_no_weight_decay_equal_the_reference(family, norm_type):
    cls, kw = _families()[family]
    m = cls(norm_layer=norm_type, **kw)
    ref = mng.load_tables()[norm_type][family]
    got = [[n, list(p.shape)] for n, p in m.named_parameters()]
    assert [n for n, _ in got] == [n for n, _ in ref["params"]]  # names and registration order
    assert got == ref["params"]                                  # shapes
    assert sorted(m.no_weight_decay()) == ref["no_weight_decay"]


def test_fast_layer_has_fewer_no_decay_names_than_layer():
    """the reference's no_weight_decay() lists V2, Instance and Graph but not Fast: 2 names for each of the 5 norms of the
    small QM9 configuration leave its list"""
    t = mng.load_tables()
    assert len(t["layer"]["qm9"]["no_weight_decay"]) == 32 and len(t["fast_layer"]["qm9"]["no_weight_decay"]) == 22
    assert len(t["graph"]["qm9"]["no_weight_decay"]) == 32 + 5 and len(t["instance"]["qm9"]["no_weight_decay"]) == 32


def test_fast_layer_norm_is_not_a_layer_norm_v2():
    from equiformer_amd.nets import layers
    assert not issubclass(layers.EquivariantLayerNormFast, layers.EquivariantLayerNormV2)
    assert layers.get_norm_layer("fast_layer") is layers.EquivariantLayerNormFast
    assert layers.get_norm_layer(None) is None


@pytest.mark.parametrize("kw", [dict(reduce="max"), dict(normalization="norm"), dict(affine=False)])
@pytest.mark.parametrize("name", ["EquivariantGraphNorm", "EquivariantInstanceNorm"])
def test_options_that_are_not_built_refuse_at_construction(name, kw):
    from equiformer_amd.nets import layers
    cls = getattr(layers, name)
    cls("8x0e+4x1e")  # the defaults are built
    with pytest.raises(NotImplementedError):
        cls("8x0e+4x1e", **kw)


def test_unknown_norm_type_raises_the_reference_error():
    from equiformer_amd.nets import layers
    with pytest.raises(ValueError, match="^Norm type batch not supported.$"):
        layers.get_norm_layer("batch")
