"""Host-side planners of the fused SeparableFCTP on E(3) (parity-aware) irreps: consumer segments and DTP paths are matched by
(degree, parity), weights / bias follow the un-fused LinearSpec of the same operator, 0o carries neither the bias nor the
second consumer -- and the SE(3) tables stay what they were (tests/golden/sfc_plan_se3.json, written on the commit before the
planners were keyed on segments by tests/golden/make_sfc_plan_se3.py).  No GPU: only planners run."""
import json
import os

import pytest

from equiformer_amd import lib, ops
from equiformer_amd.layout import DtpTable, RowLayout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SH = "1x0e+1x1o"
OC20_E3 = "256x0e+64x0o+64x1e+64x1o"
OC20_E3_ACT = "448x0e+64x0o+64x1e+64x1o"  # sep_act.lin: scalars + one gate per gated channel | gated segments
# (input irreps, consumer irreps, n2).  The OC20 E(3) model's tensor products all read 256x0e+64x0o+64x1e+64x1o rows (its
# 768x0e+192x0o+192x1e+192x1o rows belong to the FFN, which has no depth-wise tensor product).
E3_CASES = {
    "all_four_32": ("32x0e+32x0o+32x1e+32x1o", "32x0e+32x0o+32x1e+32x1o", 0),
    "unequal": ("64x0e+32x0o+32x1e+64x1o", "64x0e+32x0o+32x1e+64x1o", 0),
    "unequal_n2": ("64x0e+32x0o+32x1e+64x1o", "64x0e+32x0o+32x1e+64x1o", 32),
    "odd_only_degree": ("32x0e+32x1o", "32x0e+32x1o", 0),
    "oc20_value": (OC20_E3, OC20_E3, 0),
    "oc20_act_alpha": (OC20_E3, OC20_E3_ACT, 64),
}


def _spec(case):
    irr, out, n2 = E3_CASES[case]
    table = DtpTable(irr, SH, irr)
    return table, RowLayout(out), ops.SfcSpec(table, RowLayout(out), n2=n2)


@pytest.mark.parametrize("case", sorted(E3_CASES))
def test_e3_operators_are_planned_by_segment(case):
    table, lay, spec = _spec(case)
    n2 = spec.n2
    assert table.has_odd and spec.supported
    npw = {0: 3, 1: 1, 2: 3}
    seg_matrices = sum(K * ncat for (_, K, _, ncat) in spec.degs)
    for mode in (0, 1, 2):
        assert lib.load().eqf_sfcx_supported(table.c_ref, lay.c_ref, n2, mode) > 0, mode
        assert spec.x_mask(mode) & 1, mode
        # forward and data-gradient orientation of every plane of every segment matrix [K, N1 (+ n2 on 0e)]
        assert spec.packed_numel(mode) == 2 * npw[mode] * seg_matrices, mode
    # the un-fused linear of the same operator: same flat weight, same blocks, bias on 0e only
    lin = ops.LinearSpec(table.layout_out, lay)
    assert spec.weight_numel == lin.weight_numel
    assert spec.w_offs == [w_off for (_, _, _, _, _, w_off) in lin.pairs]
    assert [(l, K, N) for (l, K, N, _) in spec.degs] == [(l, K, N) for (l, _, K, _, N, _) in lin.pairs]
    assert spec.bias_dim == lin.bias_dim + n2 == lay.mul_of(0, 1) + n2
    # the second consumer sits on 0e alone; K of a segment = channels of the DTP output of that (degree, parity)
    for (l3, K, N1, ncat), par in zip(spec.degs, spec.pars):
        assert ncat == N1 + (n2 if (l3, par) == (0, 1) else 0)
        assert K == sum(p["mul"] for p in table.paths if (p["l3"], p["p3"]) == (l3, par))
    if n2:
        assert spec.weight2_numel == n2 * table.layout_out.mul_of(0, 1)
    # the parity of every path reaches the library beside its degree
    for i, p in enumerate(table.paths):
        assert table.c.l3[i] == p["l3"] + (lib.EQF_L3_ODD if p["p3"] == -1 else 0)


def test_a_swapped_segment_would_change_shapes():
    """unequal multiplicities: the 0e / 0o and 1e / 1o matrices differ in both dimensions, so a planner that took the blocks of
    one degree in the wrong order could not produce these sizes"""
    _, _, spec = _spec("unequal_n2")
    assert spec.degs == [(0, 128, 64, 96), (0, 64, 32, 32), (1, 128, 32, 32), (1, 160, 64, 64)]
    assert spec.pars == [1, -1, 1, -1] and spec.w_offs == [0, 8192, 10240, 14336]


def test_odd_only_degree_takes_the_odd_paths():
    table, lay, spec = _spec("odd_only_degree")
    assert repr(table.irreps_out) == "64x0e+64x1o" and spec.pars == [1, -1]
    # the same row read as SE(3) irreps (1e instead of 1o) has no producer for its degree-1 segment in this table
    assert not ops.SfcSpec(table, RowLayout("32x0e+32x1e")).supported
    assert ops.DtpLinearSpec.make(table, RowLayout("32x0e+32x1e")) is None and ops.DtpLinearSpec.make(table, lay) is not None
    assert lib.load().eqf_sfcx_supported(table.c_ref, RowLayout("32x0e+32x1e").c_ref, 0, 0) == 0  # no launch can serve it


def test_16_channel_and_six_segment_layouts_stay_unfused():
    small = "32x0e+16x0o+16x1e+16x1o+8x2e+8x2o"  # SMALL_E3_L2 of tests/test_gpu_e3.py
    assert not ops.SfcSpec(DtpTable(small, "1x0e+1x1o+1x2e", small), RowLayout(small)).supported
    six = "32x0e+32x0o+32x1e+32x1o+32x2e+32x2o"
    t6 = DtpTable(six, "1x0e+1x1o+1x2e", six)
    spec = ops.SfcSpec(t6, RowLayout(six))
    assert t6.seg_fusable and not spec.supported and spec.x_mask(0) == 0
    assert lib.load().eqf_sfcx_supported(t6.c_ref, RowLayout(six).c_ref, 0, 0) == 0


def test_e3_modules_take_the_fused_path():
    from equiformer_amd import nets
    from equiformer_amd.nets.layers import GraphAttention
    m = nets.model_entrypoint("oc20_l1_256_e3_nonlinear")(num_layers=1)
    ga = m.blocks[0].ga
    assert ga.act_sfc_spec.supported and ga.sep_value.sfc_spec.supported and m.edge_deg_embed.sfc_spec.supported
    assert ga.sep_act.fused_spec is not None and ga.alpha_fused_spec is not None
    lin = GraphAttention(OC20_E3, "1x0e", SH, OC20_E3, [64, 64], "32x0e+8x0o+8x1e+8x1o", 8, nonlinear_message=False,
                         alpha_drop=0.0, proj_drop=0.0)
    assert lin.lin_sfc_spec.supported and lin.lin_sfc_spec.n2 == 256 and lin.lin_sfc_spec.pars == [1, -1, 1, -1]


def test_se3_plans_did_not_move():
    rows = json.load(open(os.path.join(ROOT, "tests", "golden", "sfc_plan_se3.json")))
    assert len(rows) == 6
    for r in rows:
        table, lay = DtpTable(r["irreps"], r["sh"], r["irreps"]), RowLayout(r["out"])
        spec = ops.SfcSpec(table, lay, n2=r["n2"])
        assert spec.supported == r["supported"], r["out"]
        assert [lib.load().eqf_sfcx_supported(table.c_ref, lay.c_ref, r["n2"], m) for m in (0, 1, 2)] == r["x_mask"], r["out"]
        assert [lib.load().eqf_sfcx_packed_numel(table.c_ref, lay.c_ref, r["n2"], m) for m in (0, 1, 2)] == r["packed_numel"]
        assert [list(d) for d in spec.degs] == r["degs"] and spec.w_offs == r["w_offs"]
        assert (spec.weight_numel, spec.weight2_numel, spec.bias_dim) == (r["weight_numel"], r["weight2_numel"], r["bias_dim"])
        assert [int(table.c.l3[i]) for i in range(table.c.npaths)] == r["l3"]  # plain degrees: no parity flag in SE(3) tables
