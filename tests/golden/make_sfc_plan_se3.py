"""Writes tests/golden/sfc_plan_se3.json: what the host-side planners of the fused SeparableFCTP answer for the SE(3)
operators tests/test_sfcx_plan.py builds -- `supported`, the launch mask of eqf_sfcx_supported and eqf_sfcx_packed_numel in
the three matrix modes, weight sizes and offsets.  tests/test_sfc_e3_plan.py holds the planners to these values: keying them
on (degree, parity) segments must not move any SE(3) table.  Needs the built library, no GPU:

    python tests/golden/make_sfc_plan_se3.py            # rewrite the file
    python tests/golden/make_sfc_plan_se3.py --check    # exit 1 if the file differs from what this checkout computes
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "sfc_plan_se3.json")

# (input irreps = DTP node output, spherical harmonics, consumer irreps, n2): CASES, test_l3_plans and
# test_planner_verdicts_drive_the_fallback of tests/test_sfcx_plan.py
SPECS = [
    ("128x0e+64x1e+32x2e", "1x0e+1x1e+1x2e", "224x0e+64x1e+32x2e", 128),
    ("128x0e+64x1e+32x2e", "1x0e+1x1e+1x2e", "128x0e+64x1e+32x2e", 0),
    ("256x0e+128x1e", "1x0e+1x1e", "256x0e+128x1e", 0),
    ("128x0e+64x1e+64x2e+32x3e", "1x0e+1x1e+1x2e+1x3e", "128x0e+64x1e+64x2e+32x3e", 0),
    ("256x0e+128x1e+64x2e", "1x0e+1x1e+1x2e", "256x0e+128x1e+64x2e", 0),
    ("384x0e+192x1e+192x2e+96x3e", "1x0e+1x1e+1x2e+1x3e", "384x0e+192x1e+192x2e+96x3e", 128),
]


def compute():
    from equiformer_amd import lib, ops
    from equiformer_amd.layout import DtpTable, RowLayout
    rows = []
    for irr, sh, out, n2 in SPECS:
        table, lay = DtpTable(irr, sh, irr), RowLayout(out)
        spec = ops.SfcSpec(table, lay, n2=n2)
        # the library itself, not the spec's cache: the verdicts must not depend on `supported`
        mask = [lib.load().eqf_sfcx_supported(table.c_ref, lay.c_ref, n2, m) for m in (0, 1, 2)]
        numel = [lib.load().eqf_sfcx_packed_numel(table.c_ref, lay.c_ref, n2, m) for m in (0, 1, 2)]
        rows.append(dict(irreps=irr, sh=sh, out=out, n2=n2, supported=bool(spec.supported), x_mask=mask, packed_numel=numel,
                         degs=[list(d) for d in spec.degs], w_offs=list(spec.w_offs), weight_numel=spec.weight_numel,
                         weight2_numel=spec.weight2_numel, bias_dim=spec.bias_dim,
                         l3=[int(table.c.l3[i]) for i in range(table.c.npaths)]))
    return rows


if __name__ == "__main__":
    text = json.dumps(compute(), indent=1) + "\n"
    if "--check" in sys.argv:
        sys.exit(0 if open(OUT).read() == text else 1)
    open(OUT, "w").write(text)
