"""CPU checks of tests/sfc_edge_cases.py, the module behind tests/test_gpu_sfc_edges.py: the derived dispatch counts lie on
the two sides of the limits they name (re-derived from eqf_sfcx_dev_plan and the constants parsed from the sources), the
float32 yardstick stays below every bound (so that a bound never passes only through its 4 x yardstick term), and the
comparison and the guard check FAIL on each of five planted errors."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sfc_edge_cases as sc  # noqa: E402

# the derived counts of THIS tree (a retune of a threshold or of a planner fails here, with both numbers shown)
FWD_4_2 = {"qm9_sep_act": 2720, "qm9_sep_value": 4096, "qm9_sep_value_gated": 4096, "oc20_l1": 3264, "wide_l2": 2336}
FWD_2_1 = {"qm9_sep_act": 5440, "qm9_sep_value": 8192, "qm9_sep_value_gated": 8192, "oc20_l1": 6528, "md17_l3": 2720,
           "md17_l3_act": 2048, "wide_l2": 4672}
FWD_NY = {"qm9_sep_act": 6, "qm9_sep_value": 4, "oc20_l1": 5, "md17_l3": 6, "md17_l3_act": 8}
PSPLIT = {"qm9_sep_act": 3488, "qm9_sep_value": 3488, "qm9_sep_value_gated": 3488, "oc20_l1": 2048}
DEFAULT = {"Y_MIN_EDGES": 1500, "Y_MIN_EDGES_GATED": 4000, "W_MIN_EDGES": 9000, "W_MIN_EDGES_PLAIN": 20000, "sfcw rounds": 22000}


@pytest.mark.parametrize("case", sorted(sc.CASES))
def test_derived_counts_lie_on_both_sides_of_their_limits(case):
    s, c = sc.setup(case), sc.constants()
    s.x_mask(0)  # 7, and 5 for wide_l2 (asserted there)
    edges = {label: (fam, es, codes) for label, fam, es, codes in sc.dispatch_edges(case)}
    slots = c["FWD_SLOTS_D3"] if s.deg3 else c["FWD_SLOTS"]
    for label, nsp, table in (("fwd 4->2", 4, FWD_4_2), ("fwd 2->1", 2, FWD_2_1)):
        if label not in edges:
            assert case not in table and s.deg3 and nsp == 4, (case, label)  # degree 3: the LDS condition rules the 4-way split out
            continue
        _, (lo, hi), codes = edges[label]
        a, b = sc.plan(case, 0, lo)[0], sc.plan(case, 0, hi)[0]
        assert nsp * a["nx"] * a["ny"] <= slots < nsp * b["nx"] * b["ny"], (case, label, lo, hi, a, b, slots)
        assert codes == (nsp, nsp // 2) and hi == lo + 1
        assert (lo, hi) == (table[case], table[case] + 1), "%s %s: derived %d | %d, this tree's table says %d | %d" % (
            case, label, lo, hi, table[case], table[case] + 1)
        if case in FWD_NY:
            assert a["ny"] == FWD_NY[case]
    if "bwd psplit" in edges:
        _, (lo, hi), codes = edges["bwd psplit"]
        a, b = sc.plan(case, 1, lo)[0], sc.plan(case, 1, hi)[0]
        assert 2 * a["nx"] * a["ny"] <= c["BWD_PSPLIT_SLOTS"] < 2 * b["nx"] * b["ny"], (case, lo, hi, a, b)
        assert codes == (2, 1) and a["lds"] <= 4 * c["XB_WAVE1_OFF"]
        assert (lo, hi) == (PSPLIT[case], PSPLIT[case] + 1), (case, lo, hi, PSPLIT[case])
    else:
        assert case not in PSPLIT and (s.deg3 or not s.x_mask(0) & 2), case  # degree 3 always runs two waves; wide_l2: exact fp32
    _, (lo, hi), chunks = edges["wgrad chunk"]
    nitem = sc.plan(case, 2, lo)[0]["ny"]
    assert lo == c["XW_MIN_CHUNK"] * -(-c["XW_WAVES"] // nitem) and hi == lo + 1
    assert chunks == (c["XW_MIN_CHUNK"], c["XW_MIN_CHUNK"] + 32), (case, lo, hi, chunks)
    if case == "qm9_sep_act":
        assert (lo, hi) == (3904, 3905), (lo, hi)
    # the multi-wave weight-gradient planner's own verdict (kind 3): degrees <= 2 in split and bf16; never in split6 (LDS)
    assert [sc.sfcw_accepts(case, m) for m in (0, 1, 2)] == [s.multi, s.multi, False], case
    assert sc.expected_codes(case, 129, 2, 2, mode=2)[2] == 1
    for label, fam, (lo, hi), codes in sc.default_edges(case):
        assert hi == DEFAULT[label] and lo == hi - 1, (case, label, lo, hi, DEFAULT[label])
        below, above = sc.expected_codes(case, lo), sc.expected_codes(case, hi)
        assert (below[fam], above[fam]) == codes
        if s.multi and label != "sfcw rounds":
            assert codes[0] != codes[1], (case, label, codes)  # the automatic choice changes kernels across the limit
    # the tile-edge counts run the small-graph paths on both sides where the case has them
    assert sc.expected_codes(case, 129, 1, 1) == ((2 if s.deg3 else 4), (0 if case == "wide_l2" else 3 if s.deg3 else 2), 1)
    assert sc.expected_codes(case, 129, 2, 2, True) == ((8 if s.multi else 2), (0 if case == "wide_l2" else 3 if s.deg3 else 1),
                                                        (2 if s.multi else 1))


@pytest.mark.parametrize("case", sorted(sc.CASES))
def test_yardstick_stays_inside_the_bounds(case):
    _, ref, yard = sc.ref_and_yard(case, 129)
    s = sc.setup(case)
    want = {"out1", "dx", "dM", "dweight", "dbias"} | ({"dw"} if s.use_w else set()) | ({"out2", "dweight2", "dbias2"} if s.n2 else set())
    assert {q for q in sc.QUANTITIES if ref[q] is not None} == want
    for q in want:
        y = sc.rel(yard[q], ref[q])
        print("YARD %s %s %.2e" % (case, q, y))
        for mode in sc.MODE_OF:
            assert y < sc.bound_of(mode, q, 0.0), (case, q, mode, y)  # below the plain bound: the 4 x yardstick term is not what passes
        assert sc.YARD_FACTOR * y < sc.FP32_FLOOR, (case, q, y)


def _as_kernel_output(t, fill, seed=0):
    """a float32 CPU result placed in a guarded buffer the way a correct kernel would leave it"""
    t2 = t.float().reshape(-1, 32) if t.dim() == 1 else t.float()
    g = sc.guarded(t2.shape[0], t2.shape[1], fill, seed=seed)
    if fill == "acc":
        g.mid += t2
    else:
        g.mid.copy_(t2)
    return g


def _passes(mode, q, got, ref, yard):
    ck = sc.Checker("teeth", mode)
    ck.cmp("x", q, got, ref, yard)
    return not ck.bad


@pytest.mark.parametrize("mode", sorted(sc.MODE_OF))
@pytest.mark.parametrize("case", ["qm9_sep_act", "md17_l3"])
def test_the_comparison_has_teeth(case, mode):
    E = 33
    inp, ref, yard = sc.ref_and_yard(case, E)
    # what passes: the float32 evaluation through guarded buffers, overwritten and accumulated outputs
    o1 = _as_kernel_output(yard["out1"], "nan")
    assert _passes(mode, "out1", sc.check_guarded(o1), ref["out1"], yard["out1"])
    dM = _as_kernel_output(yard["dM"], "acc", seed=1)
    assert _passes(mode, "dM", sc.check_guarded(dM), ref["dM"], yard["dM"])
    dW = _as_kernel_output(yard["dweight"], "acc", seed=2)
    assert _passes(mode, "dweight", sc.check_guarded(dW).reshape(-1), ref["dweight"], yard["dweight"])
    # the planted errors are errors of the REFERENCE FUNCTION: its float32 evaluation (the yardstick) carries them too
    # 1. a reference with the last row of out1 dropped to zero
    def drop(t):
        t = t.clone()
        t[E - 1] = 0
        return t

    assert not _passes(mode, "out1", sc.check_guarded(o1), drop(ref["out1"]), drop(yard["out1"]))

    # 2. rows E-1 and E-2 swapped
    def swap(t):
        t = t.clone()
        t[[E - 1, E - 2]] = t[[E - 2, E - 1]]
        return t

    assert not _passes(mode, "out1", sc.check_guarded(o1), swap(ref["out1"]), swap(yard["out1"]))
    assert not _passes(mode, "dx", yard["dx"], swap(ref["dx"]), swap(yard["dx"]))
    # 3. one path's w_off shifted by 32
    shifted = sc.evaluate(case, inp, torch.float64, spec=sc.shifted_spec(case, 0))
    shifted32 = sc.evaluate(case, inp, torch.float32, spec=sc.shifted_spec(case, 0))
    for q in ("out1", "dx", "dw", "dweight"):
        assert not _passes(mode, q, yard[q], shifted[q], shifted32[q]), q
    # 4. a guard row with one flipped bit, before and behind the tensor, in an overwritten and in an accumulated output
    for g, row in ((o1, sc.G - 1), (o1, sc.G + E), (dM, 0), (dM, 2 * sc.G + E - 1)):
        word = g.buf[row].view(torch.int32)
        word[3] ^= 1
        with pytest.raises(AssertionError, match="guard"):
            sc.check_guarded(g)
        word[3] ^= 1
        sc.check_guarded(g)
    # ... and a NaN left in the middle of an overwritten output
    o1.mid[E - 1, 5] = float("nan")
    with pytest.raises(AssertionError, match="not finite"):
        sc.check_guarded(o1)
    # 5. an accumulated output returned without its prefill (the kernel stored where it must add)
    stored = sc.guarded(E, ref["dM"].shape[1], "acc", seed=1)
    stored.mid.copy_(yard["dM"])
    assert not _passes(mode, "dM", sc.check_guarded(stored), ref["dM"], yard["dM"])
    stored = sc.guarded(ref["dbias"].numel() // 32, 32, "acc", seed=4)
    stored.mid.copy_(yard["dbias"].reshape(-1, 32))
    assert not _passes(mode, "dbias", sc.check_guarded(stored).reshape(-1), ref["dbias"], yard["dbias"])
