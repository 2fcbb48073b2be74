"""CPU-side checks of the OC20 prediction pass (equiformer_amd/evaluate.py PredictionSink, oc20_predict_step, predict_oc20,
save_results; csrc/predict.hip): the C-ABI entry eqf_predict_append in header, binding table and build list, its argument errors
without a GPU, the sink's growth decisions from batch shapes, the split of the gathered positions by natoms, save_results against
a restatement of the reference's np.unique dedupe (base_trainer_oc20.py:742-754), and the three refusals of the public loop."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "eqf_predict_append"


# ------------------------------------------------------------------------------------------------------------------ the entry point
def test_entry_point_is_declared_bound_built_and_cites_the_reference():
    from equiformer_amd import build, evaluate, lib
    header = open(os.path.join(ROOT, "include", "equiformer_hip.h")).read()
    assert "predict.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "predict.hip"))
    before = header[:header.index("int %s(" % NAME)]
    comment = before[before.rindex("/*"):]
    assert "energy_trainer_v2.py:170-204" in comment
    assert "stream" in comment and "capture" in comment and "whole or not at all" in comment
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % NAME, text, flags=re.S)
    assert m, "%s is not declared in include/equiformer_hip.h" % NAME
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    sig = lib.SIGNATURES[NAME]
    assert len(args) == len(sig) == 18
    for a, t in zip(args, sig):
        if "*" in a:
            assert t is ctypes.c_void_p, (a, t)
        elif a.startswith("int "):
            assert t is ctypes.c_int, (a, t)
        else:
            assert a.startswith("float ") and t is ctypes.c_float, (a, t)
    names = [a.split()[-1].lstrip("*") for a in args]
    assert names[:8] == ["energy", "sid", "mol_ptr", "B", "pos", "delta", "tags", "tags_is64"]
    assert names[8:10] == ["target_mean", "target_std"] and names[-2:] == ["desc", "stream"]
    assert args[1] == "const long long* sid" and args[-2] == "long long* desc"  # int64 ids, int64 descriptor words
    # the descriptor layout the Python side mirrors
    words = int(re.search(r"#define\s+EQF_PREDICT_DESC_WORDS\s+(\d+)", header).group(1))
    assert words == len(evaluate.DESC) == 10
    for i, (word, macro) in enumerate(zip(evaluate.DESC, (
            "GRAPH_CURSOR", "ATOM_CURSOR", "GRAPH_CAP", "ATOM_CAP", "DROPPED_GRAPHS", "DROPPED_ATOMS", "ENERGY_OUT", "SID_OUT",
            "NATOMS_OUT", "POS_OUT"))):
        assert int(re.search(r"#define\s+EQF_PREDICT_%s\s+(\d+)" % macro, header).group(1)) == i, word
    # separately rounded fp32 operations: the file is compiled without contraction, as is2rs.hip is
    src = open(os.path.join(build.CSRC, "predict.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    # bound in evaluate.py, not in ops.py (tests/test_ops_trace.py pins the call list of ops.py)
    assert NAME in open(os.path.join(ROOT, "equiformer_amd", "evaluate.py")).read()
    assert NAME not in open(os.path.join(ROOT, "equiformer_amd", "ops.py")).read()


def test_argument_errors_are_return_codes(hip_lib):
    p = ctypes.c_void_p(8)
    f = hip_lib.eqf_predict_append
    norm = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0)
    assert f(None, p, p, 4, None, None, None, 0, *norm, p, None) == -1     # energy missing
    assert f(p, None, p, 4, None, None, None, 0, *norm, p, None) == -1     # sid missing
    assert f(p, p, None, 4, None, None, None, 0, *norm, p, None) == -1     # mol_ptr missing
    assert f(p, p, p, 4, None, None, None, 0, *norm, None, None) == -1     # descriptor missing
    assert f(p, p, p, -1, None, None, None, 0, *norm, p, None) == -1       # B < 0
    assert f(p, p, p, 4, None, p, None, 0, *norm, p, None) == -1           # delta without pos and tags
    assert f(p, p, p, 4, None, p, p, 1, *norm, p, None) == -1              # delta and tags without pos
    assert f(p, p, p, 4, p, p, None, 0, *norm, p, None) == -1              # pos and delta without tags
    assert f(p, p, p, 4, p, None, p, 0, *norm, p, None) == -1              # pos without delta
    assert f(None, p, p, 0, None, None, None, 0, *norm, p, None) == -1     # (errors come before the empty batch)
    assert f(p, p, p, 0, None, None, None, 0, *norm, p, None) == 0         # B == 0: no launch
    assert f(p, p, p, 0, p, p, p, 1, *norm, p, None) == 0


# ------------------------------------------------------------------------------------------------------------------ growth from shapes
def test_growth_decisions_from_batch_shapes():
    """A sink of 1 structure / 1 atom fed a sequence of batch sizes: it grows exactly when the host's running count would pass a
    capacity, to max(2 x capacity, needed), each capacity on its own; no tensor is looked at."""
    from equiformer_amd import evaluate, ops
    assert [evaluate.grown_capacity(c, n) for c, n in ((1, 0), (1, 1), (1, 2), (1, 5), (8, 9), (8, 17), (0, 3), (4096, 4096))] \
        == [1, 1, 2, 5, 16, 17, 3, 4096]
    with pytest.raises(ops.HipOnlyError):
        evaluate.PredictionSink("cpu")

    def sink(write_pos):
        s = evaluate.PredictionSink.__new__(evaluate.PredictionSink)  # (the bookkeeping alone: no device memory)
        s.write_pos, s.graph_capacity, s.atom_capacity, s.graphs, s.atoms = write_pos, 1, 1, 0, 0
        s.grown = []

        def grow(gcap, acap):
            s.grown.append((s.graphs, s.atoms, gcap, acap))  # (the prefix to copy is what was reserved BEFORE this batch)
            s.graph_capacity, s.atom_capacity = gcap, acap
        s._grow = grow
        return s
    batches = [(1, 1), (4, 100), (4, 90), (1, 5), (1, 300), (16, 4)]
    s = sink(True)
    caps = []
    for B, n in batches:
        s.reserve(B, n)
        caps.append((s.graph_capacity, s.atom_capacity))
    assert caps == [(1, 1), (5, 101), (10, 202), (10, 202), (20, 496), (40, 992)]
    assert s.grown == [(1, 1, 5, 101), (5, 101, 10, 202), (10, 196, 20, 496), (11, 496, 40, 992)]
    assert (s.graphs, s.atoms) == (27, 500)
    for (g, a), (gc, ac) in zip(((1, 1), (5, 101), (9, 191), (10, 196), (11, 496), (27, 500)), caps):
        assert g <= gc and a <= ac  # every batch fits when its launch runs
    # without write_pos no atom is counted and the atom capacity never moves
    s = sink(False)
    for B, n in batches:
        s.reserve(B, n)
    assert (s.graphs, s.atoms, s.atom_capacity) == (27, 0, 1) and [g[2] for g in s.grown] == [5, 10, 20, 40]


# ------------------------------------------------------------------------------------------------------------------ host functions
def test_positions_are_split_by_natoms_into_the_sid_dict():
    from equiformer_amd import evaluate
    pos = torch.arange(28 * 3, dtype=torch.float32).view(28, 3)
    out = evaluate.split_positions(pos, [1, 7, 20], [42, 7, 1234567890123])
    assert list(out) == ["42", "7", "1234567890123"]
    assert torch.equal(out["42"], pos[:1]) and torch.equal(out["7"], pos[1:8]) and torch.equal(out["1234567890123"], pos[8:])
    # an id met twice keeps its last rows (the reference's `pos_preds[sid] = ...`)
    twice = evaluate.split_positions(pos, [1, 7, 20], [5, 9, 5])
    assert list(twice) == ["5", "9"] and torch.equal(twice["5"], pos[8:])
    with pytest.raises(ValueError):
        evaluate.split_positions(pos, [1, 7, 19], [1, 2, 3])
    with pytest.raises(ValueError):
        evaluate.split_positions(pos, [8, 20], [1, 2, 3])
    read = dict(energy=torch.tensor([0.5, -1.25, 3.0]), sid=torch.tensor([42, 7, 1234567890123]),
                natoms=torch.tensor([1, 7, 20], dtype=torch.int32), pos=pos)
    p = evaluate.predictions_of(read, write_pos=True)
    assert p["id"] == ["42", "7", "1234567890123"] and p["energy"] == [0.5, -1.25, 3.0]
    assert all(isinstance(e, float) for e in p["energy"]) and torch.equal(p["pos"]["7"], pos[1:8])
    assert set(evaluate.predictions_of(read)) == {"id", "energy"}
    with pytest.raises(ValueError):
        evaluate.predictions_of(dict(read, pos=None), write_pos=True)


def test_save_results_is_the_reference_dedupe(tmp_path):
    """base_trainer_oc20.save_results for one process, keys=["energy"]: the rank file's lists gathered, `np.unique(ids,
    return_index=True)` and the energies reordered by its index."""
    from equiformer_amd import evaluate
    ids = ["10", "9", "100", "9", "2", "10", "33"]  # duplicates (a distributed sampler repeats ids), string order != numeric
    energy = [0.5, -1.0, 2.25, 7.0, 3.5, 8.0, -4.75]
    path = str(tmp_path / "is2re_predictions.npz")
    evaluate.save_results({"id": list(ids), "energy": list(energy)}, path)
    got = np.load(path, allow_pickle=True)
    # the reference, restated
    gathered = {"ids": [], "energy": []}
    gathered["ids"].extend(np.array(ids))
    gathered["energy"].extend(np.array(energy))
    _, idx = np.unique(gathered["ids"], return_index=True)
    want_ids, want_energy = np.array(gathered["ids"])[idx], np.array(gathered["energy"])[idx]
    assert sorted(got.files) == ["energy", "ids"]
    assert got["ids"].tolist() == want_ids.tolist() == ["10", "100", "2", "33", "9"]
    assert got["energy"].dtype == want_energy.dtype == np.float64
    assert got["energy"].tolist() == want_energy.tolist() == [0.5, 2.25, 3.5, -4.75, -1.0]  # the first occurrence is kept


# ------------------------------------------------------------------------------------------------------------------ refusals
class _Stub(torch.nn.Module):
    def __init__(self, aux):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.use_auxiliary_task = aux


def test_the_three_refusals():
    from equiformer_amd import evaluate, nets
    p = inspect.signature(evaluate.oc20_predict_step).parameters
    assert list(p)[:7] == ["model", "radius", "target_mean", "target_std", "positions_mean", "positions_std", "write_pos"]
    assert (p["target_mean"].default, p["target_std"].default, p["write_pos"].default) == (0, 1, False)
    assert p["positions_mean"].default is None and p["positions_std"].default is None
    assert list(inspect.signature(evaluate.predict_oc20).parameters)[:5] == ["model", "loader", "radius", "step", "write_pos"]
    # 1. write_pos on a model without the IS2RS head -- the attribute is the real model's
    plain = nets.model_entrypoint("oc20_l1_256_nonlinear")(num_layers=1)
    assert plain.use_auxiliary_task is False and nets.model_entrypoint("oc20_l1_256_nonlinear_aux")(num_layers=1).use_auxiliary_task
    with pytest.raises(ValueError, match="IS2RS head"):
        evaluate.oc20_predict_step(plain.eval(), 5.0, write_pos=True, sink=object())
    with pytest.raises(ValueError, match="IS2RS head"):
        evaluate.predict_oc20(plain, [], 5.0, write_pos=True, sink=object())
    # 2. a batch without sid: named, before the sink or the batch is touched (the sink here is not one)
    m = _Stub(True).eval()
    step = evaluate.oc20_predict_step(m, 5.0, write_pos=True, sink=object())
    assert isinstance(step, evaluate.BucketedEvalStep) and step.graph_targets == ("sid",) and step.node_targets == ("tags",)
    assert step.meter is None and step.write_pos
    with pytest.raises(ValueError, match="sid"):
        step.step({"pos": torch.zeros(2, 3), "cell": torch.eye(3)[None]})
    with pytest.raises(ValueError, match="sid"):
        step.step({"pos": torch.zeros(2, 3), "cell": torch.eye(3)[None], "sid": None})
    # 3. a model in training mode (inherited from BucketedEvalStep)
    m.train()
    with pytest.raises(ValueError, match="training mode"):
        step.step({"pos": torch.zeros(2, 3), "cell": torch.eye(3)[None], "sid": torch.zeros(1, dtype=torch.int64)})
    assert step.eager_steps == step.replays == 0
    # a step built without write_pos cannot serve a pass that asks for positions
    with pytest.raises(ValueError, match="write_pos"):
        evaluate.predict_oc20(m, [], 5.0, step=evaluate.oc20_predict_step(m, 5.0, sink=object()), write_pos=True)
