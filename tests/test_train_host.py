"""CPU-side checks of the training loops (equiformer_amd/train.py, csrc/trainloss.hip): the C-ABI entry points in header and
binding table with their argument errors, the schedules against the reference's functions (its checkout, or
tests/golden/trainloss/schedules.json recorded from it) and hand-computed values, and what is refused without a GPU."""
import ast
import ctypes
import functools
import json
import math
import os
import re
import sys
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fp64_trainloss as ft  # noqa: E402

NAMES = ("eqf_ef_loss_fwd", "eqf_ef_loss_bwd")


# --------------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_are_declared_bound_and_cite_the_reference():
    from equiformer_amd import build, lib, ops
    header = open(os.path.join(ROOT, "include", "equiformer_hip.h")).read()
    assert "trainloss.hip" in build.SOURCES
    cites = {"eqf_ef_loss_fwd": ("engine.py:71", "main_md17.py:384-386", "L2MAELoss :126-129", "energy_trainer_v2.py:413-459"),
             "eqf_ef_loss_bwd": ("engine.py:77", "main_md17.py:389")}
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    for name in NAMES:
        before = header[:header.index("int %s(" % name)]
        comment = before[before.rindex("/*"):]
        for cite in cites[name]:
            assert cite in comment, (name, cite)
        m = re.search(r"\bint\s+%s\s*\(([^;{]*?)\)\s*;" % name, text, flags=re.S)
        args = [a.strip() for a in m.group(1).split(",")]
        sig = lib.SIGNATURES[name]
        assert len(args) == len(sig)
        for a, t in zip(args, sig):
            want = ctypes.c_void_p if "*" in a else (ctypes.c_int if a.startswith("int ") else ctypes.c_double)
            assert t is want, (name, a, t)
        assert args[-1] == "void* stream"
    bwd = header[:header.index("int eqf_ef_loss_bwd(")]
    assert "RECOMPUTED here from row_mask" in bwd[bwd.rindex("/*"):]  # where the backward's count comes from is stated
    for c, v in ops.EF_CRITERIA.items():
        assert int(re.search(r"#define\s+EQF_LOSS_%s\s+(\d+)" % c.upper(), header).group(1)) == v


def test_argument_errors_are_return_codes(hip_lib):
    p = ctypes.c_void_p(8)
    f = hip_lib.eqf_ef_loss_fwd
    ok = [p, p, 4, p, p, None, 5, p, 2, 0.0, 1.0, 0.02, p, p, None]

    def fwd(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    assert fwd(a0=None) == -1 and fwd(a1=None) == -1 and fwd(a7=None) == -1 and fwd(a12=None) == -1  # missing pointers
    assert fwd(a2=0) == -1 and fwd(a2=-1) == -1 and fwd(a6=-1) == -1                                   # counts
    assert fwd(a8=3) == -1 and fwd(a8=-1) == -1                                                         # criterion
    assert fwd(a10=0.0) == -1 and fwd(a10=-1.0) == -1 and fwd(a10=float("nan")) == -1                  # task_std
    assert fwd(a4=None) == -1                                                                           # pred_dy without dy
    g = hip_lib.eqf_ef_loss_bwd
    okb = [p, p, p, 4, 5, p, p, None, 5, p, 0, 0.0, 1.0, p, p, None]

    def bwd(**kw):
        a = list(okb)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return g(*a)
    assert bwd(a0=None) == -1 and bwd(a13=None) == -1 and bwd(a9=None) == -1
    assert bwd(a4=3) == -1 and bwd(a3=0) == -1 and bwd(a8=-1) == -1 and bwd(a10=7) == -1 and bwd(a12=0.0) == -1
    assert bwd(a14=None) == -1 and bwd(a6=None) == -1                                                   # pred_dy without d_pred_dy / dy


def test_cpu_is_refused():
    from equiformer_amd import ops, train
    with pytest.raises(ops.HipOnlyError):
        train.EFLoss(0.0, 1.0, "l1", device="cpu")
    with pytest.raises(ops.HipOnlyError):
        ops.ef_loss(torch.zeros(3), torch.zeros(3), 3, torch.ones(2), 0.0, 1.0)
    with pytest.raises(ops.HipOnlyError):
        train.compute_stats([dict(pos=torch.zeros(4, 3), batch=torch.zeros(4, dtype=torch.long))], 5.0)
    with pytest.raises(ValueError):
        train.EFLoss(0.0, 1.0, "huber")


def test_a_reducer_is_refused():
    from equiformer_amd import train
    model = torch.nn.Linear(2, 1)
    opt = SimpleNamespace(_reducer=object(), param_groups=[dict(lr=1e-3)])
    for make in (lambda: train.qm9_train_step(model, opt, (0.0, 1.0), 5.0),
                 lambda: train.md17_train_step(model, opt, 5.0, 1.0, 80.0, task_mean=0.0, task_std=1.0),
                 lambda: train.oc20_train_step(model, opt, 5.0)):
        with pytest.raises(ValueError, match="data-parallel"):
            make()


def test_train_module_does_not_import_oracle():
    src = open(os.path.join(ROOT, "equiformer_amd", "train.py")).read()
    names = set()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Import):
            names |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add(node.module or "")
    assert not any(n == "oracle" or n.startswith("oracle.") for n in names), names
    assert "oracle" not in src


# ------------------------------------------------------------------------------------------------------------------ schedules
def _recorded():
    with open(ft.SCHEDULES) as f:
        return json.load(f)


def test_oc20_schedules_are_the_reference_functions():
    """warm-up edge (9, 10, 11), `total` (100), past it; the multistep milestones 20 / 40 / 60 and their neighbours"""
    from equiformer_amd import train
    c, m = ft.COSINE, ft.MULTISTEP
    cos = functools.partial(train.lr_lambda_cosine, warmup=c["warmup_epochs"], warmup_factor=c["warmup_factor"],
                            total=c["epochs"], lr_min_factor=c["lr_min_factor"])
    ms = functools.partial(train.lr_lambda_multistep, warmup=m["warmup_epochs"], warmup_factor=m["warmup_factor"],
                           decay_steps=m["decay_epochs"], decay_rate=m["decay_rate"])
    got = {"cosine": [cos(s) for s in ft.COSINE_STEPS], "multistep": [ms(s) for s in ft.MULTISTEP_STEPS]}
    rec = _recorded()
    if os.path.isfile(os.path.join(ft.REFERENCE, "oc20", "trainer", "lr_scheduler.py")):
        rc, rm = ft.reference_schedules()
        live = {"cosine": [rc(s, c) for s in ft.COSINE_STEPS], "multistep": [rm(s, m) for s in ft.MULTISTEP_STEPS]}
        assert live == rec  # the fixture is what the reference computes
    assert got == rec
    # by hand: the warm-up edge, the cosine's middle, the floor, the milestones
    assert cos(0) == 0.2 and cos(10) == 1.0 and cos(5) == pytest.approx(0.6, abs=1e-15)
    assert cos(50) == pytest.approx(0.01 + 0.99 * 0.5, abs=1e-15) and cos(100) == cos(150) == 0.01
    assert ms(19) == 1.0 and ms(20) == 0.3 and ms(40) == pytest.approx(0.09, abs=1e-15)
    assert ms(60) == pytest.approx(0.027, abs=1e-15) and ms(1000) == ms(60)


def test_cosine_epoch_lr_by_hand():
    """timm 0.4.12 CosineLRScheduler._get_lr, cycle_limit 1, computed by hand at the warm-up edge, mid-cycle and the end"""
    from equiformer_amd import train
    f = functools.partial(train.cosine_epoch_lr, lr=5e-4, epochs=300, warmup_epochs=5, warmup_lr=1e-6, min_lr=1e-6)
    assert f(0) == 1e-6
    assert f(1) == pytest.approx(1e-6 + (5e-4 - 1e-6) / 5, rel=1e-15)
    assert f(4) == pytest.approx(1e-6 + 4 * (5e-4 - 1e-6) / 5, rel=1e-15)
    assert f(5) == pytest.approx(1e-6 + 0.5 * (5e-4 - 1e-6) * (1 + math.cos(math.pi * 5 / 300)), rel=1e-15)
    assert f(150) == pytest.approx(1e-6 + 0.5 * (5e-4 - 1e-6), rel=1e-15)
    assert f(299) > f(300) == 1e-6 == f(301)
    g = functools.partial(train.cosine_epoch_lr, lr=1e-3, epochs=10)  # no warm-up: the cosine from epoch 0
    assert g(0) == 1e-3 and g(10) == 1e-5
