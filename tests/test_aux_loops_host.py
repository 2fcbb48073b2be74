"""CPU-side checks of the DeNS and IS2RE + IS2RS training loops (equiformer_amd/train.py, csrc/meters.hip): the meter tables, the
eqf_meter_fold entry point in header and binding table with its argument errors, the denoising-weight decay and the 1-based
auxiliary-weight schedule the loops write, the refusals, and `RunningMeters.averages` on hand-made sums.  The loops run here on
stand-in steps whose `step` records what the loop wrote before it (nothing is launched)."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -------------------------------------------------------------------------------------------------------------- the tables
def test_meter_tables():
    from equiformer_amd import dens, is2rs, train
    G, ONE = train.GRAPHS, train.ONE
    assert train.DENS_METERS == (("loss_energy", 0, G), ("loss_force", 1, 3), ("loss_denoising_pos", 2, 4),
                                 ("mae_energy", 5, G), ("mae_force", 6, 3), ("mae_denoising_pos", 7, 4))
    # by name: main_md17_dens.py:411-427 weights the energy terms by the molecules, the force terms by the uncorrupted atoms and
    # the denoising terms by the corrupted atoms
    s = dens.STATS
    assert [s[v] for _, v, _ in train.DENS_METERS] == ["loss_e", "loss_f", "loss_d", "mae_e", "mae_f", "mae_d"]
    assert [w if w == G else s[w] for _, _, w in train.DENS_METERS] == [G, "n_f", "n_d", G, "n_f", "n_d"]
    assert train.IS2RS_METERS == (("loss", train.LOSS, ONE), ("energy_mae", 3, ONE), ("energy_mse", 4, ONE),
                                  ("energy_within_threshold", 5, ONE), ("pos_mae", 6, 2))
    s = is2rs.STATS
    assert [s[v] for _, v, _ in train.IS2RS_METERS[1:]] == ["energy_mae", "energy_mse", "energy_within_threshold", "pos_mae"]
    assert s[train.IS2RS_METERS[-1][2]] == "n_free"
    # what the launch receives: -1 for the loss scalar and for a constant weight
    m = train.RunningMeters(train.DENS_METERS, "cpu")
    assert list(m._value) == [0, 1, 2, 5, 6, 7] and list(m._weight) == [-1, 3, 4, -1, 3, 4]
    assert m.names == ("loss_energy", "loss_force", "loss_denoising_pos", "mae_energy", "mae_force", "mae_denoising_pos")
    assert m.acc.dtype == torch.float64 and m.acc.shape == (12,)
    m = train.RunningMeters(train.IS2RS_METERS, "cpu")
    assert list(m._value) == [-1, 3, 4, 5, 6] and list(m._weight) == [-1, -1, -1, -1, 2]
    with pytest.raises(ValueError):
        train.RunningMeters([("m%d" % i, 0, train.ONE) for i in range(17)], "cpu")
    with pytest.raises(ValueError):
        train.RunningMeters([], "cpu")
    with pytest.raises(ValueError):
        train.RunningMeters([("x", -1, train.ONE)], "cpu")
    with pytest.raises(ValueError):
        train.RunningMeters([("x", 0, 1.5)], "cpu")


def test_averages_of_hand_made_sums():
    from equiformer_amd import train
    m = train.RunningMeters(train.DENS_METERS, "cpu")
    sums = {"loss_energy": (3.0, 4.0), "loss_force": (0.0, 0.0), "loss_denoising_pos": (1.5, 3.0), "mae_energy": (2.0, 8.0),
            "mae_force": (0.0, 0.0), "mae_denoising_pos": (-0.25, 1.0)}
    a = m.averages(sums)
    assert set(a) == set(sums)
    assert a["loss_energy"] == (0.75, 3.0, 4.0) and a["loss_denoising_pos"].avg == 0.5 and a["mae_energy"].avg == 0.25
    assert a["mae_denoising_pos"].avg == -0.25
    for n in ("loss_force", "mae_force"):  # a zero count: NaN, not 0 and not an error
        assert math.isnan(a[n].avg) and a[n].sum == 0.0 and a[n].count == 0.0
    # without sums: the device buffer, read once
    m.acc.copy_(torch.tensor([6.0, 2.0] + [0.0] * 10, dtype=torch.float64))
    a = m.averages()
    assert m.reads == 1 and a["loss_energy"] == (3.0, 6.0, 2.0) and math.isnan(a["mae_force"].avg)
    m.reset()
    assert m.acc.abs().sum().item() == 0.0


def test_fold_refuses_the_cpu():
    from equiformer_amd import ops, train
    m = train.RunningMeters(train.IS2RS_METERS, "cpu")
    with pytest.raises(ops.HipOnlyError):
        m.fold(torch.zeros(8), torch.zeros(()))


# ------------------------------------------------------------------------------------------------------------- entry point
def test_entry_point_is_declared_bound_and_cites_the_reference():
    from equiformer_amd import build, lib
    header = open(os.path.join(ROOT, "include", "equiformer_hip.h")).read()
    assert "meters.hip" in build.SOURCES
    before = header[:header.index("int eqf_meter_fold(")]
    comment = before[before.rindex("/*"):]
    for cite in ("engine.py:23-27", "main_md17_dens.py:361-427", "energy_trainer_v2.py:247-317"):
        assert cite in comment, cite
    assert int(re.search(r"#define\s+EQF_METERS_MAX\s+(\d+)", header).group(1)) == 16
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    args = [a.strip() for a in re.search(r"\bint\s+eqf_meter_fold\s*\(([^;{]*?)\)\s*;", text, flags=re.S).group(1).split(",")]
    sig = lib.SIGNATURES["eqf_meter_fold"]
    assert len(args) == len(sig) == 9 and args[-1] == "void* stream"
    want = {"const int*": ctypes.POINTER(ctypes.c_int), "const double*": ctypes.POINTER(ctypes.c_double), "int": ctypes.c_int}
    for a, t in zip(args, sig):
        kind = a.rsplit(" ", 1)[0]
        assert t is want.get(kind, ctypes.c_void_p), (a, t)


def test_argument_errors_are_return_codes(hip_lib):
    """every refusal happens before a launch: the pointers here are not device memory, a launch would fault"""
    f = hip_lib.eqf_meter_fold
    p = ctypes.c_void_p(8)
    I3 = ctypes.c_int * 3
    D3 = ctypes.c_double * 3

    def fold(stats=p, n=8, loss=p, M=3, vi=(0, -1, 5), wi=(-1, 3, -1), wc=(4.0, 0.0, 1.0), acc=p):
        return f(stats, n, loss, M, None if vi is None else I3(*vi), None if wi is None else I3(*wi),
                 None if wc is None else D3(*wc), acc, None)
    assert fold(acc=None) == -1 and fold(vi=None) == -1 and fold(wi=None) == -1
    assert fold(M=0) == -1 and fold(M=17) == -1 and fold(M=-1) == -1 and fold(n=-1) == -1
    assert fold(vi=(0, -2, 5)) == -1 and fold(vi=(8, -1, 5)) == -1 and fold(wi=(-1, 8, -1)) == -1 and fold(wi=(-2, 3, -1)) == -1
    assert fold(n=5) == -1                        # stats[5] is past n_stats
    assert fold(stats=None) == -1                 # an index reads stats
    assert fold(loss=None) == -1                  # a value is the loss
    assert fold(wc=None) == -1                    # a weight is constant
    for bad in (2.5, -1.0, 2.0 ** 29, float("nan"), float("inf")):
        assert fold(wc=(bad, 0.0, 1.0)) == -1, bad
    # M beyond 16 with valid tables of 17 entries
    I17, D17 = ctypes.c_int * 17, ctypes.c_double * 17
    assert f(p, 8, p, 17, I17(*[0] * 17), I17(*[-1] * 17), D17(*[1.0] * 17), p, None) == -1


# ---------------------------------------------------------------------------------------------------------------- schedules
def test_denoising_weight_decay():
    from equiformer_amd import train
    f = train.dens_denoising_pos_weight
    assert f(5.0, 0, 10) == 5.0 and f(5.0, 5, 10) == 2.5 and f(5.0, 10, 10) == 0.0 and f(5.0, 15, 10) == 0.0
    assert f(5.0, 3, 10) == pytest.approx(3.5, abs=1e-15) and f(5.0, 7, 10, linear_decay=False) == 5.0


class _Stand:
    """what the loops touch of a step, recorded instead of launched"""

    def _init_stand(self, loss, total_steps=None):
        self.loss, self.total_steps = loss, total_steps
        self.model = torch.nn.Linear(1, 1)
        self.optimizer = SimpleNamespace(param_groups=[dict(lr=1e-3)])
        self.steps, self.seen = 0, []
        self.w0, self.lr_initial = 15.0, 1e-3

    def step(self, batch):
        self.seen.append((self.optimizer.param_groups[0]["lr"], float(self.loss._w_host[-1])))
        self.steps += 1


def _stand_loss(cls, n_weights, spec):
    from equiformer_amd import train
    loss = cls.__new__(cls)
    loss._w_host = torch.zeros(n_weights)
    loss.weights = torch.zeros(n_weights)
    loss.meters = train.RunningMeters(spec, "cpu")
    return loss


def _is2rs_stand(total_steps=None):
    from equiformer_amd import is2rs, train

    class S(_Stand, is2rs.IS2RSTrainStep):
        def __init__(self):
            self._init_stand(_stand_loss(train.IS2RSMeteredLoss, 2, train.IS2RS_METERS), total_steps)
    return S()


def _dens_stand():
    from equiformer_amd import dens, train

    class S(_Stand, dens.DeNSTrainStep):
        def __init__(self):
            self._init_stand(_stand_loss(train.DeNSMeteredLoss, 3, train.DENS_METERS))
    return S()


def test_is2rs_loop_writes_the_one_based_weight_and_the_lr():
    import functools
    from equiformer_amd import is2rs, train
    s = _is2rs_stand()
    lam = functools.partial(train.lr_lambda_cosine, warmup=2, warmup_factor=0.2, total=8, lr_min_factor=0.01)
    lines = []
    for epoch in range(2):
        train.train_one_epoch_is2rs(s, [None] * 4, lr_lambda=lam, total_steps=8, print_freq=3, log=lines.append)
    assert [lr for lr, _ in s.seen] == [1e-3 * lam(k) for k in range(8)]
    want = [is2rs.auxiliary_task_weight(15.0, k + 1, 8) for k in range(8)]
    assert [w for _, w in s.seen] == pytest.approx(want, abs=0, rel=1e-7)  # (the host word is fp32)
    assert want[0] == 15.0 - 14.0 / 8 and want[-1] == 1.0 and want[3] == 8.0
    # the 1-based step: a multiple of print_freq (3, 6), the epoch's first and last step (1, 4; 5, 8)
    assert [int(re.search(r"step: (\d+)", ln).group(1)) for ln in lines] == [1, 3, 4, 5, 6, 8]
    assert s.loss.meters.reads == len(lines) + 2
    assert lines[0].startswith("energy_mae: ") and "aux_weight: 1.32e+01" in lines[0]
    # no total_steps: the weight stays as it is
    s = _is2rs_stand()
    s.loss._w_host[1] = 7.0
    train.train_one_epoch_is2rs(s, [None] * 3)
    assert [w for _, w in s.seen] == [7.0] * 3 and s.loss.meters.reads == 1


def test_dens_loop_writes_the_decayed_weight_and_reads_per_log_line():
    from equiformer_amd import train
    s = _dens_stand()
    lines = []
    for epoch in range(3):
        out = train.train_one_epoch_dens(s, [None] * 5, epoch, 2, 10.0, linear_decay=True, print_freq=2, log=lines.append)
    assert [w for _, w in s.seen] == [10.0] * 5 + [5.0] * 5 + [0.0] * 5
    assert len(lines) == 9 and s.loss.meters.reads == 9 + 3  # steps 0, 2, 4 of each epoch, and the end of each
    assert lines[3].startswith("Epoch: [1][0/5] \tloss_e: nan, loss_f: nan, loss_denoising_pos: nan, e_MAE: nan")
    assert lines[3].endswith("denoising_pos_weight=5.00e+00")
    mae, loss = out
    assert set(mae) == set(loss) == {"energy", "force", "denoising_pos"} and math.isnan(loss["force"].avg)
    s = _dens_stand()
    train.train_one_epoch_dens(s, [None] * 2, 1, 2, 10.0)
    assert [w for _, w in s.seen] == [10.0, 10.0] and s.loss.meters.reads == 1


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from equiformer_amd import train
    model = torch.nn.Linear(2, 1)
    reducer = SimpleNamespace(_reducer=object(), param_groups=[dict(lr=1e-3)])
    plain = SimpleNamespace(_reducer=None, param_groups=[dict(lr=1e-3)])
    with pytest.raises(ValueError, match="data-parallel"):
        train.dens_train_step(model, reducer, 5.0, 0.05, 0.5, 1.0, 80.0, 5.0, task_mean=0.0, task_std=1.0)
    model.use_auxiliary_task = True
    with pytest.raises(ValueError, match="data-parallel"):
        train.is2rs_train_step(model, reducer, 5.0, 50, 0.0, 1.0, 0.0, 1.0, 15.0)
    model.use_auxiliary_task = False
    with pytest.raises(ValueError, match="no IS2RS head"):
        train.is2rs_train_step(model, plain, 5.0, 50, 0.0, 1.0, 0.0, 1.0, 15.0)
    with pytest.raises(ValueError, match="total_steps"):
        train.train_one_epoch_is2rs(_is2rs_stand(total_steps=100), [None])
    # a step of the wrong kind, and a step of the right class whose loss does not fold
    with pytest.raises(ValueError, match="is2rs_train_step"):
        train.train_one_epoch_is2rs(_dens_stand(), [None])
    with pytest.raises(ValueError, match="dens_train_step"):
        train.train_one_epoch_dens(_is2rs_stand(), [None], 0, 1, 1.0)
    ef = train.EFTrainStep.__new__(train.EFTrainStep)
    ef.kind, ef.loss = "oc20", None
    for loop in (lambda s: train.train_one_epoch_is2rs(s, [None]), lambda s: train.train_one_epoch_dens(s, [None], 0, 1, 1.0)):
        with pytest.raises(ValueError, match="_train_step"):
            loop(ef)
    s = _dens_stand()
    s.loss = object()
    with pytest.raises(ValueError, match="dens_train_step"):
        train.train_one_epoch_dens(s, [None], 0, 1, 1.0)
    assert s.seen == []
