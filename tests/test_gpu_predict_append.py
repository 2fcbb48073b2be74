"""eqf_predict_append (csrc/predict.hip) through evaluate.PredictionSink on the GPU, bit for bit against eager torch on the CPU in
fp32 -- the arithmetic of the reference's predict (energy_trainer_v2.py:170-204): `energy * std + mean`, and on the free atoms
`pos + (delta * positions_std + positions_mean)`, every operation rounded separately.  Every batch is padded with a phantom
structure whose rows (energy, pos, delta) are NaN and whose tags say "free": nothing of it may reach the sink.  Shapes: one
one-atom structure; (1, 7, 20) atoms; 2 x 50 atoms, whose 300 floats make the 256-lane loop wrap."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MEAN, STD = 0.3, 1.7
P_MEAN, P_STD = (0.01, -0.02, 0.03), (0.4, 0.5, 0.6)
NORM = dict(target_mean=MEAN, target_std=STD, positions_mean=P_MEAN, positions_std=P_STD)
SHAPES = {"one_atom": (1,), "ragged": (1, 7, 20), "wraps": (50, 50)}
PHANTOM = 5  # rows of the phantom structure
NAN = float("nan")


def _batch(sizes, tags, seed, energy_2d=False, tag_dtype=torch.int64):
    """a padded batch on the CPU: B real structures + the phantom one"""
    g = torch.Generator().manual_seed(seed)
    B, N = len(sizes), sum(sizes)
    energy = torch.cat([torch.randn(B, generator=g) * 3, torch.tensor([NAN])])
    sid = torch.cat([torch.randint(0, 2 ** 40, (B,), generator=g), torch.tensor([-999])])
    ends = torch.tensor(sizes).cumsum(0)
    mol_ptr = torch.cat([torch.zeros(1, dtype=torch.long), ends, ends[-1:] + PHANTOM]).to(torch.int32)
    pos = torch.cat([torch.randn(N, 3, generator=g) * 4, torch.full((PHANTOM, 3), NAN)])
    delta = torch.cat([torch.randn(N, 3, generator=g), torch.full((PHANTOM, 3), NAN)])
    t = {"none": torch.zeros(N, dtype=torch.int64), "all": torch.randint(1, 3, (N,), generator=g),
         "mixed": torch.randint(0, 3, (N,), generator=g)}[tags]
    if tags == "mixed" and N > 1:
        t[0], t[-1] = 0, 2
    t = torch.cat([t, torch.ones(PHANTOM, dtype=torch.int64)]).to(tag_dtype)  # the phantom rows would count as free
    return dict(energy=energy.view(-1, 1) if energy_2d else energy, sid=sid, mol_ptr=mol_ptr, pos=pos, delta=delta, tags=t, B=B, N=N)


def _reference(b):
    """eager torch, CPU, fp32: what the reference's predict computes for the real rows"""
    B, N = b["B"], b["N"]
    energy = b["energy"].reshape(-1)[:B] * torch.tensor(STD, dtype=torch.float32) + torch.tensor(MEAN, dtype=torch.float32)
    delta = b["delta"][:N] * torch.tensor(P_STD, dtype=torch.float32) + torch.tensor(P_MEAN, dtype=torch.float32)
    pred = b["pos"][:N].clone()
    mask = b["tags"][:N] > 0
    pred[mask] = pred[mask] + delta[mask]
    natoms = (b["mol_ptr"][1:B + 1] - b["mol_ptr"][:B]).to(torch.int32)
    return dict(energy=energy, sid=b["sid"][:B].clone(), natoms=natoms, pos=pred)


def _append(sink, b, with_pos=True, reserve=True):
    d = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in b.items()}
    if reserve:
        sink.reserve(b["B"], b["N"] if with_pos else 0)
    if with_pos:
        sink.append(d["energy"], d["sid"], d["mol_ptr"], b["B"], d["pos"], d["delta"], d["tags"], **NORM)
    else:
        sink.append(d["energy"], d["sid"], d["mol_ptr"], b["B"], target_mean=MEAN, target_std=STD)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _assert_equals(read, refs, with_pos=True):
    for name in ("energy", "sid", "natoms") + (("pos",) if with_pos else ()):
        want = torch.cat([r[name] for r in refs])
        got = read[name]
        assert got.dtype == want.dtype and got.shape == want.shape, (name, got.dtype, got.shape, want.shape)
        assert not torch.isnan(got).any() if got.is_floating_point() else True, name
        assert torch.equal(_bits(got), _bits(want)), (name, (got.double() - want.double()).abs().max().item())
    assert -999 not in read["sid"].tolist()


# ---------------------------------------------------------------------------------------- 1. bit-exact appends at moving cursors
@pytest.mark.parametrize("energy_2d", [False, True])
@pytest.mark.parametrize("tags", ["none", "all", "mixed"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_appends_are_eager_torch_bit_for_bit(shape, tags, energy_2d):
    """four appends into one sink (the last three at non-zero cursors), read back once"""
    from equiformer_amd.evaluate import PredictionSink
    sizes = SHAPES[shape]
    tag_dtype = torch.int32 if shape == "ragged" and energy_2d else torch.int64
    batches = [_batch(sizes, tags, seed=10 * k + len(sizes), energy_2d=energy_2d, tag_dtype=tag_dtype) for k in range(4)]
    refs = [_reference(b) for b in batches]
    sink = PredictionSink(DEV, graphs=64, atoms=512, write_pos=True)
    for b in batches:
        _append(sink, b)
    read = sink.read()
    _assert_equals(read, refs)
    assert (sink.graph_capacity, sink.atom_capacity) == (64, 512)  # (nothing grew: the cursors alone moved)
    # fixed atoms keep the bits of the input, free atoms moved
    pos_in = torch.cat([b["pos"][:b["N"]] for b in batches])
    fixed = torch.cat([b["tags"][:b["N"]] <= 0 for b in batches])
    assert torch.equal(_bits(read["pos"][fixed]), _bits(pos_in[fixed]))
    if tags != "none":
        assert (read["pos"][~fixed] != pos_in[~fixed]).any()
    # a sink is reusable: reset, one append, the same rows at cursor 0
    sink.reset()
    _append(sink, batches[2])
    _assert_equals(sink.read(), refs[2:3])


def test_without_positions_the_atom_part_is_left_alone():
    from equiformer_amd.evaluate import DESC, PredictionSink
    batches = [_batch(SHAPES["ragged"], "mixed", seed=k) for k in range(3)]
    sink = PredictionSink(DEV, graphs=16, atoms=64, write_pos=True)
    sink.pos.fill_(-7.0)
    _append(sink, batches[0])                    # 28 atoms
    _append(sink, batches[1], with_pos=False)    # energies and ids only: the atom cursor stays
    _append(sink, batches[2])
    d = dict(zip(DESC, sink.desc.cpu().tolist()))
    assert (d["graph_cursor"], d["atom_cursor"], d["dropped_graphs"], d["dropped_atoms"]) == (9, 56, 0, 0)
    read = sink.read()
    refs = [_reference(b) for b in batches]
    _assert_equals(read, refs, with_pos=False)
    assert torch.equal(_bits(read["pos"]), _bits(torch.cat([refs[0]["pos"], refs[2]["pos"]])))
    assert (sink.pos[56:] == -7.0).all()
    # a sink built without write_pos: no position buffer, positions refused
    plain = PredictionSink(DEV, graphs=4)
    assert plain.pos is None and plain.atom_capacity == 0
    _append(plain, batches[0], with_pos=False)
    r = plain.read()
    assert r["pos"] is None and torch.equal(_bits(r["energy"]), _bits(refs[0]["energy"]))
    with pytest.raises(ValueError, match="write_pos"):
        _append(plain, batches[0])


# ------------------------------------------------------------------------------------------------------ 2. a capacity one short
@pytest.mark.parametrize("short", ["graphs", "atoms"])
def test_a_batch_that_does_not_fit_is_dropped_whole(short):
    """The buffers are larger than the capacity the descriptor states, and filled with a sentinel: the rows past the stated
    capacity are guard words.  First batch fits; the second is one structure (or one atom) too many."""
    from equiformer_amd.evaluate import DESC, PredictionSink
    a, b = _batch((1, 7, 20), "mixed", seed=1), _batch((50, 50), "all", seed=2)
    gcap = a["B"] + b["B"] - (1 if short == "graphs" else 0)
    acap = a["N"] + b["N"] - (1 if short == "atoms" else 0)
    sink = PredictionSink(DEV, graphs=gcap + 8, atoms=acap + 8, write_pos=True)
    sink.energy.fill_(-7.0), sink.sid.fill_(-7), sink.natoms.fill_(-7), sink.pos.fill_(-7.0)
    sink.desc[2:4].copy_(torch.tensor([gcap, acap]))  # the stated capacities (the host still counts gcap + 8: it grows nothing)
    _append(sink, a)
    _append(sink, b)
    d = dict(zip(DESC, sink.desc.cpu().tolist()))
    assert (d["graph_cursor"], d["atom_cursor"]) == (a["B"], a["N"]), "the cursors moved for a dropped batch"
    assert (d["dropped_graphs"], d["dropped_atoms"]) == (b["B"], b["N"])
    # nothing of the dropped batch was written: neither inside the capacity nor in the guard words past it
    assert (sink.energy[a["B"]:] == -7.0).all() and (sink.sid[a["B"]:] == -7).all() and (sink.natoms[a["B"]:] == -7).all()
    assert (sink.pos[a["N"]:] == -7.0).all()
    ref = _reference(a)
    assert torch.equal(_bits(sink.energy[:a["B"]].cpu()), _bits(ref["energy"]))
    assert torch.equal(_bits(sink.pos[:a["N"]].cpu()), _bits(ref["pos"]))
    with pytest.raises(RuntimeError, match="capacity of %d structures and %d atoms" % (a["B"] + b["B"], a["N"] + b["N"])):
        sink.read()
    # a later batch that fits is still taken, behind the first
    c = _batch((1,), "all", seed=3)
    _append(sink, c)
    d = dict(zip(DESC, sink.desc.cpu().tolist()))
    assert (d["graph_cursor"], d["atom_cursor"]) == (a["B"] + 1, a["N"] + 1)
    assert torch.equal(_bits(sink.pos[a["N"]:a["N"] + 1].cpu()), _bits(_reference(c)["pos"]))


# ------------------------------------------------------------------------------------------------------ 3. captured and replayed
def test_one_captured_append_replayed_three_times_appends_three_times_across_growth():
    """One append recorded in a HIP graph from static inputs; the inputs are overwritten and the graph replayed three times.  The
    sink starts with room for exactly one batch, so the host grows it before the second and the third replay: the recorded
    launch finds the new buffers through the descriptor, and the prefix survives the moves."""
    from equiformer_amd.evaluate import PredictionSink
    sizes = (1, 7, 20)
    batches = [_batch(sizes, "mixed", seed=40 + k) for k in range(3)]
    refs = [_reference(b) for b in batches]
    B, N = batches[0]["B"], batches[0]["N"]
    warm = PredictionSink(DEV, graphs=B, atoms=N, write_pos=True)
    _append(warm, batches[0])  # (the kernel's code object is loaded before anything is captured)
    torch.cuda.synchronize()
    sink = PredictionSink(DEV, graphs=B, atoms=N, write_pos=True)
    static = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in batches[0].items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sink.append(static["energy"], static["sid"], static["mol_ptr"], B, static["pos"], static["delta"], static["tags"], **NORM)
    assert sink.desc[:2].cpu().tolist() == [0, 0], "capturing enqueued an append"
    addresses = []
    for b in batches:
        for k in ("energy", "sid", "pos", "delta", "tags"):
            static[k].copy_(b[k])
        sink.reserve(B, N)
        addresses.append((sink.energy.data_ptr(), sink.pos.data_ptr()))
        graph.replay()
    assert (sink.graph_capacity, sink.atom_capacity) == (4 * B, 4 * N), "the sink did not grow twice"
    assert addresses[0] != addresses[1] != addresses[2], "a growth kept the old buffers"
    _assert_equals(sink.read(), refs)
