"""Controls of tests/poison.py on CPU tensors (no GPU, no HIP kernel): the intercepted module is a stand-in of this file's own
that does `import torch` and allocates the way equiformer_amd/ops.py does.  The negative controls write into band memory the
test owns, with plain torch indexing on the allocation the registry holds."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poison  # noqa: E402

STANDIN_SOURCE = '''
import torch


def make(kind, *shape, dtype=torch.float32):
    return getattr(torch, kind)(shape, dtype=dtype)      # line 6


def like(kind, x, **kw):
    return getattr(torch, kind + "_like")(x, **kw)


def fill_all_but_the_last_row(rows, cols):
    out = torch.empty((rows, cols), dtype=torch.float32)
    out[:rows - 1] = torch.arange(float((rows - 1) * cols)).reshape(rows - 1, cols)   # a kernel that skips its tail row
    return out


def accumulate(rows, cols):
    out = torch.zeros((rows, cols), dtype=torch.float32)
    out += 1.0
    return out


def pinned_or_plain():
    return torch.zeros(4, dtype=torch.float32), torch.ones(3)
'''


@pytest.fixture
def standin():
    m = types.ModuleType("poison_standin")
    m.__file__ = "poison_standin.py"
    exec(compile(STANDIN_SOURCE, m.__file__, "exec"), m.__dict__)
    return m


def _raw(reg, i=-1):
    """the whole allocation behind the i-th tensor as elements of its dtype, and the index of the tensor's first element"""
    a = reg.live[i]
    item = torch.empty((), dtype=a.dtype).element_size()
    return a.buf.view(a.dtype), a.band // item, a.nbytes // item


@pytest.mark.parametrize("kind", ["empty", "zeros"])
@pytest.mark.parametrize("side", ["before", "behind"])
def test_a_write_one_element_outside_is_reported_with_side_and_offset(standin, kind, side):
    with poison.poisoned([standin], cpu=True) as reg:
        t = standin.make(kind, 5, 7)
        raw, first, n = _raw(reg)
        assert raw[first:first + n].data_ptr() == t.data_ptr() and n == 35
        t.fill_(1.0)
        raw[first - 1 if side == "before" else first + n] = 3.0
        with pytest.raises(AssertionError) as e:
            reg.check()
    msg = str(e.value)
    assert "changed %s the tensor" % side in msg and "offset 0 %s it" % side in msg, msg
    assert "poison_standin.py:6" in msg and "shape [5, 7]" in msg and "1 elements" in msg, msg


def test_a_write_further_out_gives_its_offset(standin):
    with poison.poisoned([standin], cpu=True) as reg:
        standin.make("empty", 3, 8)
        raw, first, n = _raw(reg)
        raw[first + n + 8 + 2] = 0.0   # row 1 behind the tensor, column 2
        raw[first - 5] = 0.0
        with pytest.raises(AssertionError) as e:
            reg.check()
    msg = str(e.value)
    assert "offset 10 behind it" in msg and "offset 4 before it" in msg, msg


def test_an_add_into_the_band_of_a_zeros_tensor_is_reported(standin):
    with poison.poisoned([standin], cpu=True) as reg:
        t = standin.make("zeros", 4, 4)
        raw, first, n = _raw(reg)
        before = raw[first + n + 3].item()
        assert before == before and abs(before) < 2.0   # a finite sentinel, not a NaN: the add below changes it
        raw[first + n + 3] += 1.0                        # what an atomic add one row too far does
        assert torch.equal(t, torch.zeros(4, 4))
        with pytest.raises(AssertionError) as e:
            reg.check()
    assert "offset 3 behind it" in str(e.value) and "(zero)" in str(e.value), str(e.value)


def test_untouched_allocations_pass_and_check_releases_them(standin):
    with poison.poisoned([standin], cpu=True) as reg:
        for dtype in (torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool):
            for kind in ("empty", "zeros"):
                for shape in ((), (0,), (1,), (3, 5), (2, 3, 480), (0, 16)):
                    t = standin.make(kind, *shape, dtype=dtype)
                    assert t.shape == torch.Size(shape) and t.dtype == dtype and t.is_contiguous()
                    if t.numel():
                        t.fill_(1)
        assert reg.allocations == 8 * 2 * 6 and len(reg.live) == reg.allocations
        reg.check()
        assert reg.live == [] and reg.allocations == 96
        reg.check()   # nothing left: passes


def test_a_routine_that_skips_its_last_row_returns_nan_exactly_there(standin):
    with poison.poisoned([standin], cpu=True) as reg:
        out = standin.fill_all_but_the_last_row(6, 5)
        reg.check()
    assert torch.isfinite(out[:5]).all() and torch.isnan(out[5]).all()
    assert torch.equal(out[:5], torch.arange(25.0).reshape(5, 5))


def test_zeros_are_zeros_and_accumulate(standin):
    with poison.poisoned([standin], cpu=True) as reg:
        out = standin.accumulate(3, 9)
        reg.check()
    assert torch.equal(out, torch.ones(3, 9))


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64, torch.uint8, torch.bool])
def test_integer_empty_comes_back_zero_filled(standin, dtype):
    with poison.poisoned([standin], cpu=True) as reg:
        t = standin.make("empty", 7, 3, dtype=dtype)
        u = standin.like("empty", t)
        reg.check()
    assert t.dtype == dtype and not t.any() and not u.any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int32, torch.int64, torch.uint8])
def test_empty_like_of_every_dtype_the_package_allocates(standin, dtype):
    x = torch.ones(5, 12).to(dtype)
    with poison.poisoned([standin], cpu=True) as reg:
        e, z = standin.like("empty", x), standin.like("zeros", x)
        f = standin.like("empty", x, dtype=torch.float32)
        p = standin.like("empty", x.t())   # a dense permuted tensor: torch keeps its strides
        assert reg.allocations == 4
        reg.check()
    for t in (e, z):
        assert t.dtype == dtype and t.shape == x.shape and t.stride() == x.stride() and t.device == x.device
    assert f.dtype == torch.float32 and f.shape == x.shape
    assert p.shape == x.t().shape and p.stride() == torch.empty_like(x.t()).stride()
    assert not z.any()
    assert torch.isnan(e).all() if dtype.is_floating_point else not e.any()


def test_modules_are_restored_after_a_normal_exit_and_after_an_exception(standin):
    with poison.poisoned([standin], cpu=True):
        assert standin.torch is not torch and isinstance(standin.torch, poison._PoisonedTorch)
        assert standin.torch.float32 is torch.float32 and standin.torch.nn is torch.nn   # everything else is forwarded
    assert standin.torch is torch
    with pytest.raises(KeyError):
        with poison.poisoned([standin], cpu=True):
            assert standin.torch is not torch
            raise KeyError("inside")
    assert standin.torch is torch and poison._active == []


def test_default_modules_are_restored_and_cpu_allocations_pass_through(standin):
    import importlib
    mods = [importlib.import_module(m) for m in poison.DEFAULT_MODULES]
    with poison.poisoned() as reg:
        assert all(isinstance(m.torch, poison._PoisonedTorch) for m in mods)
        t = mods[0].torch.empty((4, 4), dtype=torch.float32)       # a CPU allocation: not intercepted
        assert reg.allocations == 0 and t.untyped_storage().nbytes() == 64
        assert mods[0]._arena.MAX_REQ == -1   # ops._zeros: every accumulator its own torch.zeros, not a slice of a slab
    assert all(m.torch is torch for m in mods) and mods[0]._arena.MAX_REQ == type(mods[0]._arena).MAX_REQ > 0
    assert "MAX_REQ" not in vars(mods[0]._arena)
    with poison.poisoned([standin]) as reg:
        z, o = standin.pinned_or_plain()
        assert reg.allocations == 0 and torch.equal(z, torch.zeros(4)) and torch.equal(o, torch.ones(3))


def test_views_outlive_the_registry(standin):
    with poison.poisoned([standin], cpu=True) as reg:
        t = standin.make("zeros", 4, 6)
        v = t[1:3]
        reg.check()
    del reg
    t += 2.0
    assert torch.equal(v, torch.full((2, 6), 2.0)) and t._base is None and t.is_leaf
    g = t.clone().requires_grad_(True)
    (g * v.sum()).sum().backward()
    assert torch.equal(g.grad, torch.full((4, 6), 24.0))


def test_guard_input_keeps_values_and_requires_grad(standin):
    x = torch.randn(5, 6, dtype=torch.float64).t()   # not contiguous
    idx = torch.arange(9, dtype=torch.int32)
    with poison.poisoned([standin], cpu=True) as reg:
        a = poison.guard_input(x.requires_grad_(True))
        b = poison.guard_input(x.detach().float())
        i = poison.guard_input(idx)
        assert reg.allocations == 3
        raw, first, n = _raw(reg, 0)
        assert torch.isnan(raw[:first]).all() and torch.isnan(raw[first + n:]).all() and n == 30
        assert raw.numel() - first - n == first == poison.band_bytes((6, 5), torch.float64) // 8
        reg.check()
        poison.guard_input(idx)
        _raw(reg)[0][0] = 77   # somebody wrote in front of an input
        with pytest.raises(AssertionError) as e:
            reg.check()
        assert "before the tensor" in str(e.value) and "test_poison_alloc.py" in str(e.value)
    assert a.requires_grad and a.is_leaf and not b.requires_grad and a.is_contiguous()
    assert torch.equal(a.detach(), x.detach()) and a.dtype == torch.float64 and b.dtype == torch.float32
    assert torch.equal(i, idx) and i.dtype == torch.int32
    (a * a).sum().backward()
    assert torch.equal(a.grad, 2 * x.detach())
    c = poison.guard_input(x)   # no registry open: still a guarded copy
    assert torch.equal(c.detach(), x.detach()) and c.requires_grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.int64, torch.uint8])
@pytest.mark.parametrize("shape", [(), (1,), (3,), (5, 7), (130, 480), (2, 3, 33)])
def test_the_data_pointer_keeps_the_alignment_of_the_base(standin, shape, dtype):
    with poison.poisoned([standin], cpu=True) as reg:
        t = standin.make("empty", *shape, dtype=dtype)
        a = reg.live[-1]
        item = t.element_size()
        assert (t.data_ptr() - a.buf.data_ptr()) % 512 == 0 and t.data_ptr() - a.buf.data_ptr() == a.band
        assert a.band == max(4096, -(-128 * max(shape[-1] if shape else 1, 1) * item // 512) * 512)
        assert a.buf.numel() == 2 * a.band + t.numel() * item
        reg.check()


def test_the_fixture_checks_and_prints_its_line(standin, capsys):
    class _Node:
        nodeid = "tests/x.py::test_y"
    gen = poison._fixture()(types.SimpleNamespace(node=_Node))
    reg = next(gen)
    assert poison._active == [reg]
    with pytest.raises(StopIteration):
        next(gen)
    assert capsys.readouterr().out.strip() == "POISON tests/x.py::test_y allocations=0 guarded_bytes=0" and poison._active == []
