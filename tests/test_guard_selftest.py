"""The guard arena of the memory-contract tier (tests/_guard.py) must be able to FAIL: four faulty fake operations are caught, a correct one
passes.  CPU tensors only; every write of a fake operation stays inside the arena's own buffer (it goes through a view of that buffer that
is one row / one element wider than the tensor), nothing here calls the library and nothing runs on a GPU."""
import types

import numpy as np
import pytest
import torch

import _guard as GD

ROWS, COLS = 5, 24
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def _wide(arena, t, before=0, after=0):
    """A flat view of the arena's own buffer around tensor ``t``: ``before`` elements of the front guard, the tensor, ``after`` elements of the
    back guard -- what a kernel with a ragged-edge bug would address."""
    e = [e for e in arena.entries if e.view.data_ptr() == t.data_ptr()][0]
    isz = t.element_size()
    return e.buf[e.t0 - before * isz:e.t1 + after * isz].view(t.dtype)


def _setup(dtype, misalign=0):
    arena = GD.GuardArena(torch, "cpu")
    x = arena.place(np.arange(ROWS * COLS, dtype=np.float32).reshape(ROWS, COLS) / 64.0, name="x", dtype=dtype, misalign=misalign)
    y = arena.alloc((ROWS, COLS), dtype, name="y", misalign=misalign)
    return arena, x, y


def _good(arena, x, y):
    y.copy_(x * 2)


def _store_past_end(arena, x, y):
    y.copy_(x * 2)
    _wide(arena, y, after=1)[-1] = 1.0


def _store_before_start(arena, x, y):
    y.copy_(x * 2)
    _wide(arena, y, before=1)[0] = 1.0


def _last_row_unstored(arena, x, y):
    y[:-1].copy_(x[:-1] * 2)


def _reads_past_input(arena, x, y):
    y.copy_(x * 2)
    xs = _wide(arena, x, after=1)                       # the input and the first guard element behind it
    y[-1, -1] = xs[-2:].float().sum().to(y.dtype)        # "sum of the last row's tail", one element too long


def _verdict(arena, y):
    guard_ok = stored_ok = True
    try:
        arena.check()
    except GD.GuardError:
        guard_ok = False
    try:
        GD.assert_stored(torch, y, "y")
    except GD.GuardError:
        stored_ok = False
    return guard_ok, stored_ok


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("misalign", [0, 1])
def test_correct_operation_passes(dtype, misalign):
    arena, x, y = _setup(dtype, misalign)
    assert GD.poisoned(torch, y) == y.numel()            # an untouched output is all NaN
    _good(arena, x, y)
    assert _verdict(arena, y) == (True, True)
    assert torch.equal(y, x * 2)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).replace("torch.", ""))
@pytest.mark.parametrize("op,guard_ok,stored_ok", [(_store_past_end, False, True), (_store_before_start, False, True),
                                                   (_last_row_unstored, True, False), (_reads_past_input, True, False)],
                         ids=["store_past_end", "store_before_start", "last_row_unstored", "reads_past_input"])
def test_faulty_operations_are_caught(dtype, op, guard_ok, stored_ok):
    arena, x, y = _setup(dtype)
    op(arena, x, y)
    assert _verdict(arena, y) == (guard_ok, stored_ok)


def test_report_names_buffer_side_offset_and_count():
    arena, x, y = _setup(torch.float32)
    _good(arena, x, y)
    _wide(arena, y, after=3)[-1] = 0.0                    # third element behind the end: bytes 8 .. 11
    _wide(arena, x, before=2)[0] = 0.0                    # second element before the start: bytes -8 .. -5
    rep = {(n, s): (f, c) for n, s, f, c in arena.report()}
    assert rep == {("y", "back"): (8, 4), ("x", "front"): (5, 4)}      # (front: the distance of the nearest changed byte from the start)
    with pytest.raises(GD.GuardError, match="y back guard: 4 byte"):
        arena.check()


def test_geometry_conditions():
    arena = GD.GuardArena(torch, "cpu")
    for shape, dtype, mis in (((3, 40), torch.bfloat16, 0), ((7, 2240), torch.float32, 0), ((1000,), torch.uint8, 0), ((4, 9), torch.float16, 1),
                              ((6, 3, 32, 32), torch.bfloat16, 3)):
        t = arena.alloc(shape, dtype, misalign=mis)
        e = arena.entries[-1]
        isz = t.element_size()
        assert t.is_contiguous() and tuple(t.shape) == shape
        assert (t.data_ptr() - mis * isz) % 256 == 0                                       # on the boundary (plus the asked offset)
        assert (t.data_ptr() % 16 == 0) == (mis * isz % 16 == 0)
        assert e.buf.data_ptr() + e.t1 == t.data_ptr() + t.numel() * isz                   # the back guard starts at the last byte + 1
        pitch = shape[-1] * isz if len(shape) > 1 else min(t.numel() * isz, 32 * 1024)
        for g in (e.t0, e.buf.numel() - e.t1):
            assert g >= max(128 * pitch, 64 * 1024)
        assert bool((e.buf[:e.t0] == 0xFF).all()) and bool((e.buf[e.t1:] == 0xFF).all()) and GD.poisoned(torch, t) == t.numel()
    i = arena.alloc((5,), torch.int32)
    assert bool((i == -1).all())


def test_routing_proxy_sends_a_modules_allocations_through_the_arena():
    mod = types.SimpleNamespace(torch=torch)

    def fake_op(n):                                         # what the package's host classes do: reach the allocator through the module's name
        a = mod.torch.empty((n, 8), dtype=mod.torch.float32, device="cpu")
        b = mod.torch.empty_like(a)
        c = mod.torch.zeros(n, dtype=mod.torch.float32, device="cpu")
        d = mod.torch.empty(n)                              # no device: not the arena's business
        return a, b, c, d

    arena = GD.GuardArena(torch, "cpu")
    with GD.routed(arena, mod):
        a, b, c, d = fake_op(4)
        assert isinstance(a, mod.torch.Tensor) and mod.torch.float32 is torch.float32
    assert mod.torch is torch                               # put back
    assert len(arena.entries) == 3 and all("fake_op" in n for n in arena.names())
    assert GD.poisoned(torch, a) == 32 and GD.poisoned(torch, b) == 32 and bool((c == 0).all())
    arena.check()
    a2, _, _, _ = fake_op(4)
    assert len(arena.entries) == 3                          # outside the block nothing is routed
