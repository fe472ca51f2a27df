"""Guard arena for the memory-contract tests: every tensor a kernel may touch sits in a buffer of its own,

    [ front guard | tensor | back guard ]            (all of it 0xFF before the call)

so that a store outside the tensor changes a guard byte, an output element that is never stored stays NaN, and a read outside an
input that reaches a result poisons it.  All-ones bytes are a NaN in bf16, fp16 and fp32 and -1 in int32: one fill is the canary for
stores, the mark of elements never written and the poison of stray reads.

Geometry (conditions, not tuned numbers):
  * the tensor starts on a 256-byte boundary (plus ``misalign`` elements when asked for) and the back guard starts at its last byte + 1;
  * each guard is at least 128 rows of the tensor's row pitch (one row tile is the largest burst a ragged-edge bug misplaces) and never
    less than 64 KiB.  A one-dimensional tensor (a workspace) is taken in rows of up to 32 KiB.

``routed(arena, module, ...)`` sends the allocations a module makes through its module-level name ``torch`` (``torch.empty``,
``torch.empty_like``, ``torch.zeros`` for tensors on the arena's device) into the arena for the duration of a ``with`` block: the
module's attribute is replaced by a forwarding proxy and put back afterwards.  Nothing in the package knows about this."""
import contextlib
import sys

import numpy as np

FILL = 0xFF
ALIGN = 256
MIN_GUARD = 64 * 1024
GUARD_ROWS = 128
ROW_1D = 32 * 1024


class GuardError(AssertionError):
    pass


def _shape_of(size):
    if len(size) == 1 and not isinstance(size[0], (int, np.integer)):
        size = tuple(size[0])
    return tuple(int(s) for s in size)


class _Entry(object):
    __slots__ = ("name", "buf", "t0", "t1", "view", "kind")

    def __init__(self, name, buf, t0, t1, view, kind):
        self.name, self.buf, self.t0, self.t1, self.view, self.kind = name, buf, t0, t1, view, kind


class GuardArena(object):
    def __init__(self, torch, device="cuda"):
        self.torch = torch
        self.device = torch.device(device)
        self.entries = []

    # ---- geometry ------------------------------------------------------------------------------
    @staticmethod
    def guard_bytes(shape, itemsize):
        nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize if len(shape) else itemsize
        pitch = shape[-1] * itemsize if len(shape) >= 2 else min(max(nbytes, itemsize), ROW_1D)
        g = max(GUARD_ROWS * pitch, MIN_GUARD)
        return (g + ALIGN - 1) // ALIGN * ALIGN

    def _carve(self, shape, dtype, name, kind, misalign=0):
        torch = self.torch
        shape = tuple(int(s) for s in shape)
        itemsize = torch.empty((), dtype=dtype).element_size()
        nbytes = int(np.prod(shape, dtype=np.int64)) * itemsize
        guard = self.guard_bytes(shape, itemsize)
        off = int(misalign) * itemsize
        assert 0 <= off < ALIGN
        # (+ ALIGN: room to move the tensor's start onto the boundary whatever address the allocator hands back)
        buf = torch.full((guard + ALIGN + off + nbytes + guard,), FILL, dtype=torch.uint8, device=self.device)
        base = buf.data_ptr()
        t0 = (base + guard + ALIGN - 1) // ALIGN * ALIGN - base + off
        t1 = t0 + nbytes
        view = buf[t0:t1].view(dtype).view(shape)
        assert view.is_contiguous() and view.data_ptr() == base + t0 and (view.data_ptr() - off) % ALIGN == 0
        assert t0 >= guard and buf.numel() - t1 >= guard
        e = _Entry(name or "%s#%d" % (kind, len(self.entries)), buf, t0, t1, view, kind)
        self.entries.append(e)
        return e

    # ---- placing tensors -------------------------------------------------------------------------
    def place(self, src, name=None, misalign=0, dtype=None):
        """An input: a copy of ``src`` (NumPy array or tensor) between guards; returns the contiguous view."""
        torch = self.torch
        t = torch.from_numpy(np.ascontiguousarray(src)) if isinstance(src, np.ndarray) else src
        if dtype is not None:
            t = t.to(dtype)
        e = self._carve(tuple(t.shape), t.dtype, name, "input", misalign)
        e.view.copy_(t)
        return e.view

    def alloc(self, shape, dtype, name=None, misalign=0):
        """An output (or scratch): poisoned, every element NaN / -1 until a kernel stores it."""
        shape = (int(shape),) if isinstance(shape, (int, np.integer)) else tuple(int(s) for s in shape)
        return self._carve(shape, dtype, name, "output", misalign).view

    # ---- checks -----------------------------------------------------------------------------------
    def report(self):
        """[(name, side, first changed offset, changed bytes)] over all guards; the offset counts from the tensor's end for the back guard
        and back from the tensor's start (1 = the byte just before it) for the front guard."""
        torch = self.torch
        if not self.entries:
            return []
        guards = []
        for e in self.entries:
            guards.append((e, "front", e.buf[:e.t0]))
            guards.append((e, "back", e.buf[e.t1:]))
        flags = torch.stack([(g != FILL).any() for _, _, g in guards]).cpu().numpy()      # one round trip when everything is clean
        out = []
        for hit, (e, side, g) in zip(flags, guards):
            if not hit:
                continue
            idx = torch.nonzero(g != FILL).flatten()
            first = int(idx[0]) if side == "back" else int(g.numel() - int(idx[-1]))
            out.append((e.name, side, first, int(idx.numel())))
        return out

    def check(self):
        bad = self.report()
        if bad:
            raise GuardError("guard bytes changed: " + "; ".join(
                "%s %s guard: %d byte(s), first at %s%d" % (n, s, c, "end+" if s == "back" else "start-", f) for n, s, f, c in bad))

    def names(self):
        return [e.name for e in self.entries]

    def release(self):
        self.entries = []


def poisoned(torch, t):
    """How many elements of ``t`` still hold the fill pattern (NaN for the float types, -1 for integers)."""
    if t.is_floating_point():
        return int(torch.isnan(t).sum())
    return int((t == -1).sum())


def assert_stored(torch, t, what):
    n = poisoned(torch, t)
    if n:
        flat = (torch.isnan(t) if t.is_floating_point() else (t == -1)).flatten()
        first = int(torch.nonzero(flat).flatten()[0])
        raise GuardError("%s: %d of %d element(s) still hold the fill pattern (never stored, or computed from poisoned memory); first at flat index %d"
                         % (what, n, t.numel(), first))


class _TorchProxy(object):
    """Forwards everything to the real ``torch`` module except the allocation functions, which land in the arena when they ask for a tensor
    on the arena's device."""

    def __init__(self, real, arena):
        object.__setattr__(self, "_real", real)
        object.__setattr__(self, "_arena", arena)

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _mine(self, device):
        if device is None:
            return False
        return self._real.device(device).type == self._arena.device.type

    @staticmethod
    def _caller():
        f = sys._getframe(2)
        return "%s:%d" % (f.f_code.co_name, f.f_lineno)

    def empty(self, *size, **kw):
        if not self._mine(kw.get("device")):
            return self._real.empty(*size, **kw)
        shape, dtype = _shape_of(size), kw.get("dtype") or self._real.get_default_dtype()
        return self._arena.alloc(shape, dtype, name="%s %s%s" % (self._caller(), str(dtype).replace("torch.", ""), list(shape)))

    def empty_like(self, t, **kw):
        if not self._mine(kw.get("device", t.device)) or kw.get("dtype") is not None:
            return self._real.empty_like(t, **kw)
        return self._arena.alloc(tuple(t.shape), t.dtype, name="%s %s%s" % (self._caller(), str(t.dtype).replace("torch.", ""), list(t.shape)))

    def zeros(self, *size, **kw):
        if not self._mine(kw.get("device")):
            return self._real.zeros(*size, **kw)
        shape, dtype = _shape_of(size), kw.get("dtype") or self._real.get_default_dtype()
        return self._arena.alloc(shape, dtype, name="%s %s%s" % (self._caller(), str(dtype).replace("torch.", ""), list(shape))).zero_()


@contextlib.contextmanager
def routed(arena, *modules):
    """Route the ``torch.empty`` / ``empty_like`` / ``zeros`` calls of ``modules`` (which reach them through a module attribute ``torch``)
    into ``arena`` inside the block."""
    saved = [(m, m.torch) for m in modules]
    try:
        for m, real in saved:
            m.torch = _TorchProxy(real, arena)
        yield arena
    finally:
        for m, real in saved:
            m.torch = real
