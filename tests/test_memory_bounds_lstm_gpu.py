"""Memory-contract tier of the fused LSTM gates (include/bsmm_lstm.h), the contract of tests/test_memory_bounds_gpu.py: every tensor a kernel
may touch sits between poisoned guards (tests/_guard.py) and the outputs are poisoned; after each call no guard byte has changed, every
element of c_next, h_next, dc and the four d-gates has been stored, and the values are those of tests/_lstm_ref.py -- a result computed from
poisoned memory would be a NaN.  The calls go through the C ABI so that the test decides where each tensor lies: aligned placements and
placements 2 and 4 bytes off (the kernels pick 16-byte or element accesses from the pointers; fp32 tensors move by one element)."""
import ctypes

import numpy as np
import pytest

import _guard as GD
import _lstm_ref as LR
import _parity as P
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu
CODE = {"f32": 0, "f16": 1, "bf16": 2}
FB = 1.0
NAMES = ("c_next", "h_next", "dc", "di", "du", "df", "do")
# K, N, axis: the 16-byte path and a long row on the element path (axis 0); the 16-byte path, slices of the fused tensor that are not 16-byte
# aligned although its rows are, and rows shorter than a 16-byte access (axis 1)
SHAPES = [(96, 40, 0), (3, 8193, 0), (40, 96, 1), (36, 1043, 1), (5, 8, 1)]
CASES = [(s, d, off) for s in SHAPES for d in ("f32", "f16", "bf16") for off in (0, 2, 4) if not (d == "f32" and off == 2)]
PADDED = [(d, off) for d in ("f32", "f16", "bf16") for off in (0, 2, 4) if not (d == "f32" and off == 2)]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from blocksparse_amd import _lib
    return torch, _lib, _lib.load()


def _close(got, want64, dtype, what):
    want = orc.round_to(np.asarray(want64), dtype) if dtype != "f32" else np.asarray(want64)
    got = P.to_host(got).reshape(want.shape)
    assert np.isfinite(got).all(), what
    l2, mx = P.errors(got, want)
    assert l2 <= P.L2_BAR[dtype] and mx <= P.MAX_BAR[dtype], (what, l2, mx)


def _call(_lib, L, K, N, axis, dtype, gate_ld, dgate_ld, stream, c, gates, bias, eh, ec, cn, hn, dc, dgates):
    """Both entry points on raw addresses; ``gates`` / ``dgates``: four addresses."""
    a = _lib.BsmmLstmArgs(K=K, N=N, axis=axis, dtype=CODE[dtype], gate_ld=gate_ld, dgate_ld=dgate_ld, forget_bias=FB, stream=stream)
    _lib.check(L.bsmm_lstm_gates(c, gates[0], gates[1], gates[2], gates[3], bias, cn, hn, ctypes.byref(a)), "bsmm_lstm_gates")
    _lib.check(L.bsmm_lstm_gates_grad(c, gates[0], gates[1], gates[2], gates[3], bias, eh, ec, dc, dgates[0], dgates[1], dgates[2], dgates[3],
                                      ctypes.byref(a)), "bsmm_lstm_gates_grad")


@pytest.mark.parametrize("case", CASES, ids=["K%d-N%d-a%d-%s-off%d" % (c[0] + c[1:]) for c in CASES])
def test_lstm_gates_stay_inside(env, case):
    torch, _lib, L = env
    (K, N, axis), dtype, off = case
    td = getattr(torch, P.TORCH_DT[dtype])
    esize = 4 if dtype == "f32" else 2
    mis = off // esize                                   # elements of the activations
    mis32 = 1 if off else 0                              # elements of the fp32 bias
    ax = 0 if axis == 0 else -1
    shape, hshape = ((K, N), (4 * K, N)) if axis == 0 else ((N, K), (N, 4 * K))
    C, H, EH, EC, B = LR.make_inputs(K, N, axis, dtype, K + N + off)
    parts = LR.split(H, ax)
    cn, hn = LR.forward(C, parts, B, FB, ax)
    dc, d, _ = LR.backward(C, parts, EH, EC, B, FB, ax)
    want = (cn, hn, dc) + d
    arena = GD.GuardArena(torch, "cuda")
    c, eh, ec = arena.place(C, "c", mis, td), arena.place(EH, "eh", mis, td), arena.place(EC, "ec", mis, td)
    b = arena.place(B, "bias", mis32)
    stream = _lib.raw_stream(c.device)
    step = (K * N if axis == 0 else K) * esize           # bytes between the gates of the fused tensor
    for form in ("fused", "four"):
        out = lambda name: arena.alloc(shape, td, "%s-%s" % (name, form), mis)
        ocn, ohn, odc = out("c_next"), out("h_next"), out("dc")
        if form == "fused":
            h = arena.place(H, "h", mis, td)
            dh = arena.alloc(hshape, td, "dh", mis)      # ONE guarded buffer: the kernel writes its four slices
            gp, dp, ld = [h.data_ptr() + q * step for q in range(4)], [dh.data_ptr() + q * step for q in range(4)], 4 * K
            dviews = torch.chunk(dh, 4, dim=ax)
            inputs = [(h, H)]
        else:
            gt = [arena.place(np.ascontiguousarray(p), "gate%d" % q, mis, td) for q, p in enumerate(parts)]
            dviews = [arena.alloc(shape, td, "dgate%d" % q, mis) for q in range(4)]
            gp, dp, ld = [t.data_ptr() for t in gt], [t.data_ptr() for t in dviews], K
            inputs = list(zip(gt, parts))
        _call(_lib, L, K, N, axis, dtype, ld, ld, stream, c.data_ptr(), gp, b.data_ptr(), eh.data_ptr(), ec.data_ptr(), ocn.data_ptr(), ohn.data_ptr(),
              odc.data_ptr(), dp)
        torch.cuda.synchronize()
        arena.check()
        for name, t, w in zip(NAMES, (ocn, ohn, odc) + tuple(dviews), want):
            GD.assert_stored(torch, t, "%s: %s" % (form, name))
            _close(t, w, dtype, (case, form, name))
        for t, src in inputs + [(c, C), (eh, EH), (ec, EC), (b, B)]:             # the inputs are as they were
            assert np.array_equal(P.to_host(t), src)
    # One gradient absent and no bias: NULL for ec, then for eh, on the fused tensor again.  The call with NULL must store the bits of the call
    # with an explicit tensor of zeros (the statement of include/bsmm_lstm.h).  Against float64 only the L2 bar is asked here: with one term
    # of dC missing the gradients are heavy-tailed (largest element ~19 x the mean magnitude at (3, 8193)), and the max bar of _parity.py
    # presumes one 16-bit step on the largest element stays below 6 % of the mean -- a single value that float64 puts within 3e-8 of a bf16
    # rounding boundary (below what fp32 resolves) then decides the figure, whichever way a correct kernel rounds it.
    h = arena.place(H, "h-again", mis, td)
    zeros = arena.place(np.zeros(shape, dtype=np.float32), "zeros", mis, td)
    gp = [h.data_ptr() + q * step for q in range(4)]
    a = _lib.BsmmLstmArgs(K=K, N=N, axis=axis, dtype=CODE[dtype], gate_ld=4 * K, dgate_ld=4 * K, forget_bias=FB, stream=stream)
    for grads in ("eh", "ec"):
        wdc, wd, _ = LR.backward(C, parts, EH if grads == "eh" else None, EC if grads == "ec" else None, None, FB, ax)
        outs = {}
        for absent in (None, zeros.data_ptr()):
            odc, dh = arena.alloc(shape, td, "dc-%s" % grads, mis), arena.alloc(hshape, td, "dh-%s" % grads, mis)
            _lib.check(L.bsmm_lstm_gates_grad(c.data_ptr(), gp[0], gp[1], gp[2], gp[3], None, eh.data_ptr() if grads == "eh" else absent,
                                              ec.data_ptr() if grads == "ec" else absent, odc.data_ptr(), dh.data_ptr(), dh.data_ptr() + step,
                                              dh.data_ptr() + 2 * step, dh.data_ptr() + 3 * step, ctypes.byref(a)), "bsmm_lstm_gates_grad")
            torch.cuda.synchronize()
            arena.check()
            outs[absent is None] = (odc, dh)
        iv = torch.int32 if dtype == "f32" else torch.int16
        for name, t, z in zip(("dc", "dh"), outs[True], outs[False]):
            GD.assert_stored(torch, t, "%s only: %s" % (grads, name))
            assert torch.equal(t.view(iv), z.view(iv)), (case, grads, name)
        for name, t, w in zip(NAMES[2:], (outs[True][0],) + tuple(torch.chunk(outs[True][1], 4, dim=ax)), (wdc,) + wd):
            want = orc.round_to(np.asarray(w), dtype) if dtype != "f32" else np.asarray(w)
            l2, mx = P.errors(P.to_host(t), want)
            assert l2 <= P.L2_BAR[dtype], (case, grads, name, l2, mx)
    arena.release()


@pytest.mark.parametrize("case", PADDED, ids=["%s-off%d" % c for c in PADDED])
def test_padded_gate_rows_are_neither_read_nor_written(env, case):
    """Four gate tensors of (N, K) inside rows of K + 8 elements (gate_ld = dgate_ld = K + 8), the 8 padding columns poisoned in the inputs
    and in the outputs: no padding reaches a result (it would be a NaN) and no padding column of a d-gate is stored."""
    torch, _lib, L = env
    dtype, off = case
    K, N, pad = 40, 96, 8
    td = getattr(torch, P.TORCH_DT[dtype])
    mis, mis32 = off // (4 if dtype == "f32" else 2), (1 if off else 0)
    C, H, EH, EC, B = LR.make_inputs(K, N, 1, dtype, 5 * K + N + off)
    parts = LR.split(H, -1)
    cn, hn = LR.forward(C, parts, B, FB, -1)
    dc, d, _ = LR.backward(C, parts, EH, EC, B, FB, -1)
    arena = GD.GuardArena(torch, "cuda")
    c, eh, ec = arena.place(C, "c", mis, td), arena.place(EH, "eh", mis, td), arena.place(EC, "ec", mis, td)
    b = arena.place(B, "bias", mis32)
    gt = []
    for q, p in enumerate(parts):
        t = arena.alloc((N, K + pad), td, "gate%d" % q, mis)                     # poisoned, then the live columns filled
        t[:, :K].copy_(P.to_dev(np.ascontiguousarray(p), dtype, torch))
        gt.append(t)
    dg = [arena.alloc((N, K + pad), td, "dgate%d" % q, mis) for q in range(4)]
    ocn, ohn, odc = (arena.alloc((N, K), td, n, mis) for n in ("c_next", "h_next", "dc"))
    _call(_lib, L, K, N, 1, dtype, K + pad, K + pad, _lib.raw_stream(c.device), c.data_ptr(), [t.data_ptr() for t in gt], b.data_ptr(), eh.data_ptr(),
          ec.data_ptr(), ocn.data_ptr(), ohn.data_ptr(), odc.data_ptr(), [t.data_ptr() for t in dg])
    torch.cuda.synchronize()
    arena.check()
    for name, t, w in zip(NAMES, (ocn, ohn, odc) + tuple(t[:, :K] for t in dg), (cn, hn, dc) + d):
        GD.assert_stored(torch, t, name)
        _close(t.contiguous(), w, dtype, (case, name))
    for t in gt + dg:                                                            # every padding byte still holds the fill
        assert bool((t[:, K:].contiguous().view(torch.uint8) == GD.FILL).all())
    for t, p in zip(gt, parts):
        assert np.array_equal(P.to_host(t[:, :K]), p)
    arena.release()
