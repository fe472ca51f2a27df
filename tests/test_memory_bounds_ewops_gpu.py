"""Memory-contract tier of the layer epilogue (include/bsmm_ew.h), the contract of tests/test_memory_bounds_gpu.py: every tensor a kernel
may touch sits between poisoned guards (tests/_guard.py), outputs, masks and the workspace are poisoned; after each call no guard byte has
changed, every element of y / dx / db and every word of the mask has been stored, and the values are those of tests/_ewops_ref.py -- a
result computed from poisoned memory would be a NaN (a mask word read from poison would keep everything).  The calls go through the C ABI so
that the test decides where each tensor lies: aligned placements and placements 2 and 4 bytes off for the activations (the kernels pick
16-byte or element accesses from the pointers; fp32 tensors and the workspace move by one element, the mask stays 4-byte aligned)."""
import ctypes

import numpy as np
import pytest

import _ewops_ref as ER
import _guard as GD
import _parity as P
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu
CODE = {"f32": 0, "f16": 1, "bf16": 2}
SEED, OFFSET, KEEP = (1 << 40) + 12345, 9, 0.8
# K, N, axis: 16-byte path; ragged rows on the element path; a row cut over workgroups (partials in the workspace) on both paths; rows that are
# no multiple of 16 bytes; many rows of few features; a pad byte in the last mask word on the 16-byte path
SHAPES = [(96, 40, 0), (40, 1043, 0), (3, 8200, 0), (3, 8193, 0), (1043, 36, 1), (8, 3001, 1), (40, 96, 1), (5, 8, 1)]
CASES = [(s, d, off) for s in SHAPES for d in ("f32", "f16", "bf16") for off in (0, 2, 4) if not (d == "f32" and off == 2)]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from blocksparse_amd import _lib
    return torch, _lib, _lib.load()


def _close(got, want64, dtype, what):
    want = orc.round_to(np.asarray(want64), dtype) if dtype != "f32" else np.asarray(want64)
    l2, mx = P.errors(P.to_host(got).reshape(want.shape), want)
    assert l2 <= P.L2_BAR[dtype] and mx <= P.MAX_BAR[dtype], (what, l2, mx)


@pytest.mark.parametrize("case", CASES, ids=["K%d-N%d-a%d-%s-off%d" % (c[0] + c[1:]) for c in CASES])
def test_ewops_stay_inside(env, case):
    torch, _lib, L = env
    (K, N, axis), dtype, off = case
    td = getattr(torch, P.TORCH_DT[dtype])
    mis = off // (4 if dtype == "f32" else 2)            # elements of the activations
    mis32 = 1 if off else 0                              # elements of the fp32 tensors and of the workspace
    shape = (K, N) if axis == 0 else (N, K)
    total, words = K * N, (K * N + 31) // 32
    act = (K + N + off) % 3
    X, E, R, B = ER.make_inputs(K, N, axis, dtype, True, K + N + off)
    want_mask = ER.mask_words(total, SEED, OFFSET, KEEP)
    kept, scale = ER.unpack(want_mask, total), ER.scale_of(KEEP)
    arena = GD.GuardArena(torch, "cuda")
    x, dy, r = arena.place(X, "x", mis, td), arena.place(E, "dy", mis, td), arena.place(R, "residual", mis, td)
    b = arena.place(B, "b", mis32)
    state = arena.place(np.array([SEED, OFFSET], dtype=np.int64), "state")
    stream = _lib.raw_stream(x.device)

    def args(which, generate=0):
        a = _lib.BsmmEwArgs(K=K, N=N, axis=axis, dtype=CODE[dtype], act=act, generate=generate, threshold=ER.threshold_of(KEEP), scale=scale,
                            workspace=None, workspace_bytes=0, stream=stream)
        need = int(L.bsmm_ew_workspace_bytes(ctypes.byref(a), which))
        assert need % 4 == 0
        ws = arena.alloc(max(need // 4, 1), torch.float32, "workspace-%d" % which, mis32)
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        return a

    def settled(outputs, what):
        arena.check()
        for t, name in outputs:
            GD.assert_stored(torch, t, "%s: %s" % (what, name))

    out = lambda name: arena.alloc(shape, td, name, mis)
    # bias + activation, forward and backward (ReLU from the stored y)
    y = out("y")
    a = args(_lib.EW_BIAS_ACT)
    _lib.check(L.bsmm_bias_act(x.data_ptr(), b.data_ptr(), y.data_ptr(), ctypes.byref(a)), "bsmm_bias_act")
    settled([(y, "y")], "bias_act")
    _close(y, ER.forward(X, B, axis, act), dtype, (case, "y"))
    dx, db = out("dx"), arena.alloc(K, torch.float32, "db", mis32)
    a = args(_lib.EW_BIAS_ACT_GRAD)
    _lib.check(L.bsmm_bias_act_grad(dy.data_ptr(), (y if act == 1 else x).data_ptr(), b.data_ptr(), dx.data_ptr(), db.data_ptr(), ctypes.byref(a)),
               "bsmm_bias_act_grad")
    settled([(dx, "dx"), (db, "db")], "bias_act_grad")
    wdx, wdb = ER.backward(E, X, B, axis, act)
    _close(dx, wdx, dtype, (case, "dx"))
    _close(db, wdb, "f32", (case, "db"))
    if act == 0:                                         # the plain bias without dx: only db is written
        db0 = arena.alloc(K, torch.float32, "db-only", mis32)
        _lib.check(L.bsmm_bias_act_grad(dy.data_ptr(), None, b.data_ptr(), None, db0.data_ptr(), ctypes.byref(a)), "bsmm_bias_act_grad")
        settled([(db0, "db")], "bias_act_grad without dx")
        assert torch.equal(db0, db)
    # the mask alone, and its application
    mask = arena.alloc(words, torch.int32, "mask")
    _lib.check(L.bsmm_dropout_mask(mask.data_ptr(), state.data_ptr(), total, ER.threshold_of(KEEP), stream), "bsmm_dropout_mask")
    arena.check()
    assert np.array_equal(ER.as_u32(mask), want_mask)    # every word stored (a poisoned word is all ones), pad bits zero
    y2 = out("y-apply")
    _lib.check(L.bsmm_dropout_apply(x.data_ptr(), mask.data_ptr(), y2.data_ptr(), total, scale, CODE[dtype], stream), "bsmm_dropout_apply")
    settled([(y2, "y")], "dropout_apply")
    _close(y2, np.where(kept.reshape(shape), X.astype(np.float64) * scale, 0.0), dtype, (case, "apply"))
    # the fused forward: generating, then reading the mask it wrote; then the fused backward
    mask2, y3, y4 = arena.alloc(words, torch.int32, "mask-fused"), out("y-fused"), out("y-recompute")
    a = args(_lib.EW_BIAS_ACT_DROPOUT, generate=1)
    _lib.check(L.bsmm_bias_act_dropout(x.data_ptr(), b.data_ptr(), r.data_ptr(), state.data_ptr(), mask2.data_ptr(), y3.data_ptr(), ctypes.byref(a)),
               "bsmm_bias_act_dropout")
    settled([(y3, "y")], "fused forward")
    assert np.array_equal(ER.as_u32(mask2), want_mask)
    a.generate = 0
    _lib.check(L.bsmm_bias_act_dropout(x.data_ptr(), b.data_ptr(), r.data_ptr(), None, mask2.data_ptr(), y4.data_ptr(), ctypes.byref(a)),
               "bsmm_bias_act_dropout")
    settled([(y4, "y")], "fused recompute")
    assert torch.equal(y3, y4) and np.array_equal(ER.as_u32(mask2), want_mask)
    _close(y3, ER.forward(X, B, axis, act, kept, scale, R), dtype, (case, "y-fused"))
    dx2, db2 = out("dx-fused"), arena.alloc(K, torch.float32, "db-fused", mis32)
    a = args(_lib.EW_BIAS_ACT_DROPOUT_GRAD)
    _lib.check(L.bsmm_bias_act_dropout_grad(dy.data_ptr(), x.data_ptr(), b.data_ptr(), mask2.data_ptr(), dx2.data_ptr(), db2.data_ptr(), ctypes.byref(a)),
               "bsmm_bias_act_dropout_grad")
    settled([(dx2, "dx"), (db2, "db")], "fused backward")
    wdx, wdb = ER.backward(E, X, B, axis, act, kept, scale)
    _close(dx2, wdx, dtype, (case, "dx-fused"))
    _close(db2, wdb, "f32", (case, "db-fused"))
    # the inputs are as they were
    assert np.array_equal(P.to_host(x), X) and np.array_equal(P.to_host(dy), E) and np.array_equal(P.to_host(r), R) and np.array_equal(P.to_host(b), B)
    assert state.tolist() == [SEED, OFFSET]
    arena.release()
