"""Memory-contract tier of the layer norm (include/bsmm_norm.h), the contract of tests/test_memory_bounds_gpu.py: every tensor a kernel may
touch sits between poisoned guards (tests/_guard.py), outputs and the workspace are poisoned; after each call no guard byte has changed,
every element of y / mean / rstd (dx / dg / db) has been stored, and the values are those of tests/_layer_norm_ref.py -- a result computed
from poisoned memory would be a NaN.  The calls go through the C ABI so that the test decides where each tensor lies: aligned placements
and placements 2 and 4 bytes off (the kernels pick 16-byte or element accesses from the pointers; fp32 tensors and the workspace move
by one element), on shapes with ragged strips, a ragged last slice of K, segments, and rows that are no multiple of 16 bytes."""
import ctypes

import numpy as np
import pytest

import _guard as GD
import _layer_norm_ref as LR
import _parity as P
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu
CODE = {"f32": 0, "f16": 1, "bf16": 2}
SHAPES = [(96, 37, 0, 2), (1031, 24, 0, 1), (36, 1043, 1, 1)]        # K, N, axis, S
# bytes the activations are moved off their 256-byte boundary
# ReLU on the small shape only: there a seed exists whose smallest pre-activation is far from fp32 rounding of the mask (asserted below)
CASES = [(s, d, off, relu) for s in SHAPES for d in ("f32", "f16", "bf16") for off in (0, 2, 4) for relu in ((0, 1) if s[0] * s[1] < 4096 else (0,))
         if not (d == "f32" and off == 2)]


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


@pytest.mark.parametrize("case", CASES, ids=["K%d-N%d-a%d-S%d-%s-off%d-relu%d" % (c[0] + c[1:]) for c in CASES])
def test_layer_norm_stays_inside(env, case):
    torch, _lib, L = env
    (K, N, axis, S), dtype, off, relu = case
    td = getattr(torch, P.TORCH_DT[dtype])
    mis = off // (4 if dtype == "f32" else 2)            # elements of the activations
    mis32 = 1 if off else 0                              # elements of the fp32 tensors and of the workspace
    shape = (K, N) if axis == 0 else (N, K)
    for attempt in range(64):
        rng = np.random.RandomState(K + N + off + 7919 * attempt)
        X = orc.round_to(rng.normal(0.0, 1.0, shape).astype(np.float32), dtype)
        E = orc.round_to(rng.normal(0.0, 1.0, shape).astype(np.float32), dtype)
        G, B = rng.normal(0.0, 1.0, K).astype(np.float32), rng.normal(0.0, 1.0, K).astype(np.float32)
        if not relu or np.abs(LR.pre_activation(X, G, B, axis, S)).min() >= 1e-4:
            break
    assert not relu or np.abs(LR.pre_activation(X, G, B, axis, S)).min() >= 1e-4
    arena = GD.GuardArena(torch, "cuda")
    x, dy = arena.place(X, "x", mis, td), arena.place(E, "dy", mis, td)
    g, b = arena.place(G, "g", mis32), arena.place(B, "b", mis32)
    y, dx = arena.alloc(shape, td, "y", mis), arena.alloc(shape, td, "dx", mis)
    mean, rstd = arena.alloc((S, N), torch.float32, "mean", mis32), arena.alloc((S, N), torch.float32, "rstd", mis32)
    dg, db = arena.alloc(K, torch.float32, "dg", mis32), arena.alloc(K, torch.float32, "db", mis32)
    a = _lib.BsmmLnArgs(K=K, N=N, segments=S, axis=axis, dtype=CODE[dtype], relu=relu, epsilon=1e-6, workspace=None, workspace_bytes=0,
                        stream=_lib.raw_stream(x.device))
    for backward in (0, 1):
        need = int(L.bsmm_layer_norm_workspace_bytes(ctypes.byref(a), backward))
        assert need % 4 == 0
        ws = arena.alloc(max(need // 4, 1), torch.float32, "workspace-%d" % backward, mis32)
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        if backward == 0:
            _lib.check(L.bsmm_layer_norm(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ctypes.byref(a)),
                       "bsmm_layer_norm")
            arena.check()
            for t, name in ((y, "y"), (mean, "mean"), (rstd, "rstd")):
                GD.assert_stored(torch, t, name)
            assert GD.poisoned(torch, dx) == dx.numel() and GD.poisoned(torch, dg) == K and GD.poisoned(torch, db) == K
            _close(y, LR.forward(X, G, B, axis, S, 1e-6, bool(relu)), dtype, (case, "y"))
            m, r = LR.stats(X, axis, S, 1e-6)
            _close(mean, m, "f32", (case, "mean"))
            _close(rstd, r, "f32", (case, "rstd"))
        else:
            _lib.check(L.bsmm_layer_norm_grad(dy.data_ptr(), x.data_ptr(), g.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(), dx.data_ptr(),
                                              dg.data_ptr(), db.data_ptr(), ctypes.byref(a)), "bsmm_layer_norm_grad")
            arena.check()
            for t, name in ((dx, "dx"), (dg, "dg"), (db, "db")):
                GD.assert_stored(torch, t, name)
            wdx, wdg, wdb = LR.backward(E, X, G, B, axis, S, 1e-6, bool(relu))
            _close(dx, wdx, dtype, (case, "dx"))
            _close(dg, wdg, "f32", (case, "dg"))
            _close(db, wdb, "f32", (case, "db"))
    # the inputs are as they were
    assert np.array_equal(P.to_host(x), X) and np.array_equal(P.to_host(dy), E) and np.array_equal(P.to_host(g), G) and np.array_equal(P.to_host(b), B)
    arena.release()
