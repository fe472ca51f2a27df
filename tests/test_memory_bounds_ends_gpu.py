"""Memory-contract tier of the operators at the ends of a model (include/bsmm_ends.h), the contract of tests/test_memory_bounds_gpu.py: every
tensor a kernel may touch sits between poisoned guards (tests/_guard.py), outputs and the workspace are poisoned; after each call no guard
byte has changed, every element of loss / g / dx / y / dw has been stored, and the values are those of tests/_ends_ref.py -- a result computed
from poisoned memory would be a NaN.  The calls go through the C ABI so that the test decides where each tensor lies: aligned placements and
placements 2 and 4 bytes off for the activations (the kernels pick 16-byte or element accesses from the pointers); fp32 tensors, the integer
tensors and the workspace move by one element.  The forward in place over the logits is included."""
import ctypes

import numpy as np
import pytest

import _ends_ref as ER
import _guard as GD
import _parity as P

pytestmark = pytest.mark.gpu
CODE = {"f32": 0, "f16": 1, "bf16": 2}
S, R, W, G, V, T = 1, 2, 3, 4, 256, 512
# (N, K, path when aligned, path when off): the shapes of tests/test_ends_gpu.py that reach each path
XENT_SHAPES = [(3, 10, S, S), (64, 256, S | V, S), (4, 1024, S | V, S), (16, 1031, R, R), (3, 4096, R | V, R), (3, 8192, R | V, W), (3, 8193, W, W),
               (2, 32768, W | V, G), (2, 16385, G, G), (2, 32776, G | V, G), (8197, 8, S | V | T, S | T)]
OFFS = [(d, off) for d in ("f32", "f16", "bf16") for off in (0, 2, 4) if not (d == "f32" and off == 2)]
XENT_CASES = [(s, d, off) for s in XENT_SHAPES for d, off in OFFS]
EMBED_SHAPES = [((7, 5, 40), "outside"), ((50, 96, 300), "skew"), ((50, 96, 300), "straddle"), ((300, 1043, 64), "tiled"), ((16, 2056, 33), "equal")]
EMBED_CASES = [(s, p, d, off) for s, p in EMBED_SHAPES for d, off in OFFS]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import _lib
    return torch, _lib, _lib.load()


def _fp32_close(got, want64, what):
    l2, mx = P.errors(P.to_host(got).reshape(np.shape(want64)), want64)
    assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (what, l2, mx)


@pytest.mark.parametrize("case", XENT_CASES, ids=["N%d-K%d-%s-off%d" % (c[0][:2] + c[1:]) for c in XENT_CASES])
def test_xent_stays_inside(env, case):
    torch, _lib, L = env
    (N, K, path0, path1), dtype, off = case
    td = getattr(torch, P.TORCH_DT[dtype])
    mis = off // (4 if dtype == "f32" else 2)
    mis32 = 1 if off else 0
    X, labels, DY = ER.xent_inputs(N, K, dtype, "uniform")
    wloss, wg, wp, wdist = ER.xent_ref(X, labels)
    scale = ER.stash_scale(dtype)
    arena = GD.GuardArena(torch, "cuda")
    x = arena.place(X, "x", mis, td)
    lab = arena.place(labels.astype(np.int32), "labels", mis32)
    dy = arena.place(DY, "dy", mis32)
    stream = _lib.raw_stream(x.device)

    def settled(outputs, what):
        arena.check()
        for t, name in outputs:
            GD.assert_stored(torch, t, "%s: %s" % (what, name))

    def values(loss, g, what):
        _fp32_close(loss, wloss, (case, what, "loss"))
        got = P.to_host(g)
        if dtype == "f32":
            ratio, at = ER.f32_g_ratio(got, wg, wp, wdist)
            assert ratio <= 1.0, (case, what, ratio, at)
        else:
            ER.check_16bit(got, wg * scale, dtype, (case, what, "g"))

    # the forward, out of place
    loss, g = arena.alloc(N, torch.float32, "loss", mis32), arena.alloc((N, K), td, "g", mis)
    a = _lib.BsmmXentArgs(x=x.data_ptr(), labels=lab.data_ptr(), loss=loss.data_ptr(), g=g.data_ptr(), N=N, K=K, dtype=CODE[dtype], stream=stream)
    assert L.bsmm_xent_path(ctypes.byref(a)) == (path1 if off else path0)
    _lib.check(L.bsmm_xent_fwd(ctypes.byref(a)), "bsmm_xent_fwd")
    settled([(loss, "loss"), (g, "g")], "forward")
    values(loss, g, "forward")
    assert np.array_equal(P.to_host(x), X) and np.array_equal(lab.cpu().numpy(), labels)
    # the forward in place over a copy of the logits
    xin, loss2 = arena.place(X, "x-in-place", mis, td), arena.alloc(N, torch.float32, "loss-in-place", mis32)
    a = _lib.BsmmXentArgs(x=xin.data_ptr(), labels=lab.data_ptr(), loss=loss2.data_ptr(), g=xin.data_ptr(), N=N, K=K, dtype=CODE[dtype], stream=stream)
    _lib.check(L.bsmm_xent_fwd(ctypes.byref(a)), "bsmm_xent_fwd")
    settled([(loss2, "loss"), (xin, "g")], "forward in place")
    assert torch.equal(loss2, loss) and torch.equal(xin, g)
    # the backward, out of place and over the stash
    dx = arena.alloc((N, K), td, "dx", mis)
    a = _lib.BsmmXentArgs(g=g.data_ptr(), dy=dy.data_ptr(), dx=dx.data_ptr(), N=N, K=K, dtype=CODE[dtype], stream=stream)
    _lib.check(L.bsmm_xent_bwd(ctypes.byref(a)), "bsmm_xent_bwd")
    settled([(dx, "dx")], "backward")
    stash = P.to_host(g)
    wdx = stash.astype(np.float64) / scale * DY.astype(np.float64)[:, None]
    if dtype == "f32":
        ER.check_f32_dx(P.to_host(dx), stash, DY, (case, "dx"))
    else:
        ER.check_16bit(P.to_host(dx), wdx, dtype, (case, "dx"))
    a = _lib.BsmmXentArgs(g=xin.data_ptr(), dy=dy.data_ptr(), dx=xin.data_ptr(), N=N, K=K, dtype=CODE[dtype], stream=stream)
    _lib.check(L.bsmm_xent_bwd(ctypes.byref(a)), "bsmm_xent_bwd")
    settled([(xin, "dx")], "backward in place")
    assert torch.equal(xin, dx) and np.array_equal(P.to_host(dy), DY)
    arena.release()


@pytest.mark.parametrize("case", EMBED_CASES, ids=["C%d-K%d-n%d-%s-%s-off%d" % (c[0] + c[1:]) for c in EMBED_CASES])
def test_embedding_stays_inside(env, case):
    torch, _lib, L = env
    (C, K, n0), pattern, dtype, off = case
    td = getattr(torch, P.TORCH_DT[dtype])
    mis = off // (4 if dtype == "f32" else 2)
    mis32 = 1 if off else 0
    IDX = ER.embed_indices(C, n0, pattern)
    n = IDX.size
    Wt, DY, _ = ER.embed_values(C, K, n, dtype)
    arena = GD.GuardArena(torch, "cuda")
    w, dy = arena.place(Wt, "w", mis, td), arena.place(DY, "dy", mis, td)
    idx = arena.place(IDX.astype(np.int32), "idx", mis32)
    order = arena.place(ER.stable_order(IDX), "order", mis32)
    stream = _lib.raw_stream(w.device)
    a = _lib.BsmmEmbedArgs(C=C, K=K, nIdx=n, dtype=CODE[dtype], workspace=None, workspace_bytes=0, stream=stream)
    assert L.bsmm_ends_workspace_bytes(ctypes.byref(a), _lib.ENDS_EMBED_FWD) == 0
    y = arena.alloc((n, K), td, "y", mis)
    _lib.check(L.bsmm_embed_fwd(w.data_ptr(), idx.data_ptr(), y.data_ptr(), ctypes.byref(a)), "bsmm_embed_fwd")
    arena.check()
    GD.assert_stored(torch, y, "forward: y")
    assert np.array_equal(P.to_host(y), ER.embed_fwd_ref(Wt, IDX))
    need = int(L.bsmm_ends_workspace_bytes(ctypes.byref(a), _lib.ENDS_EMBED_GRAD))
    assert need > 0 and need % 4 == 0
    ws = arena.alloc(need // 4, torch.float32, "workspace", mis32)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    dw = arena.alloc((C, K), torch.float32, "dw", mis32)
    _lib.check(L.bsmm_embed_grad(dy.data_ptr(), idx.data_ptr(), order.data_ptr(), dw.data_ptr(), ctypes.byref(a)), "bsmm_embed_grad")
    arena.check()
    GD.assert_stored(torch, dw, "backward: dw")
    want, named = ER.embed_grad_ref(DY, IDX, C)
    ER.check_dw(P.to_host(dw), want, named, (case, "dw"))
    assert np.array_equal(P.to_host(w), Wt) and np.array_equal(P.to_host(dy), DY) and np.array_equal(idx.cpu().numpy(), IDX.astype(np.int32))
    assert np.array_equal(order.cpu().numpy(), ER.stable_order(IDX))
    arena.release()
