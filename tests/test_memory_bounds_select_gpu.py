"""Memory-contract tier of the fused row selection (include/bsmm_select.h), the contract of tests/test_memory_bounds_gpu.py: every tensor a
kernel may touch sits between poisoned guards (tests/_guard.py) and the outputs are poisoned; after each call no guard byte has changed,
every output element has been stored, and the values are those of tests/_select_ref.py -- a result computed from poisoned memory would be
a NaN.  The calls go through the C ABI so that the test decides where each tensor lies: aligned placements and placements 2 and 4 bytes
off (the kernels pick 16-byte or element accesses from the pointers; fp32 tensors move by one element).  Row lengths on both sides of
every path threshold, and row counts that leave the last workgroup of the wave-per-row paths fewer rows than it has waves."""
import ctypes

import numpy as np
import pytest

import _guard as GD
import _parity as P
import _select_ref as SR
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu
CODE = {"f32": 0, "f16": 1, "bf16": 2}
# K, R, mask rows (a divisor of R): R = 5 and 6 leave a last workgroup of one resp. two rows where four waves wait
SHAPES = [(5, 5, 1), (512, 6, 3), (513, 5, 5), (1024, 5, 1), (1025, 2, 2), (2048, 3, 1), (2049, 2, 1), (4096, 2, 2)]
CASES = [(s, d, off) for s in SHAPES for d in ("f32", "f16", "bf16") for off in (0, 2, 4) if not (d == "f32" and off == 2)]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from blocksparse_amd import _lib, select
    return torch, _lib, _lib.load(), select


def _check(got, want64, dtype, what, l2_only=False):
    want = orc.round_to(np.asarray(want64), dtype) if dtype != "f32" else np.asarray(want64)
    got = P.to_host(got).reshape(want.shape)
    assert np.isfinite(got).all(), what
    l2, mx = P.errors(got, want)
    assert l2 <= P.L2_BAR[dtype] and (l2_only or mx <= P.MAX_BAR[dtype]), (what, l2, mx)


@pytest.mark.parametrize("case", CASES, ids=["K%d-R%d-m%d-%s-off%d" % (c[0] + c[1:]) for c in CASES])
def test_select_entry_points_stay_inside(env, case):
    torch, _lib, L, select = env
    (K, R, mrows), dtype, off = case
    td = getattr(torch, P.TORCH_DT[dtype])
    mis = off // (4 if dtype == "f32" else 2)            # elements of the activations
    mis32 = 1 if off else 0                              # elements of the fp32 mask
    rng = np.random.default_rng(K + R + off)
    k, scale, alpha = max(1, min(17, K - 1)), 0.5, 0.5
    X, DY = SR.round_in(rng.normal(0.0, 1.0, (R, K)), dtype), SR.round_in(rng.normal(0.0, 1.0, (R, K)), dtype)
    X[:, ::4] = X[:, :1]                                 # ties: the tie prefix runs too
    M = np.where(rng.random((mrows, K)) < 0.3, 0.0, rng.choice([1.0, 0.5, 2.0], (mrows, K))).astype(np.float32)
    M[:, 0] = 1.0
    Mfull = np.tile(M, (R // mrows, 1))
    assert select.select_path(K, td, off == 0) == SR.path_name(K, dtype, off == 0)
    arena = GD.GuardArena(torch, "cuda")
    x, dy, m = arena.place(X, "x", mis, td), arena.place(DY, "dy", mis, td), arena.place(M, "mask", mis32)
    stream = _lib.raw_stream(x.device)
    a = _lib.BsmmSelectArgs(R=R, K=K, k=k, mask_rows=mrows, dtype=CODE[dtype], rebase=1, scale=scale, alpha=alpha, stream=stream)
    out = lambda name: arena.alloc((R, K), td, name, mis)
    rect, topk, soft, dtopk, srelu, drelu = (out(n) for n in ("rect", "topk", "softmax", "dtopk", "sparse_relu", "drelu"))
    _lib.check(L.bsmm_rectified_top_k(x.data_ptr(), rect.data_ptr(), ctypes.byref(a)), "bsmm_rectified_top_k")
    _lib.check(L.bsmm_masked_top_k_softmax(x.data_ptr(), m.data_ptr(), topk.data_ptr(), ctypes.byref(a)), "bsmm_masked_top_k_softmax")
    _lib.check(L.bsmm_masked_softmax_grad(dy.data_ptr(), topk.data_ptr(), m.data_ptr(), dtopk.data_ptr(), ctypes.byref(a)), "bsmm_masked_softmax_grad")
    _lib.check(L.bsmm_sparse_relu(x.data_ptr(), srelu.data_ptr(), ctypes.byref(a)), "bsmm_sparse_relu")
    _lib.check(L.bsmm_select_relu_grad(dy.data_ptr(), srelu.data_ptr(), drelu.data_ptr(), ctypes.byref(a)), "bsmm_select_relu_grad")
    a.k = K                                              # the plain softmax, without a mask
    _lib.check(L.bsmm_masked_top_k_softmax(x.data_ptr(), None, soft.data_ptr(), ctypes.byref(a)), "bsmm_masked_top_k_softmax")
    torch.cuda.synchronize()
    arena.check()
    for name, t in (("rect", rect), ("topk", topk), ("softmax", soft), ("dtopk", dtopk), ("sparse_relu", srelu), ("drelu", drelu)):
        GD.assert_stored(torch, t, name)
    want_rect = orc.round_to(select.rectified_top_k_test(X, k, True), dtype) if dtype != "f32" else select.rectified_top_k_test(X, k, True)
    assert np.array_equal(P.to_host(rect), want_rect), (case, "rect")
    y64, S = SR.topk_softmax(X, k, Mfull, scale)
    _check(topk, y64, dtype, (case, "topk"), l2_only=True)           # (k of K values are non-zero: see close_l2 of test_select_gpu.py)
    assert np.array_equal(P.to_host(topk) != 0, (S & (Mfull != 0)) & (orc.round_to(y64, dtype) != 0 if dtype != "f32" else y64 != 0)), (case, "topk set")
    _check(soft, SR.topk_softmax(X, K, None, scale)[0], dtype, (case, "softmax"))
    _check(dtopk, SR.softmax_grad(DY, P.to_host(topk), Mfull, scale), dtype, (case, "dtopk"), l2_only=True)
    if K > 1:
        _check(srelu, SR.sparse_relu(X, alpha)[0], dtype, (case, "sparse_relu"))
    assert np.array_equal(P.to_host(drelu), np.where(P.to_host(srelu) > 0, DY, np.float32(0))), (case, "drelu")
    for t, src in ((x, X), (dy, DY), (m, M)):                        # the inputs are as they were
        assert np.array_equal(P.to_host(t), src)
    arena.release()
