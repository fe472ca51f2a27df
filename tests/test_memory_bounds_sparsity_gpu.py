"""Memory-contract tier of the dynamic-sparsity kernels (include/bsmm_sparsity.h), the contract of tests/test_memory_bounds_gpu.py: every
tensor a kernel may touch sits between poisoned guards (tests/_guard.py); after the call no guard byte has changed, every output element
has been stored and none was computed from poisoned memory, and the values are those of tests/_sparsity_ref.py.  The calls go through the
C ABI so that the test decides where each tensor lies: aligned and misaligned placements (the kernels pick 16-byte or element accesses
from the pointers), N = 200 on feature axis 1 with three pairs (a contraction that is no multiple of 16), an odd N (no multiple of 8: the
element path of both stages), and CB = 33 / KB = 65 (edge tiles of the second stage)."""
import ctypes

import numpy as np
import pytest

import _guard as GD
import _parity as P
import _sparsity_ref as SR
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu
CODE = {"f32": 0, "f16": 1, "bf16": 2}


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from blocksparse_amd import _lib
    return torch, _lib, _lib.load()


def _td(torch, dtype):
    return getattr(torch, P.TORCH_DT[dtype])


@pytest.mark.parametrize("misalign", (0, 1))
@pytest.mark.parametrize("dtype", ("f32", "f16", "bf16"))
@pytest.mark.parametrize("bs", (8, 32, 64))
def test_weight_kernels_stay_inside(env, bs, dtype, misalign):
    torch, _lib, L = env
    blocks = 37
    rng = np.random.RandomState(bs + misalign)
    W = orc.round_to(rng.normal(0.0, 0.01, (blocks, bs, bs)).astype(np.float32), dtype)
    W[4] = 0.0
    gate_np = (rng.rand(blocks) < 0.6).astype(np.float32)
    gate_np[4], gate_np[0] = 1.0, 0.0
    arena = GD.GuardArena(torch, "cuda")
    w = arena.place(W, "w", misalign, _td(torch, dtype))
    gate = arena.place(gate_np, "gate", misalign)
    st = _lib.raw_stream(w.device)
    for nt, norm in ((0, "max"), (1, "l2")):
        out = arena.alloc(blocks, torch.float32, "norm-" + norm, misalign)
        _lib.check(L.bsmm_block_norm(w.data_ptr(), out.data_ptr(), blocks, bs, CODE[dtype], nt, st), "bsmm_block_norm")
        GD.assert_stored(torch, out, "norm " + norm)
        ref = SR.block_norm(W, norm)
        if nt == 0:
            assert np.array_equal(P.to_host(out), ref.astype(np.float32))
        else:
            assert P.errors(P.to_host(out), ref)[0] <= P.L2_BAR["f32"]
        g2 = arena.alloc(blocks, torch.float32, "threshold-gate-" + norm, misalign)
        thr = float(np.float32(np.median(ref) * 1.0001))
        _lib.check(L.bsmm_block_threshold_prune(w.data_ptr(), g2.data_ptr(), thr, nt, blocks, bs, CODE[dtype], st), "bsmm_block_threshold_prune")
        GD.assert_stored(torch, g2, "threshold gate " + norm)
        got = P.to_host(g2)
        sure = np.abs(ref - thr) > 1e-5 * thr                       # (norms within fp32 rounding of the threshold may fall either way)
        assert set(np.unique(got)) <= {0.0, 1.0} and np.array_equal(got[sure], SR.threshold_gate(ref, thr)[sure])
    # sparsity prune: every gate is written exactly once
    idx_np = rng.permutation(blocks).astype(np.int32)
    idx = arena.place(idx_np, "idx", misalign)
    g3 = arena.alloc(blocks, torch.float32, "prune-gate", misalign)
    _lib.check(L.bsmm_block_prune(g3.data_ptr(), idx.data_ptr(), blocks, 11, st), "bsmm_block_prune")
    GD.assert_stored(torch, g3, "prune gate")
    want = np.zeros(blocks, dtype=np.float32)
    want[idx_np[:11]] = 1.0
    assert np.array_equal(P.to_host(g3), want)
    # decay in place, last: it rewrites w
    _lib.check(L.bsmm_block_l2_decay(w.data_ptr(), gate.data_ptr(), 0.05, 1e-12, blocks, bs, CODE[dtype], st), "bsmm_block_l2_decay")
    arena.check()
    GD.assert_stored(torch, w, "decayed w")
    P.assert_blocks(P.to_host(w), SR.l2_decay(W, gate_np, 0.05, 1e-12), dtype, blocks, ctx=("decay", bs, dtype, misalign))
    assert np.array_equal(P.to_host(w)[gate_np == 0], W[gate_np == 0])
    arena.release()


# axis, bsize, N, CB, KB, pairs, dtype, misalign (elements) of the activations / of the reduced arrays and dw
REDUCE_CASES = [
    (1, 32, 200, 3, 5, 3, "bf16", 0, 0),          # the contraction 600 is no multiple of 16
    (1, 32, 200, 3, 5, 3, "bf16", 1, 1),
    (1, 8, 203, 3, 5, 2, "f16", 0, 0),            # odd N: rows of the reduced arrays are not 16-byte aligned
    (1, 8, 200, 33, 65, 3, "bf16", 0, 0),         # edge tiles of the second stage, two tiles by three
    (1, 8, 200, 33, 65, 3, "f16", 3, 5),
    (1, 64, 200, 3, 5, 8, "f32", 0, 0),
    (1, 16, 1, 3, 5, 1, "bf16", 0, 0),            # N = 1
    (1, 16, 72, 40, 33, 1, "f32", 1, 0),          # 640 features: more than one 512-feature tile per row, the second partly filled
    (0, 16, 264, 3, 5, 3, "f32", 0, 0),
    (0, 8, 264, 33, 65, 3, "bf16", 0, 0),
    (0, 32, 264, 3, 5, 8, "f16", 1, 1),
    (0, 8, 2056, 3, 5, 1, "bf16", 0, 0),          # more than one workgroup along n
]


@pytest.mark.parametrize("case", REDUCE_CASES, ids=["a%d-bs%d-N%d-%dx%d-p%d-%s-m%d%d" % c for c in REDUCE_CASES])
def test_reduce_and_reduced_dw_stay_inside(env, case):
    torch, _lib, L = env
    axis, bs, N, CB, KB, pc, dtype, mis_in, mis_out = case
    rng = np.random.RandomState(N + bs)
    shape = (lambda f: (f, N)) if axis == 0 else (lambda f: (N, f))
    xs = [orc.round_to(rng.normal(0.0, 0.1, shape(CB * bs)).astype(np.float32), dtype) for _ in range(pc)]
    ys = [orc.round_to(rng.normal(0.0, 0.1, shape(KB * bs)).astype(np.float32), dtype) for _ in range(pc)]
    rd = SR.RED_DTYPE[dtype]
    arena = GD.GuardArena(torch, "cuda")
    txs = [arena.place(a, "x%d" % i, mis_in, _td(torch, dtype)) for i, a in enumerate(xs)]
    tys = [arena.place(a, "dy%d" % i, mis_in, _td(torch, dtype)) for i, a in enumerate(ys)]
    st = _lib.raw_stream(txs[0].device)
    need = int(L.bsmm_reduced_dw_workspace_bytes(CB, KB, pc * N))
    assert need % 4 == 0
    for nt, norm in ((0, "max"), (1, "l2")):
        red = []
        for ts, host, fb, name in ((txs, xs, CB, "x_red"), (tys, ys, KB, "y_red")):
            out = arena.alloc((fb, pc, N), _td(torch, rd), name + "-" + norm, mis_out)
            ptrs = (ctypes.c_void_p * pc)(*[t.data_ptr() for t in ts])
            _lib.check(L.bsmm_feature_reduce(ptrs, pc, out.data_ptr(), fb * bs, N, bs, axis, CODE[dtype], nt, st), "bsmm_feature_reduce")
            GD.assert_stored(torch, out, name + " " + norm)
            got = P.to_host(out)
            ref = SR.feature_reduce(host, bs, axis, norm)
            if nt == 0:
                assert np.array_equal(got, orc.round_to(ref, rd)), (case, name)
            else:
                rep = P.block_report(got, ref, rd, fb)
                assert rep["finite"] and rep["elem_bad"] == 0, (case, name, rep)
            red.append((out, got))
        ws = arena.alloc(need // 4, torch.float32, "workspace-" + norm)
        dw = arena.alloc((CB, KB), torch.float32, "dw-" + norm, mis_out)
        _lib.check(L.bsmm_reduced_dw(red[0][0].data_ptr(), red[1][0].data_ptr(), dw.data_ptr(), CB, KB, pc * N, 1.0, 0, CODE[rd], ws.data_ptr(), need, st),
                   "bsmm_reduced_dw")
        GD.assert_stored(torch, dw, "dw " + norm)
        l2, _ = P.errors(P.to_host(dw), SR.reduced_dw(red[0][1], red[1][1]))
        assert l2 <= P.L2_BAR["f32"], (case, norm, l2)
        # accumulate onto what is there; scale 0 stores nothing at all
        before = dw.clone()
        _lib.check(L.bsmm_reduced_dw(red[0][0].data_ptr(), red[1][0].data_ptr(), dw.data_ptr(), CB, KB, pc * N, 0.5, 1, CODE[rd], ws.data_ptr(), need, st),
                   "bsmm_reduced_dw")
        l2, _ = P.errors(P.to_host(dw), 1.5 * P.to_host(before).astype(np.float64))
        assert l2 <= P.L2_BAR["f32"], (case, norm, "accumulate", l2)
        fresh = arena.alloc((CB, KB), torch.float32, "dw-scale0-" + norm, mis_out)
        _lib.check(L.bsmm_reduced_dw(red[0][0].data_ptr(), red[1][0].data_ptr(), fresh.data_ptr(), CB, KB, pc * N, 0.0, 0, CODE[rd], ws.data_ptr(), need, st),
                   "bsmm_reduced_dw")
        assert GD.poisoned(torch, fresh) == fresh.numel()
    arena.check()
    arena.release()
