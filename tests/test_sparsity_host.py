"""CPU tier of the dynamic-sparsity operators (include/bsmm_sparsity.h, blocksparse_amd/sparsity.py): the exported symbols, argument
checks that answer before anything is launched, the host arithmetic (workspace size, the number of kept blocks, the relayout index map) and
the float64 reference helper of the GPU tests against a per-element loop.  No compute calls here."""
import ctypes
import os
import re

import numpy as np
import pytest

import _sparsity_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import _lib
    return _lib


def test_sparsity_header_symbols_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "bsmm_sparsity.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(bsmm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.SPARSITY_SYMBOLS), declared ^ set(lib.SPARSITY_SYMBOLS)
    assert not declared & set(lib.SYMBOLS)
    L = lib.load()
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in declared:
        assert hasattr(L, s), s
        getattr(raw, s)


def test_sparsity_sources_read_no_environment_and_keep_no_state():
    """The promise of include/bsmm.h holds for the new translation unit: no getenv, no process-wide switch, no allocation, no host sync."""
    src = ""
    for f in ("bsmm_sparsity.hip", "bsmm_sparsity_kernels.h"):
        src += open(os.path.join(ROOT, "blocksparse_amd", "csrc", f)).read()
    src = re.sub(r"//[^\n]*", "", src)                     # (the comments may say what the code does not do)
    for word in ("getenv", "hipMalloc", "hipFree", "Synchronize", "atomic", "static "):
        assert word not in src, word


def test_argument_checks_answer_before_any_launch(lib):
    L = lib.load()
    one = ctypes.c_void_p(256)           # a non-null, aligned dummy address: never dereferenced
    ARG, UNSUP, WS = -1, -2, -3
    # block norm / decay / prune
    assert L.bsmm_block_norm(None, one, 4, 32, lib.BF16, 0, None) == ARG
    assert L.bsmm_block_norm(one, None, 4, 32, lib.BF16, 0, None) == ARG
    assert L.bsmm_block_norm(one, one, 0, 32, lib.BF16, 0, None) == ARG
    assert L.bsmm_block_norm(one, one, 4, 12, lib.BF16, 0, None) == UNSUP
    assert L.bsmm_block_norm(one, one, 4, 32, 7, 0, None) == UNSUP
    assert L.bsmm_block_norm(one, one, 4, 32, lib.BF16, 2, None) == UNSUP
    assert L.bsmm_block_l2_decay(None, None, 0.05, 1e-12, 4, 32, lib.F32, None) == ARG
    assert L.bsmm_block_l2_decay(one, None, 0.05, 1e-12, 4, 12, lib.F32, None) == UNSUP
    assert L.bsmm_block_threshold_prune(one, None, 0.5, 0, 4, 32, lib.F16, None) == ARG
    assert L.bsmm_block_threshold_prune(one, one, 0.5, 0, 4, 12, lib.F16, None) == UNSUP
    assert L.bsmm_block_prune(None, one, 4, 2, None) == ARG
    assert L.bsmm_block_prune(one, None, 4, 2, None) == ARG
    assert L.bsmm_block_prune(one, one, 4, 5, None) == ARG
    # feature reduce
    arr = (ctypes.c_void_p * 8)(*([256] * 8))
    hole = (ctypes.c_void_p * 2)(256, None)
    assert L.bsmm_feature_reduce(None, 1, one, 64, 64, 32, 1, lib.BF16, 0, None) == ARG
    assert L.bsmm_feature_reduce(arr, 1, None, 64, 64, 32, 1, lib.BF16, 0, None) == ARG
    assert L.bsmm_feature_reduce(hole, 2, one, 64, 64, 32, 1, lib.BF16, 0, None) == ARG
    assert L.bsmm_feature_reduce(arr, 0, one, 64, 64, 32, 1, lib.BF16, 0, None) == ARG
    assert L.bsmm_feature_reduce(arr, 9, one, 64, 64, 32, 1, lib.BF16, 0, None) == ARG
    assert L.bsmm_feature_reduce(arr, 1, one, 48, 64, 12, 1, lib.BF16, 0, None) == UNSUP
    assert L.bsmm_feature_reduce(arr, 1, one, 128, 64, 64, 0, lib.BF16, 0, None) == UNSUP       # bsize 64 is feature axis 1 only
    assert L.bsmm_feature_reduce(arr, 1, one, 64, 64, 32, 2, lib.BF16, 0, None) == UNSUP
    assert L.bsmm_feature_reduce(arr, 1, one, 64, 64, 32, 1, 5, 0, None) == UNSUP
    assert L.bsmm_feature_reduce(arr, 1, one, 72, 64, 32, 1, lib.BF16, 0, None) == ARG         # F is not a multiple of bsize
    assert L.bsmm_feature_reduce(arr, 1, one, 64, 60, 32, 0, lib.BF16, 0, None) == ARG         # feature axis 0: N % 8
    # reduced dW
    need = L.bsmm_reduced_dw_workspace_bytes(3, 5, 600)
    assert need > 0
    assert L.bsmm_reduced_dw(None, one, one, 3, 5, 600, 1.0, 0, lib.BF16, one, need, None) == ARG
    assert L.bsmm_reduced_dw(one, one, None, 3, 5, 600, 1.0, 0, lib.BF16, one, need, None) == ARG
    assert L.bsmm_reduced_dw(one, one, one, 0, 5, 600, 1.0, 0, lib.BF16, one, need, None) == ARG
    assert L.bsmm_reduced_dw(one, one, one, 3, 5, 600, 1.0, 0, lib.F32, one, need, None) == UNSUP
    assert L.bsmm_reduced_dw(one, one, one, 3, 5, 600, 1.0, 0, lib.BF16, None, need, None) == WS
    assert L.bsmm_reduced_dw(one, one, one, 3, 5, 600, 1.0, 0, lib.BF16, one, need - 1, None) == WS
    assert L.bsmm_reduced_dw(one, one, one, 3, 5, 600, 0.0, 0, lib.BF16, one, need, None) == 0    # scale 0: accepted, nothing launched


def test_workspace_bytes_monotone_in_the_contraction(lib):
    L = lib.load()
    assert L.bsmm_reduced_dw_workspace_bytes(0, 5, 100) == 0 and L.bsmm_reduced_dw_workspace_bytes(3, 5, 0) == 0
    for CB, KB in ((3, 5), (33, 65), (128, 128), (1, 1), (512, 512)):
        tiles = -(-CB // 32) * -(-KB // 32)
        last = 0
        for kc in list(range(1, 700, 7)) + [1024, 2112, 8192, 8200, 65536, 1 << 20]:
            b = L.bsmm_reduced_dw_workspace_bytes(CB, KB, kc)
            assert b >= last and b >= tiles * 4096 and b % (tiles * 4096) == 0, (CB, KB, kc, b, last)
            last = b


def test_keep_count():
    from blocksparse_amd import sparsity
    for fn in (sparsity.prune_keep, SR.keep_count):
        assert fn(37, 0.5) == 19
        assert fn(37, 0.9) == 4
        assert fn(37, 0.0) == 37
        assert fn(37, 1.0) == 0


def test_relayout_index_map_on_numpy_inputs():
    from blocksparse_amd import BlocksparseMatMul, sparsity
    rng = np.random.default_rng(4)
    lay = (rng.random((6, 7)) < 0.5).astype(np.int32)
    lay[0, 0] = lay[5, 6] = 1
    lay[2, 3] = 0
    old = BlocksparseMatMul(lay, block_size=8, feature_axis=1)
    new_lay = lay.copy()
    dropped = [tuple(ck) for ck in old.updat_list[1:4]]
    for c, k in dropped:
        new_lay[c, k] = 0
    new_lay[2, 3] = 1
    W = rng.normal(size=old.w_shape).astype(np.float32)
    new, W2 = old.relayout(W, new_lay, init=0.25)
    assert (new.bsize, new.axis, new.z_order) == (old.bsize, old.axis, old.z_order) and new.blocks == old.blocks - 3 + 1
    assert W2.shape == new.w_shape and W2.dtype == W.dtype
    # the new operator's own Morton-ordered list decides where a block lands
    where_old = {ck: w for w, ck in enumerate(old.updat_list)}
    for w, ck in enumerate(new.updat_list):
        if ck == (2, 3):
            assert (W2[w] == 0.25).all()
        else:
            assert ck not in dropped and (W2[w] == W[where_old[ck]]).all()
    assert all(ck not in new.updat_list for ck in dropped)
    assert (W2 == SR.relayout(W, old.updat_list, new.updat_list, 0.25)).all()
    src, dst = sparsity.relayout_map(old.updat_list, new.updat_list)
    assert len(src) == old.blocks - 3 and len(set(dst.tolist())) == len(dst)
    assert [old.updat_list[s] for s in src] == [new.updat_list[d] for d in dst]
    with pytest.raises(ValueError):
        old.relayout(W, np.ones((5, 7)))


def test_cpu_tensors_are_rejected_loudly():
    import torch
    from blocksparse_amd import BlocksparseMatMul, blocksparse_norm, blocksparse_l2_decay, blocksparse_prune
    w = torch.zeros(4, 8, 8)
    for call in (lambda: blocksparse_norm(w), lambda: blocksparse_l2_decay(w), lambda: blocksparse_prune(w, torch.ones(4), 0, sparsity=0.5)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    b = BlocksparseMatMul(np.ones((2, 2)), block_size=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        b.block_reduced_full_dw([torch.zeros(b.i_shape(8))], [torch.zeros(b.o_shape(8))])


def test_reference_helper_against_a_per_element_loop():
    """tests/_sparsity_ref.py (vectorised float64) against the definitions written out element by element, on 2 x 3 blocks."""
    rng = np.random.default_rng(9)
    bs, CB, KB, N, P = 8, 2, 3, 8, 2
    for axis in (0, 1):
        xs = [rng.normal(size=(CB * bs, N) if axis == 0 else (N, CB * bs)) for _ in range(P)]
        ys = [rng.normal(size=(KB * bs, N) if axis == 0 else (N, KB * bs)) for _ in range(P)]
        at = (lambda t, f, n: t[f, n]) if axis == 0 else (lambda t, f, n: t[n, f])
        for norm in ("max", "l2"):
            def red(ts, FB):
                out = np.zeros((FB, P, N))
                for fb in range(FB):
                    for p in range(P):
                        for n in range(N):
                            vals = [at(ts[p], fb * bs + i, n) for i in range(bs)]
                            out[fb, p, n] = max(abs(v) for v in vals) if norm == "max" else sum(v * v for v in vals) ** 0.5
                return out
            xr, yr = red(xs, CB), red(ys, KB)
            np.testing.assert_allclose(SR.feature_reduce(xs, bs, axis, norm), xr, rtol=1e-13)
            np.testing.assert_allclose(SR.feature_reduce(ys, bs, axis, norm), yr, rtol=1e-13)
            old = rng.normal(size=(CB, KB))
            dw = np.zeros((CB, KB))
            for c in range(CB):
                for k in range(KB):
                    dw[c, k] = 0.5 * sum(xr[c, p, n] * yr[k, p, n] for p in range(P) for n in range(N)) + old[c, k]
            np.testing.assert_allclose(SR.reduced_dw(xr, yr, 0.5, old), dw, rtol=1e-12)
            # the dense gradient's block norms, and the bound the reduced score is
            dense = np.zeros((CB * bs, KB * bs))
            for i in range(CB * bs):
                for j in range(KB * bs):
                    dense[i, j] = sum(at(xs[p], i, n) * at(ys[p], j, n) for p in range(P) for n in range(N))
            np.testing.assert_allclose(SR.dense_dw(xs, ys, axis), dense, rtol=1e-12, atol=1e-12)
            bn = np.zeros((CB, KB))
            for c in range(CB):
                for k in range(KB):
                    blk = dense[c * bs:(c + 1) * bs, k * bs:(k + 1) * bs]
                    bn[c, k] = np.abs(blk).max() if norm == "max" else np.sqrt((blk ** 2).sum())
            np.testing.assert_allclose(SR.dense_block_norms(dense, bs, norm), bn, rtol=1e-13)
            assert (SR.reduced_dw(xr, yr) >= bn * (1 - 1e-12)).all()
    # weights: norms, decay, the two gate rules
    W = rng.normal(size=(6, bs, bs))
    W[2] = 0.0
    gate = np.array([1, 0, 1, 1, 0.5, 1], dtype=np.float32)
    for b in range(6):
        flat = [W[b, i, j] for i in range(bs) for j in range(bs)]
        assert SR.block_norm(W, "max")[b] == max(abs(v) for v in flat)
        np.testing.assert_allclose(SR.block_norm(W, "l2")[b], sum(v * v for v in flat) ** 0.5, rtol=1e-13)
        ss = sum(v * v for v in flat)
        d = min(0.3 / (ss + 1e-12) ** 0.5, 1.0)
        want = W[b] if gate[b] == 0 else W[b] - W[b] * d
        np.testing.assert_allclose(SR.l2_decay(W, gate, 0.3, 1e-12)[b], want, rtol=1e-13, atol=1e-300)
    norms = np.array([3.0, 1.0, 2.0, 2.0, 0.0, 5.0])
    assert SR.threshold_gate(norms, 2.0).tolist() == [1, 0, 1, 1, 0, 1]
    assert SR.sparsity_gate(norms, 0.5).tolist() == [1, 0, 1, 0, 0, 1]       # keep 3: the tie at 2.0 goes to the lower id
