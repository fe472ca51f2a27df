"""Memory-contract tier of the attention operators (blocksparse_amd/transformer.py) and of SparseProj: the four statements of
tests/test_memory_bounds_gpu.py -- the route the case is there for was taken, no guard byte around any input or output changed, every output
element stored and none computed from poisoned memory, values within tests/test_bst_gpu.py's bars of oracle/bst_oracle.py -- for nt, nn, tn,
masked softmax, its gradient and the fused scores + softmax pair, over that file's layouts: G.MATH_CASES, the ragged layout (empty query rows
and key columns), block sizes 8 / 16 / 32 / 64, head states the fused kernel takes (32 / 64 / 128) and one it does not, a query row of
exactly 20 blocks (the fused kernel's limit, NTS_MAXT tiles of four) and one of 21, which must take the two-launch route, and the layouts of
tests/_bst_long.py, whose query rows do not fit the register cache of the softmax kernels (the three-pass path)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_bst as G
import _bst_long as BL
import _guard as GD
from oracle import bst_oracle as O
from oracle import bsmm_oracle as R

pytestmark = pytest.mark.gpu
L2 = {"f32": 2e-6, "f16": 1e-3, "bf16": 1e-3}          # tests/test_bst_gpu.py
TD = {"f32": "float32", "f16": "float16", "bf16": "bfloat16"}


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from blocksparse_amd import BlocksparseTransformer, SparseProj, transformer, sparse_proj, _lib
    _lib.load()
    return torch, BlocksparseTransformer, SparseProj, transformer, sparse_proj


def _ragged():
    lay = np.zeros((2, 5, 7), dtype=np.int32)
    lay[0, 1, 2] = lay[0, 1, 6] = lay[0, 4, 0] = 1
    lay[1, 0, 0] = lay[1, 3, 3] = lay[1, 3, 4] = 1
    return lay


def _layout(key):
    if key == "ragged":
        return _ragged()
    if key == "row20":
        return np.ones((1, 3, 20), dtype=np.int32)
    if key == "row21":
        return np.ones((1, 2, 21), dtype=np.int32)
    if key == "local32":
        return O.local_strided_layout(32)
    if key == "one":
        return np.ones((1, 1, 1), dtype=np.int32)
    if key.startswith("long_rows_shared_b"):
        return BL.long_rows_shared(int(key[len("long_rows_shared_b"):]))
    if key.startswith("long_rows_b"):
        return BL.long_rows(int(key[len("long_rows_b"):]))
    return G.layouts()[key]


# id, layout, heads, bsize, head state, batch, mask callback, activation type, score type, fused kernel serves it
BST_CASES = []
for name, lkey, heads, bsize, hs, batch, cbn, seed in G.MATH_CASES:
    for act, score in (("f32", "bf16"), ("f16", "f16"), ("bf16", "bf16")):
        BST_CASES.append(("%s-%s" % (name, act), lkey, heads, bsize, hs, batch, cbn, act, score, bsize == 32 and hs in (32, 64, 128)))
for bsize, hs in ((32, 24), (64, 40), (16, 8), (8, 16), (32, 96), (32, 160), (64, 136), (32, 32), (32, 128), (64, 64)):
    BST_CASES.append(("ragged-b%d-hs%d-f32" % (bsize, hs), "ragged", 2, bsize, hs, 2, "head", "f32", "bf16", bsize == 32 and hs in (32, 64, 128)))
for act in ("f16", "bf16"):
    for bsize, hs in ((32, 64), (32, 32), (32, 128), (32, 96), (64, 64), (8, 8), (16, 16)):
        BST_CASES.append(("ragged-b%d-hs%d-%s" % (bsize, hs, act), "ragged", 2, bsize, hs, 2, "head", act, act, bsize == 32 and hs != 96))
for hs in (32, 64, 128):
    BST_CASES.append(("row20-hs%d-bf16" % hs, "row20", 2, 32, hs, 1, None, "bf16", "bf16", True))
BST_CASES.append(("row20-hs64-f32", "row20", 2, 32, 64, 1, None, "f32", "bf16", True))
BST_CASES.append(("row20-hs64-f16", "row20", 2, 32, 64, 2, None, "f16", "f16", True))
BST_CASES.append(("row21-hs64-bf16", "row21", 1, 32, 64, 1, None, "bf16", "bf16", False))
BST_CASES.append(("row21-hs128-f32", "row21", 1, 32, 128, 1, None, "f32", "bf16", False))
BST_CASES.append(("local32-hs64-bf16", "local32", 2, 32, 64, 2, "causal_o", "bf16", "bf16", True))
BST_CASES.append(("local32-hs128-f16", "local32", 2, 32, 128, 1, "causal_o", "f16", "f16", True))
BST_CASES.append(("one-hs64-f32", "one", 3, 32, 64, 1, None, "f32", "bf16", True))
# query rows of N, N + 1 and 2N + 3 blocks (N = SmCache<VEC>::N of csrc/bst_kernels.h): the three-pass softmax and softmax gradient
for bsize, hs, act in ((32, 64, "bf16"), (32, 64, "f16"), (64, 64, "bf16"), (8, 8, "bf16")):
    BST_CASES.append(("long_rows-b%d-hs%d-%s" % (bsize, hs, act), "long_rows_b%d" % bsize, 2, bsize, hs, BL.batch_of(bsize), "head", act, act, False))
BST_CASES.append(("long_rows_shared-b32-hs64-bf16", "long_rows_shared_b32", 3, 32, 64, 2, None, "bf16", "bf16", False))
# the three (activation, score) pairs of by_types (csrc/bst_api.hip) that no operator above composes: nt / nn / tn only (MM_ONLY)
MM_ONLY = set()
for act, score in (("f32", "f16"), ("bf16", "f16"), ("f16", "bf16")):
    for bsize, hs in ((32, 64), (32, 40), (16, 24)):
        BST_CASES.append(("ragged-b%d-hs%d-%s-%s" % (bsize, hs, act, score), "ragged", 2, bsize, hs, 2, "head", act, score, False))
        MM_ONLY.add(BST_CASES[-1][0])
BST_IDS = [c[0] for c in BST_CASES]
assert len(set(BST_IDS)) == len(BST_IDS)


def _err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("case", BST_CASES, ids=BST_IDS)
def test_attention_memory_contract(env, case):
    torch, BST, _, tr, _ = env
    name, lkey, heads, bsize, hs, batch, cbn, act, score, fused_serves = case
    lay = np.asarray(_layout(lkey))
    cb = O.causal_mask_callback if cbn == "causal_o" else G.CALLBACKS[cbn]
    bst = BST(lay, block_size=bsize, heads=heads, mask_callback=cb)
    L = O.build_luts(lay)
    inp = G.gen_inputs(lay, heads, bsize, hs, batch, bst.blocks, 7 + len(name))
    rq, rs = (lambda a: R.round_to(a, act)), (lambda a: R.round_to(a, score))
    Q, K, V, E = rq(inp["Q"]), rq(inp["K"]), rq(inp["V"]), rq(inp["E"])
    W, X, DY = rs(inp["W"]), rs(inp["X"]), rs(inp["DY"])
    scale = 1.0 / np.sqrt(hs)
    tda, tds = getattr(torch, TD[act]), getattr(torch, TD[score])
    arena = GD.GuardArena(torch, "cuda")
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    tq, tk, tv, te = (arena.place(f32(a), n, 0, tda) for n, a in (("q", Q), ("k", K), ("v", V), ("e", E)))
    tw, tx, tdy = (arena.place(f32(a), n, 0, tds) for n, a in (("w", W), ("x", X), ("dy", DY)))
    mask_np = bst.softmax_mask_np
    mask_t = bst._table("mask", "cuda") if cb else None
    Yref = O.masked_softmax(L, X, bsize, scale, mask_np)
    Yr = rs(Yref)
    ty_in = arena.place(f32(Yr), "y", 0, tds)
    outs = {}
    with GD.routed(arena, tr):
        outs["NT"] = bst._nt(tq, tk, tds)
        outs["NN"] = bst._xn(tw, tv, False)
        outs["TN"] = bst._xn(tw, te, True)
        fused = fgrad = None
        if name not in MM_ONLY:
            outs["SM"] = bst._softmax_fwd(tx, scale, mask_t, tds)
            outs["SMG"] = bst._softmax_bwd(tdy, ty_in, scale)
            fused = bst._nt_softmax(tq, tk, scale, mask_t, tds)
            fgrad = bst._nt_softmax_grad(te, tv, ty_in, scale)
            outs["QKS"] = bst.query_key_softmax(tq, tk, scale=scale)          # the operator: fused where served, nt + softmax elsewhere
    torch.cuda.synchronize()
    fails = []
    # (a) the route
    if (fused is not None) != fused_serves or (fgrad is not None) != fused_serves:
        fails.append("(a) fused kernels served %s / %s, the case expects %s" % (fused is not None, fgrad is not None, fused_serves))
    if fused is not None:
        outs["FUSED"] = fused
    if fgrad is not None:
        outs["FGRAD"] = fgrad
    # (b) guards
    for n, side, first, count in arena.report():
        fails.append("(b) %s %s guard: %d byte(s) changed, nearest at %d" % (n, side, count, first))
    # (c) stored
    for n, out in outs.items():
        try:
            GD.assert_stored(torch, out, n)
        except GD.GuardError as err:
            fails.append("(c) " + str(err))
    # (d) oracle, the bars of tests/test_bst_gpu.py
    Wn = rs(O.nt(L, Q, K, bsize, heads))
    Yn = O.masked_softmax(L, Wn, bsize, scale, mask_np)
    refs = {"NT": (Wn, score), "NN": (rq(O.nn(L, W, V, bsize, heads)), act), "TN": (rq(O.tn(L, W, E, bsize, heads)), act), "SM": (Yr, score),
            "SMG": (rs(O.masked_softmax_grad(L, DY, Yr, scale)), score), "QKS": (rs(Yn), score), "FUSED": (rs(Yn), score),
            "FGRAD": (rs(O.masked_softmax_grad(L, rs(O.nt(L, E, V, bsize, heads)), Yr, scale)), score)}
    for n, out in outs.items():
        err = _err(_np(out), refs[n][0])
        if not err < L2[refs[n][1]]:           # (NaN or Inf in the output: err is nan / inf and this fails too)
            fails.append("(d) %s: L2 %.3e >= %.1e" % (n, err, L2[refs[n][1]]))
    arena.release()
    assert not fails, name + "\n  " + "\n  ".join(fails)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("nhidden,nproj,N", [(96, 17, 40), (33, 33, 7), (512, 128, 1000), (70, 1, 1)])
def test_sparse_proj_memory_contract(env, dt, nhidden, nproj, N):
    """gather, scatter, scatter_add, scatter_mul and the gradient of scatter_mul: guards, every element stored, values equal to torch indexing."""
    torch, _, SparseProj, _, spm = env
    td = getattr(torch, TD[dt])
    np.random.seed(nhidden + nproj)
    sp = SparseProj(nhidden, nproj=nproj)
    rs = np.random.RandomState(N)
    arena = GD.GuardArena(torch, "cuda")
    x = arena.place(rs.normal(size=(nhidden, N)).astype(np.float32), "x", 0, td)
    y = arena.place(rs.normal(size=(nproj, N)).astype(np.float32), "y", 0, td)
    dz = arena.place(rs.normal(size=(nhidden, N)).astype(np.float32), "dz", 0, td)
    idx = torch.from_numpy(sp.gather_lut.astype(np.int64)).cuda()
    with GD.routed(arena, spm):
        g = sp.gather(x)
        s = sp.scatter(y)
        a = sp.scatter_add(x, y)
        m = sp.scatter_mul(x, y)
        dx, dy = sp._mul_grad(dz, x, y)
    torch.cuda.synchronize()
    assert len(arena.entries) == 3 + 6
    arena.check()
    for n, out in (("gather", g), ("scatter", s), ("scatter_add", a), ("scatter_mul", m), ("mul_grad dx", dx), ("mul_grad dy", dy)):
        GD.assert_stored(torch, out, n)
    assert torch.equal(g, x[idx])
    z = torch.zeros_like(x); z[idx] = y
    assert torch.equal(s, z)
    ref = x.clone(); ref[idx] = (x[idx].float() + y.float()).to(td)
    assert torch.equal(a, ref)
    ref = x.clone(); ref[idx] = (x[idx].float() * y.float()).to(td)
    assert torch.equal(m, ref)
    rdx = dz.clone(); rdx[idx] = (dz[idx].float() * y.float()).to(td)
    rdy = (dz[idx].float() * x[idx].float()).to(td)
    assert torch.equal(dx, rdx) and torch.equal(dy, rdy)
    arena.release()
