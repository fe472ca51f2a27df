"""GPU tier of the attention matmul tests: bst_nt / bst_nn / bst_tn (csrc/bst_kernels.h) on the case table of tests/_bst_mm.py, all six
(activation, score) type pairs of by_types (csrc/bst_api.hip) and the BST_FLAG_FP32_MFMA route.  tests/test_bst_mm_host.py shows on the CPU
that float32 models of the kernels pass these very assertions on these very inputs and that their mutants do not.

Selector cases assert equality of bits with the single selected product rounded once (no tolerance; a mismatch is reported with its
coordinates); random-data cases assert _parity.assert_blocks per unit against the float64 oracle, and for fp32 outputs the unit bar of
_bst_mm.f32_unit_bar.  Which kernel a case reaches follows from csrc/bst_api.hip (restated in _bst_mm.nt_kernel / xn_kernel, printed in
every `FIGURES` line):
  nt  bsize 8 / 16: bst_nt_valu_kernel;  bsize 32 / 64 with head state 32 / 64 / 128: bst_nt_mfma_kernel (staged, NT_NB = 8 tiles per wave),
      its SPLIT form for fp32 activations without the flag;  other head states (96, 40, 8): bst_nt_mfma_direct_kernel (klim tail at 40 and 8);
  nn / tn  bsize 8 / 16: bst_xn_valu_kernel;  bsize 32 / 64: bst_xn_mfma16_kernel for (f16, f16) and (bf16, bf16) at head states that are
      multiples of 32, bst_xn_split_kernel for (f32, bf16) without the flag, bst_xn_mfma_kernel (widening) for everything else -- (f32, f16),
      (f16, bf16), (bf16, f16), the flagged (f32, bf16), and the same-type pairs at head states 40 and 8 (cvalid == false lanes)."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_bst as G
import _bst_mm as M
import _parity as P
from oracle import bst_oracle as O
from oracle import bsmm_oracle as R

pytestmark = pytest.mark.gpu
TD = {"f32": "float32", "f16": "float16", "bf16": "bfloat16"}


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import BlocksparseTransformer
    return torch, BlocksparseTransformer


def _tt(torch, a, dt):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to("cuda").to(getattr(torch, TD[dt]))


def _np(t):
    return t.detach().float().cpu().numpy()


def _nt(torch, bst, a, b, score, flag):
    """bst._nt, or the same call with BST_FLAG_FP32_MFMA (no host class sets the flag)"""
    sdt = getattr(torch, TD[score])
    if not flag:
        return bst._nt(a, b, sdt)
    from blocksparse_amd import _lib, transformer as T
    lut = bst._table("nt_lut", a.device)
    c = torch.empty((a.shape[0], bst.heads, bst.blocks, bst.blk_size, bst.blk_size), dtype=sdt, device=a.device)
    args = bst._args(lut, a.shape[0], a.shape[2] // bst.heads, T._code(a.dtype), T._code(sdt))
    args.flags = _lib.BST_FLAG_FP32_MFMA
    _lib.check(_lib.load().bst_nt(a.data_ptr(), b.data_ptr(), c.data_ptr(), ctypes.byref(args)), "bst_nt")
    return c


def _xn(torch, bst, w, b, trans, flag):
    if not flag:
        return bst._xn(w, b, trans)
    from blocksparse_amd import _lib, transformer as T
    ctx_c = bst.ctx_blks_k if trans else bst.ctx_blks_q
    lut = bst._table("tn_lut" if trans else "nn_lut", b.device)
    c = torch.empty((b.shape[0], ctx_c * bst.blk_size, b.shape[2]), dtype=b.dtype, device=b.device)
    args = bst._args(lut, b.shape[0], b.shape[2] // bst.heads, T._code(b.dtype), T._code(w.dtype))
    args.flags = _lib.BST_FLAG_FP32_MFMA
    fn = _lib.load().bst_tn if trans else _lib.load().bst_nn
    _lib.check(fn(w.data_ptr(), b.data_ptr(), c.data_ptr(), ctypes.byref(args)), "bst_tn" if trans else "bst_nn")
    return c


def _bst(BST, c, cb=None):
    bst = BST(M.LAYOUTS[c["lay"]], block_size=c["bs"], heads=c["heads"], mask_callback=cb)
    L = M.luts(c["lay"])
    assert bst.lut_heads == L["lut_heads"] and bst.blocks == L["blocks"] and np.array_equal(bst.nt_lut, L["nt_lut"])
    return bst


def _kernel(c, op):
    return M.nt_kernel(c["bs"], c["hs"], c["act"], c["flag"]) if op.startswith("nt") else M.xn_kernel(c["bs"], c["hs"], c["act"], c["score"], c["flag"])


def _selectors(torch, BST, cases, ops=M.SEL_OPS):
    """Section A on every case of the list; all cases are examined before anything is raised."""
    fails = []
    for c in cases:
        bst = _bst(BST, c)
        for op in ops:
            inp = M.selector_case(c, op)
            if op in ("nn", "tn"):
                got = _xn(torch, bst, _tt(torch, inp["W"], c["score"]), _tt(torch, inp["B"], c["act"]), op == "tn", c["flag"])
            else:
                got = _nt(torch, bst, _tt(torch, inp["Q"], c["act"]), _tt(torch, inp["K"], c["act"]), c["score"], c["flag"])
            assert got.dtype == getattr(torch, TD[c["act"] if op in ("nn", "tn") else c["score"]])
            try:
                n = M.assert_bits(_np(got), inp["want"], "%s %s [%s]" % (c["id"], op, _kernel(c, op)))
                print("FIGURES %s %s [%s]: %d elements bit-equal" % (c["id"], op, _kernel(c, op), n))
            except AssertionError as err:
                print("FIGURES " + str(err))
                fails.append(str(err))
    assert not fails, "%d selector results differ\n  " % len(fails) + "\n  ".join(fails[:8])


def _random(torch, BST, c, ops=("nt", "nn", "tn")):
    """Section B on one case; returns the list lengths examined by nn and tn."""
    bst = _bst(BST, c)
    r = M.random_case(c)
    bar = M.f32_unit_bar(c)["bar"] if c["act"] == "f32" else None
    fails, lengths = [], {}
    for op in ops:
        if op == "nt":
            got, want = _nt(torch, bst, _tt(torch, r["Q"], c["act"]), _tt(torch, r["K"], c["act"]), c["score"], c["flag"]), r["NT"]
        else:
            got = _xn(torch, bst, _tt(torch, r["W"], c["score"]), _tt(torch, r["E" if op == "tn" else "V"], c["act"]), op == "tn", c["flag"])
            want = r["TN" if op == "tn" else "NN"]
        try:
            lengths[op] = M.check_units(_np(got), want, c, op, "%s [%s]" % (c["id"], _kernel(c, op)), bar)["lengths"]
        except AssertionError as err:
            fails.append(str(err))
    assert not fails, "\n".join(fails)
    return lengths


@pytest.mark.parametrize("kind", [k[0] for k in M.A_KINDS])
@pytest.mark.parametrize("bs,hs", M.A_SHAPES, ids=["b%d-hs%d" % s for s in M.A_SHAPES])
def test_selector_operands(env, bs, hs, kind):
    """Section A: nt with a one-hot Q, nt with a one-hot K, nn and tn with one +-2^s score per output row, for the six type pairs and the
    flagged (f32, bf16) route, on a per-head layout (lut_heads == heads, 2 heads x 2 batch entries) or a shared 2-D layout (lut_stride == 0, 3
    heads), each with an empty query row and an empty key column.  Kernels by (bsize, head state): see the module docstring -- head states 32 /
    64 / 128 staged nt and mfma16, 96 direct nt and mfma16 with three feature tiles, 40 and 8 direct nt with the klim tail and split / widening
    xn with cvalid == false lanes, bsize 8 / 16 the V_FMA kernels with BS * hs no multiple of 256."""
    torch, BST = env
    cases = M.section("A", bs=bs, hs=hs, lay=kind)
    assert len(cases) == len(M.VARIANTS)
    _selectors(torch, BST, cases)


@pytest.mark.parametrize("bs,hs", M.B_SHAPES, ids=["b%d-hs%d" % s for s in M.B_SHAPES])
def test_random_data_per_unit(env, bs, hs):
    """Section B: the six type pairs on G.gen_inputs data, fp32 activations also on full-significand data; nt per block, nn / tn per (batch
    entry, head, output row-block).  b32-hs64: staged nt (SPLIT for fp32), mfma16 / split / widening xn; b32-hs40: direct nt, split / widening
    xn; b64-hs32: staged nt, four tiles per block; b16-hs24: the V_FMA kernels."""
    torch, BST = env
    cases = M.section("B", bs=bs, hs=hs)
    assert len(cases) == 8
    fails = []
    for c in cases:
        try:
            _random(torch, BST, c)
        except AssertionError as err:
            fails.append(str(err))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("heads,batch,lkey", M.C_PAIRS, ids=["h%dn%d" % p[:2] for p in M.C_PAIRS])
def test_more_than_eight_head_batch_pairs(env, heads, batch, lkey):
    """Section C: hp = xcd + 8 * grp of xcd_head_map with grp > 0 -- 9, 10, 9, 16 and 17 (head, batch entry) pairs, per-head and shared
    tables; section A for (bf16, bf16) and (f32, bf16) at bsize 32 / hs 64 (staged nt and its SPLIT form, mfma16, split xn) and (f16, f16) at
    bsize 64 / hs 32 (staged nt, mfma16)."""
    torch, BST = env
    cases = M.section("C", heads=heads, batch=batch)
    assert len(cases) == 3 and heads * batch > 8
    _selectors(torch, BST, cases)


@pytest.mark.parametrize("act,score", [("bf16", "bf16"), ("f32", "bf16")])
def test_fused_pair_with_nine_head_batch_pairs(env, act, score):
    """bst_nt_softmax_kernel and its GRAD form (SPLIT for fp32 activations) at 3 heads x 3 batch entries, per-head tables and a head-dependent
    mask, against the two-launch path at the bars of tests/test_bst_gpu.py: no element more than one step away and tensor L2 < 2e-4 forward,
    tensor L2 < 3e-4 for the gradient."""
    torch, BST = env
    c = M.BY_ID["C-c_per_head3-h3n3-b32-hs64-%s-%s" % (act, score)]
    bst = _bst(BST, c, G.head_cb)
    L = M.luts(c["lay"])
    inp = G.gen_inputs(np.asarray(M.LAYOUTS[c["lay"]]), 3, 32, 64, 3, bst.blocks, c["seed"])
    scale = 1.0 / np.sqrt(64)
    sdt = getattr(torch, TD[score])
    tq, tk, tv, te = (_tt(torch, R.round_to(inp[n], act), act) for n in ("Q", "K", "V", "E"))
    mask_t = bst._table("mask", "cuda")
    assert mask_t.shape[0] == 3
    fused = bst._nt_softmax(tq, tk, scale, mask_t, sdt)
    assert fused is not None, "the fused kernel serves this configuration"
    two = bst._softmax_fwd(bst._nt(tq, tk, sdt), scale, mask_t, sdt)
    nblk = fused.numel() // 1024
    rep = P.block_report(_np(fused).reshape(-1, 1024), _np(two).astype(np.float64).reshape(-1, 1024), score, nblk)
    print("FIGURES fused forward h3n3 %s/%s: tensor_l2 %.3e elem_flips %d elem_bad %d" % (act, score, rep["tensor_l2"], rep["elem_flips"], rep["elem_bad"]))
    assert rep["finite"] and rep["elem_bad"] == 0 and rep["tensor_l2"] < 2e-4, rep
    assert np.count_nonzero(_np(two)) > 0.5 * two.numel(), "mostly zeros: nothing compared"
    Yp = R.round_to(O.masked_softmax(L, R.round_to(inp["X"], score), 32, scale, bst.softmax_mask_np), score)
    ty = _tt(torch, Yp, score)
    fgrad = bst._nt_softmax_grad(te, tv, ty, scale)
    assert fgrad is not None
    two = bst._softmax_bwd(bst._nt(te, tv, sdt), ty, scale)
    rep = P.block_report(_np(fgrad).reshape(-1, 1024), _np(two).astype(np.float64).reshape(-1, 1024), score, nblk)
    print("FIGURES fused gradient h3n3 %s/%s: tensor_l2 %.3e elem_flips %d elem_bad %d" % (act, score, rep["tensor_l2"], rep["elem_flips"], rep["elem_bad"]))
    assert rep["finite"] and rep["tensor_l2"] < 3e-4, rep
    assert np.count_nonzero(_np(two)) > 0.5 * two.numel(), "mostly zeros: nothing compared"


@pytest.mark.parametrize("hs", M.D_HS)
@pytest.mark.parametrize("bs", sorted(M.D_NB))
def test_nt_walk_edges(env, bs, hs):
    """Section D: a 3 x 6 layout whose first nb cells are present (bsize 32: nb = 1, 2, 7, 8, 9, 10, 15, 16, 17; bsize 64: 1 .. 5, four tiles a
    block), so ntiles % 8 is 0, 1, 2, 4 and 7 and the query row changes inside a walk.  hs 32 / 64 / 128: bst_nt_mfma_kernel -- the tb + 1 and
    tb + 2 look-ahead guards, the conditional Q DMA, qsplit_row of the SPLIT form; hs 40 / 96: bst_nt_mfma_direct_kernel, four tiles per
    workgroup with the tb >= ntiles exit.  (f32, bf16) split and flagged, (bf16, bf16), (f16, bf16); both selector forms and random data."""
    torch, BST = env
    cases = M.section("D", bs=bs, hs=hs)
    assert len(cases) == 4 * len(M.D_NB[bs])
    _selectors(torch, BST, cases, ("nt_q", "nt_k"))
    fails = []
    for c in cases:
        try:
            _random(torch, BST, c, ("nt",))
        except AssertionError as err:
            fails.append(str(err))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("lkey", ["steps", "steps_t"])
@pytest.mark.parametrize("bs,hs", M.E_SHAPES, ids=["b%d-hs%d" % s for s in M.E_SHAPES])
def test_xn_step_edges(env, bs, hs, lkey):
    """Section E: a 9 x 13 layout with query rows of 0, 1, 2, 3, 4, 5, 8, 9 and 13 blocks (nn) and its transpose (tn meets the same counts):
    four waves take every fourth step, prefetch q + 4 and reduce through LDS; bsize 64 doubles the steps (26: seven for wave 0, three changes
    of LDS buffer in bst_xn_mfma16_kernel).  (f32, bf16): bst_xn_split_kernel, flagged: bst_xn_mfma_kernel; (bf16, bf16) and (f16, f16):
    bst_xn_mfma16_kernel (hs 40: the widening kernel); (f16, bf16): bst_xn_mfma_kernel.  Selectors and random data per unit."""
    torch, BST = env
    cases = M.section("E", bs=bs, hs=hs, lay=lkey)
    assert len(cases) == 5
    _selectors(torch, BST, cases, ("nn", "tn"))
    fails = []
    for c in cases:
        try:
            lengths = _random(torch, BST, c, ("nn", "tn"))
            assert lengths["tn" if lkey == "steps_t" else "nn"] == [1, 2, 3, 4, 5, 8, 9, 13], (c["id"], lengths)
        except AssertionError as err:
            fails.append(str(err))
    assert not fails, "\n".join(fails)
