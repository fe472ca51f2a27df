"""GPU tier for the attention rows that do not fit the register cache of bst_softmax_kernel / bst_softmax_grad_kernel (csrc/bst_kernels.h:
SmCache<VEC>::N = 24 block entries at bsize 8 / 16 / 32, 12 at bsize 64; longer rows run three loops over global memory with the library exp2f
and their own mask and scale handling), for bst_masked_softmax with different input and output types, and for bst_partial_ar_mask_kernel with
more than one workgroup per mask row.  Layouts, inputs and the per-unit criterion come from tests/_bst_long.py; tests/test_bst_softmax_host.py
shows on the CPU that a float32 model of the kernels passes the same calls on the same inputs.  Every report is printed (`FIGURES ...`)."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_bst as G
import _bst_long as BL
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
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda").to(getattr(torch, TD[dt]))


def _np(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def _err(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-30)


def _same_masks(bst, mask_np):
    """the instance packed the masks the oracle was evaluated with"""
    if mask_np is None:
        assert bst.softmax_mask_np is None
    else:
        assert np.array_equal(bst.softmax_mask_np, mask_np)


@pytest.mark.parametrize("xdt,ydt", BL.TYPE_PAIRS, ids=["%s-%s" % p for p in BL.TYPE_PAIRS])
@pytest.mark.parametrize("bsize", BL.BSIZES)
def test_softmax_forward_long_rows(env, bsize, xdt, ydt):
    """Rows of N, N + 1 and 2N + 3 blocks in one launch (N = the register cache): per-head tables with a head-dependent mask and one shared table
    without a mask, probabilities from ~1 down to fp16 subnormals and zeros, all four (input, output) type pairs; each unit against the float64
    oracle rounded once; a second call (through masked_softmax(..., dtype=)) is bit-equal."""
    torch, BST = env
    N = BL.cache_entries(bsize)
    for kind in ("per_head", "shared"):
        lay, heads, cb = BL.layout_of(kind, bsize)
        bst = BST(lay, block_size=bsize, heads=heads, mask_callback=cb)
        assert bst.nn_max == 2 * N + 3 and bst.lut_heads == (2 if kind == "per_head" else 1)
        mask_t = bst._table("mask", "cuda") if cb else None
        for amp in BL.FWD_AMPS:
            c = BL.forward_case(bsize, kind, amp, xdt)
            _same_masks(bst, c["mask_np"])
            tx = _tt(torch, c["X"], xdt)
            y1 = bst._softmax_fwd(tx, BL.SCALE, mask_t, getattr(torch, TD[ydt]))
            y2 = bst.masked_softmax(tx, scale=BL.SCALE, dtype=getattr(torch, TD[ydt]))
            assert y1.dtype == y2.dtype == getattr(torch, TD[ydt])
            assert torch.equal(y1, y2), "two identical calls differ"
            w = BL.check_units(_np(y1), c["Y"], c["L"], ydt, "forward b%d %s->%s %s amp %d" % (bsize, xdt, ydt, kind, amp))
            assert w["lengths"] == [N, N + 1, 2 * N + 3]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("bsize", BL.BSIZES)
def test_softmax_backward_long_rows(env, bsize, dt):
    """bst_softmax_grad_kernel on the same rows: probabilities = the once-rounded oracle softmax of scores of amplitude 1 and 3 (largest ~0.4, no
    saturated row), each unit against the float64 gradient rounded once."""
    torch, BST = env
    N = BL.cache_entries(bsize)
    lay, heads, cb = BL.layout_of("per_head", bsize)
    bst = BST(lay, block_size=bsize, heads=heads, mask_callback=cb)
    for amp in BL.BWD_AMPS:
        c = BL.backward_case(bsize, amp, dt)
        dx = bst._softmax_bwd(_tt(torch, c["DY"], dt), _tt(torch, c["Yp"], dt), BL.SCALE)
        w = BL.check_units(_np(dx), c["DX"], c["L"], dt, "backward b%d %s amp %d" % (bsize, dt, amp))
        assert w["lengths"] == [N, N + 1, 2 * N + 3]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("bsize", [32, 64])
def test_long_row_masks(env, bsize, dt):
    """In the row of 2N + 3 blocks: a query row with no visible key comes out uniform over the row's keys (oracle/bst_oracle.py, include/bst.h) and
    finite, a query row with one visible key -- in the row's last block -- is exactly 1 there and exactly 0 elsewhere; everything else to the
    criterion.  Then the partial autoregressive mask with the key inside that last block."""
    torch, BST = env
    tdt = getattr(torch, TD[dt])
    for amp in BL.FWD_AMPS:
        c = BL.mask_case(bsize, amp, dt)
        bst = BST(c["lay"], block_size=bsize, heads=2, mask_callback=c["cb"])
        _same_masks(bst, c["mask_np"])
        tx = _tt(torch, c["X"], dt)
        got = _np(bst._softmax_fwd(tx, BL.SCALE, bst._table("mask", "cuda"), tdt))
        assert np.isfinite(got).all()
        for h in range(2):
            for q, row, what in ((c["qlong"][h], BL.MASKED_ROW, "longest"), (c["qnext"][h], 7, "N + 1")):
                ids = [b for b, _ in c["L"]["nn_list"][h][q]]
                uni = got[:, h, ids, row, :]
                assert np.all(uni == uni.flat[0]) and np.allclose(uni, 1.0 / (len(ids) * bsize), rtol=1e-2), (what, h, np.unique(uni)[:8])
            ids = [b for b, _ in c["L"]["nn_list"][h][c["qlong"][h]]]
            one = got[:, h, ids, BL.ONE_KEY_ROW, :]
            assert np.all(one[:, -1, BL.ONE_KEY_COL] == 1.0) and one.sum() == one.shape[0], (h, one.sum(), one[:, -1, BL.ONE_KEY_COL])
        BL.check_units(got, c["Y"], c["L"], dt, "row masks b%d %s amp %d" % (bsize, dt, amp))
        # the head mask made causal from a key inside the last block of the longest row on
        a = BL.ar_case(bsize, amp, dt)
        bst = BST(a["lay"], block_size=bsize, heads=2, mask_callback=a["cb"])
        ar = bst.partial_autoregressive_mask(BL.ar_key(bsize), "cuda").cpu().numpy().view(O.mask_dtype(bsize))
        assert np.array_equal(ar, a["mask_kernel"])
        got = _np(bst.masked_softmax(_tt(torch, a["X"], dt), scale=BL.SCALE, autoregress_at_key=BL.ar_key(bsize)))
        BL.check_units(got, a["Y"], a["L"], dt, "autoregressive b%d %s amp %d" % (bsize, dt, amp))
        last = [b for b, (q, k) in enumerate(a["L"]["nt_list"][0]) if k == a["lay"].shape[2] - 1]
        cut = BL.ar_key(bsize) % bsize
        assert np.all(got[:, 0, last][..., cut:] == 0) and np.any(got[:, 0, last][..., :cut] != 0)


def test_register_and_three_pass_rows_agree(env):
    """A dense row of 24 blocks runs from registers; the same 24 blocks of scores in a row of 25 whose extra block (the 8th) is masked completely
    run the three passes.  The 24 shared blocks agree within one bf16 step element by element and to tensor L2 < 2e-4 (the bar between two
    implementations of one softmax in tests/test_bst_gpu.py); the masked block is exactly 0."""
    torch, BST = env
    heads, batch = 2, 2
    b24 = BST(np.ones((1, 24), dtype=np.int32), block_size=32, heads=heads)
    b25 = BST(np.ones((1, 25), dtype=np.int32), block_size=32, heads=heads, mask_callback=lambda shape, h, q, k, b: np.full(shape, k != 7))
    assert b24.nn_max == BL.cache_entries(32) and b25.nn_max == BL.cache_entries(32) + 1
    L24 = O.build_luts(np.ones((1, 24), dtype=np.int32))
    for amp in BL.FWD_AMPS:
        x24 = BL.draw((batch, heads, 24, 32, 32), amp, 4242 + amp, "bf16")
        x25 = np.insert(x24, 7, BL.draw((batch, heads, 32, 32), amp, 4243 + amp, "bf16"), axis=2)
        y24 = _np(b24._softmax_fwd(_tt(torch, x24, "bf16"), BL.SCALE, None, torch.bfloat16))
        y25 = _np(b25._softmax_fwd(_tt(torch, x25, "bf16"), BL.SCALE, b25._table("mask", "cuda"), torch.bfloat16))
        assert np.isfinite(y25).all() and np.all(y25[:, :, 7] == 0), "the masked block"
        shared = np.delete(y25, 7, axis=2)
        steps = np.abs(P._ordinal(shared.astype(np.float32), "bf16") - P._ordinal(y24.astype(np.float32), "bf16"))
        rep = P.block_report(shared.reshape(batch * heads, -1), y24.reshape(batch * heads, -1), "bf16", batch * heads)
        print("FIGURES register against three-pass amp %d: tensor_l2 %.3e group_l2 %.3e elem_flips %d, largest step %d" %
              (amp, rep["tensor_l2"], rep["block_l2"], rep["elem_flips"], steps.max()))
        assert steps.max() <= 1 and rep["tensor_l2"] < 2e-4, (amp, rep, int(steps.max()))
        # and either against the oracle
        BL.check_units(y24, O.masked_softmax(L24, x24, 32, BL.SCALE, None), L24, "bf16", "register row of 24 amp %d" % amp)


@pytest.mark.parametrize("bsize", BL.BSIZES)
def test_partial_autoregressive_mask_many_blocks(env, bsize):
    """64, 65 and 130 blocks per head: one full workgroup of bst_partial_ar_mask_kernel, a second one with a single thread, a third with a tail
    of two; per-head and shared tables.  Bit-equal to the oracle."""
    torch, BST = env
    cases = ((np.ones((1, 8, 8), dtype=np.int32), 1, 64), (np.ones((1, 5, 13), dtype=np.int32), 1, 65),
             (np.ones((2, 5, 13), dtype=np.int32), 2, 65), (np.ones((1, 10, 13), dtype=np.int32), 3, 130))
    for lay, heads, blocks in cases:
        bst = BST(lay, block_size=bsize, heads=heads, mask_callback=G.head_cb)
        assert bst.blocks == blocks
        L = O.build_luts(lay)
        Kb = lay.shape[2]
        for key in (0, (Kb // 2) * bsize + bsize // 2, Kb * bsize - 1):
            got = bst.partial_autoregressive_mask(key, "cuda").cpu().numpy().view(O.mask_dtype(bsize))
            ref = O.partial_autoregressive_mask(bst.softmax_mask, L["nt_lut"], bsize, key)
            assert got.shape == ref.shape and np.array_equal(got, ref), (bsize, blocks, key, int((got != ref).sum()))
            assert not np.array_equal(ref, bst.softmax_mask), "the key masks nothing: nothing tested"


@pytest.mark.parametrize("bsize", [32, 64])
@pytest.mark.parametrize("act,score", [("f32", "bf16"), ("bf16", "bf16"), ("f16", "f16")])
def test_all_ops_long_rows(env, act, score, bsize):
    """nt / nn / tn and both softmax kernels on rows of 2N + 3 blocks (each of the four waves of bst_xn_mfma_kernel takes many steps), with the
    bars of test_bst_gpu.py::test_all_ops_against_oracle."""
    import test_bst_gpu as T
    torch, BST = env
    res = T._run_case(torch, BST, BL.long_rows(bsize), 2, bsize, 64, BL.batch_of(bsize), G.head_cb, 61 + bsize, act, score)
    print("FIGURES all ops b%d %s/%s: %s" % (bsize, act, score, " ".join("%s %.3e" % kv for kv in sorted(res.items()))))
    for k, v in res.items():
        bar = T.L2[score] if k in ("NT", "SM", "SMG") else T.L2[act]
        assert v < bar, (bsize, act, score, k, v)


@pytest.mark.parametrize("act", ["f32", "f16"])
def test_operators_compose_on_long_rows(env, act):
    """query_key_softmax and attention where the fused kernels do not serve (rows of 51 blocks): values and dq / dk / dv against the float64 chain
    with the scores rounded to _score_dtype, at the bars test_bst_gpu.py uses for these operators."""
    torch, BST = env
    bsize, hs, heads, batch = 32, 64, 3, 2
    lay = BL.long_rows_shared(bsize)
    bst = BST(lay, block_size=bsize, heads=heads, mask_callback=G.causal_cb)
    L = O.build_luts(lay)
    score = "f16" if act == "f16" else "bf16"
    assert bst._score_dtype(getattr(torch, TD[act])) == getattr(torch, TD[score])
    inp = G.gen_inputs(np.asarray(lay), heads, bsize, hs, batch, bst.blocks, 71)
    Q, K, V, E = (R.round_to(inp[n], act) for n in ("Q", "K", "V", "E"))
    scale = 1.0 / np.sqrt(hs)
    rs = lambda a: R.round_to(a, score)
    W = rs(O.nt(L, Q, K, bsize, heads))
    A64 = O.masked_softmax(L, W, bsize, scale, bst.softmax_mask_np)
    A = rs(A64)
    Y, DV = O.nn(L, A, V, bsize, heads), O.tn(L, A, E, bsize, heads)
    DW = rs(O.masked_softmax_grad(L, rs(O.nt(L, E, V, bsize, heads)), A, scale))
    DQ, DK = O.nn(L, DW, K, bsize, heads), O.tn(L, DW, Q, bsize, heads)
    q, k, v = (_tt(torch, a, act).requires_grad_(True) for a in (Q, K, V))
    e = _tt(torch, E, act)
    assert bst._nt_softmax(q.detach(), k.detach(), scale, bst._table("mask", "cuda"), getattr(torch, TD[score])) is None
    a = bst.query_key_softmax(q.detach(), k.detach(), scale=scale)
    assert a.dtype == getattr(torch, TD[score])
    figs = {"a": _err(_np(a), A)}
    y = bst.attention(q, k, v, scale=scale)
    y.backward(e)
    ra = lambda t: R.round_to(t, act)
    figs.update(y=_err(_np(y), ra(Y)), dq=_err(_np(q.grad), ra(DQ)), dk=_err(_np(k.grad), ra(DK)), dv=_err(_np(v.grad), ra(DV)))
    print("FIGURES operators on long rows %s: %s" % (act, " ".join("%s %.3e" % kv for kv in figs.items())))
    for name, bar in (("a", 1e-3), ("y", 1e-3), ("dq", 1e-2), ("dk", 1e-2), ("dv", 1e-3)):
        assert figs[name] < bar, (act, name, figs[name])
