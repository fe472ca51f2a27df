"""CPU tier of the long-row softmax tests (tests/test_bst_long_rows_gpu.py): the layouts do what they are for, and a float32 NumPy model of
bst_softmax_kernel / bst_softmax_grad_kernel (tests/_bst_long.py) passes the very same per-unit _parity.assert_blocks calls, on the very same
inputs, that the GPU file makes -- so the inputs and the criterion are passable by correct single-precision arithmetic before a GPU is involved.
Every report is printed (`FIGURES ...`): the model's figures are what a device run is compared with."""
import numpy as np
import pytest

import _bst_long as BL
from oracle import bst_oracle as O
from oracle import bsmm_oracle as R


@pytest.mark.parametrize("bsize", BL.BSIZES)
def test_layouts_reach_past_the_register_cache(bsize):
    N = BL.cache_entries(bsize)
    lay = BL.long_rows(bsize)
    assert lay.shape == (2, 4, 2 * N + 3)
    L = O.build_luts(lay)                                            # (raises on unequal block counts)
    assert L["nn_max"] == 2 * N + 3 > N and L["blocks"] == 4 * N + 4
    assert BL.row_lengths(L, 0) == [N, N + 1, 0, 2 * N + 3] and BL.row_lengths(L, 1) == [2 * N + 3, 0, N, N + 1]
    for h in range(2):
        for q, ent in enumerate(L["nn_list"][h]):
            if len(ent) in (N, N + 1):
                ks = [k for _, k in ent]
                assert ks != list(range(len(ks))), "a prefix of the key blocks: ent[] would be the identity"
    assert not np.array_equal(lay[0, 0], lay[1, 2]) and not np.array_equal(lay[0, 1], lay[1, 3])       # other subsets in head 1
    sh = BL.long_rows_shared(bsize)
    assert sh.ndim == 2 and np.array_equal(sh, lay[0])
    Ls = O.build_luts(sh)
    assert Ls["lut_heads"] == 1 and BL.row_lengths(Ls, 2) == [N, N + 1, 0, 2 * N + 3]
    for kind in ("per_head", "shared"):
        _, heads, _ = BL.layout_of(kind, bsize)
        assert BL.batch_of(bsize) * heads * Ls["blocks"] * bsize * bsize < 1.5e6
    assert (2 * N + 2) * bsize < BL.ar_key(bsize) < (2 * N + 3) * bsize


def _tiny(y, dt):
    """(subnormals, zeros) among the values of a 16-bit array"""
    smallest_normal = {"f16": 2.0 ** -14, "bf16": 2.0 ** -126}[dt]
    a = np.abs(np.asarray(y, dtype=np.float64))
    return int(((a > 0) & (a < smallest_normal)).sum()), int((a == 0).sum())


@pytest.mark.parametrize("kind", ["per_head", "shared"])
@pytest.mark.parametrize("xdt,ydt", BL.TYPE_PAIRS)
@pytest.mark.parametrize("bsize", BL.BSIZES)
def test_forward_model_meets_the_criterion(bsize, xdt, ydt, kind):
    for amp in BL.FWD_AMPS:
        c = BL.forward_case(bsize, kind, amp, xdt)
        got = BL.model_softmax(c["L"], c["X"], bsize, BL.SCALE, c["mask_np"], ydt)
        w = BL.check_units(got, c["Y"], c["L"], ydt, "model forward b%d %s->%s %s amp %d" % (bsize, xdt, ydt, kind, amp))
        N = BL.cache_entries(bsize)
        assert w["lengths"] == [N, N + 1, 2 * N + 3] and w["units"] == 3 * BL.batch_of(bsize) * c["heads"]
        if amp == 16 and ydt == "f16":
            for name, y in (("oracle", R.round_to(c["Y"], ydt)), ("model", got)):
                sub, zero = _tiny(y, ydt)
                print("b%d %s %s amp 16 fp16 output: %d subnormals, %d zeros (%s)" % (bsize, xdt, kind, sub, zero, name))
                assert sub > 0 and zero > 0, (name, sub, zero)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("bsize", BL.BSIZES)
def test_backward_model_meets_the_criterion(bsize, dt):
    for amp in BL.BWD_AMPS:
        c = BL.backward_case(bsize, amp, dt)
        print("b%d %s amp %d: largest probability %.3f" % (bsize, dt, amp, c["Yp"].max()))
        assert c["Yp"].max() < 0.9, "a saturated row: dy - sum(dy * y) cancels to fp32 noise there"
        got = BL.model_softmax_grad(c["L"], c["DY"], c["Yp"], BL.SCALE, dt)
        BL.check_units(got, c["DX"], c["L"], dt, "model backward b%d %s amp %d" % (bsize, dt, amp))


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("bsize", [32, 64])
def test_mask_cases_model_meets_the_criterion(bsize, dt):
    for amp in BL.FWD_AMPS:
        c = BL.mask_case(bsize, amp, dt)
        got = BL.model_softmax(c["L"], c["X"], bsize, BL.SCALE, c["mask_np"], dt)
        BL.check_units(got, c["Y"], c["L"], dt, "model row masks b%d %s amp %d" % (bsize, dt, amp))
        for h in range(2):
            ids = [b for b, _ in c["L"]["nn_list"][h][c["qlong"][h]]]
            keep = O.unpack_mask(c["mask_np"][h, ids], bsize)                      # [nb, q, k]
            assert keep[:, BL.MASKED_ROW].sum() == 0 and keep[:, BL.ONE_KEY_ROW].sum() == 1 and keep[-1, BL.ONE_KEY_ROW, BL.ONE_KEY_COL]
            uni = got[:, h, ids, BL.MASKED_ROW, :]
            assert np.all(uni == uni.flat[0]) and np.allclose(uni, 1.0 / (len(ids) * bsize), rtol=1e-2)
            one = got[:, h, ids, BL.ONE_KEY_ROW, :]
            assert np.all(one[:, -1, BL.ONE_KEY_COL] == 1.0) and one.sum() == one.shape[0]
        a = BL.ar_case(bsize, amp, dt)
        got = BL.model_softmax(a["L"], a["X"], bsize, BL.SCALE, a["mask_np"], dt)
        BL.check_units(got, a["Y"], a["L"], dt, "model autoregressive b%d %s amp %d" % (bsize, dt, amp))
        last = [b for b, (q, k) in enumerate(a["L"]["nt_list"][0]) if k == a["lay"].shape[2] - 1]
        cut = BL.ar_key(bsize) % bsize
        assert np.all(got[:, 0, last][..., cut:] == 0) and np.any(got[:, 0, last][..., :cut] != 0)


def test_register_and_three_pass_inputs():
    """The pair of test_register_and_three_pass_rows_agree: the model gives the 24 shared blocks the same probabilities with and without a 25th,
    completely masked block in the row."""
    x24 = BL.draw((2, 2, 24, 32, 32), 16, 4242, "bf16")
    x25 = np.insert(x24, 7, BL.draw((2, 2, 32, 32), 16, 4243, "bf16"), axis=2)
    L24, L25 = O.build_luts(np.ones((1, 24), dtype=np.int32)), O.build_luts(np.ones((1, 25), dtype=np.int32))
    m25, _ = O.build_masks(L25, 32, lambda shape, h, q, k, b: np.full(shape, k != 7))
    y24 = BL.model_softmax(L24, x24, 32, BL.SCALE, None, "bf16")
    y25 = BL.model_softmax(L25, x25, 32, BL.SCALE, m25, "bf16")
    assert np.all(y25[:, :, 7] == 0) and np.array_equal(np.delete(y25, 7, axis=2), y24)
