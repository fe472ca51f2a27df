"""Layouts, inputs, a float32 model and the per-unit criterion for the softmax rows that do not fit the register cache of
bst_softmax_kernel / bst_softmax_grad_kernel (csrc/bst_kernels.h: SmCache<VEC>::N block entries, 24 at bsize 8 / 16 / 32 and 12 at bsize 64;
longer rows take three loops over global memory).  Shared by tests/test_bst_softmax_host.py (no GPU: the model must pass the criterion on these
very inputs) and tests/test_bst_long_rows_gpu.py (the kernels must).  NumPy only.

Criterion: _parity.assert_blocks, unchanged, with one group = one workgroup's unit = the blocks of one (batch, head, query row-block).  One
rounding flip of the dominant probability of a peaked row is 4e-3 .. 8e-3 of that ROW's norm in bf16 -- a coin toss no kernel controls; over the
bsize rows of a unit it is at most 1.4e-3 (bsize 8) and usually far less, while a real fault of a unit (a dropped block, an unreduced max, a wrong
mask word) moves every element of it by several steps."""
import functools
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden_bst as G
import _parity as P
from oracle import bst_oracle as O
from oracle import bsmm_oracle as R

SCALE = 0.5
FWD_AMPS = (1, 16)          # scaled scores over ~ +-35 natural-log units at 16: probabilities from ~1 down to ~1e-30 in one row (inside fp32's range)
BWD_AMPS = (1, 3)           # at a saturated row dy - sum(dy * y) cancels to fp32 noise: no single-precision kernel meets an element statement there
TYPE_PAIRS = (("bf16", "bf16"), ("f16", "f16"), ("bf16", "f16"), ("f16", "bf16"))
BSIZES = (8, 16, 32, 64)


def cache_entries(bsize):
    """SmCache<bsize / 8>::N of csrc/bst_kernels.h"""
    return 12 if bsize == 64 else 24


def batch_of(bsize):
    return 1 if bsize == 64 else 2


@functools.lru_cache(maxsize=None)
def _long_rows(bsize):
    N = cache_entries(bsize)
    Kb = 2 * N + 3
    rs = np.random.RandomState(100 + bsize)
    lay = np.zeros((2, 4, Kb), dtype=np.int32)
    for h, lens in enumerate(((N, N + 1, 0, Kb), (Kb, 0, N, N + 1))):
        for q, n in enumerate(lens):
            while True:
                ks = np.sort(rs.permutation(Kb)[:n])
                if n in (0, Kb) or not np.array_equal(ks, np.arange(n)):          # a subset, not a prefix: ent[] is not the identity
                    break
            lay[h, q, ks] = 1
    lay.flags.writeable = False
    return lay


def long_rows(bsize):
    """[2 heads][4 query blocks][2N + 3 key blocks]: query rows of N, N + 1, 0 and 2N + 3 blocks in head 0, of 2N + 3, 0, N and N + 1 in head 1
    (equal block counts, as the per-head tables need); the N and N + 1 rows are seeded random subsets of the key blocks."""
    return _long_rows(bsize)


def long_rows_shared(bsize):
    """Head 0 of long_rows(bsize) as a 2-D layout: one table for all heads (lut_heads == 1, lut_stride == 0); run it with 3 heads."""
    return _long_rows(bsize)[0]


def layout_of(kind, bsize):
    """(layout, heads, mask callback) of the two forward configurations"""
    if kind == "per_head":
        return long_rows(bsize), 2, G.head_cb
    if kind == "shared":
        return long_rows_shared(bsize), 3, None
    raise KeyError(kind)


def row_lengths(L, h):
    return [len(ent) for ent in L["nn_list"][h if L["lut_heads"] > 1 else 0]]


def draw(shape, amp, seed, dtype):
    """N(0, 1) x amp through fp16 and then the storage type, as G.gen_inputs draws X and DY"""
    rs = np.random.RandomState(seed)
    return R.round_to((rs.normal(0.0, 1.0, shape) * amp).astype(np.float16).astype(np.float32), dtype)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.flags.writeable = False
    return arrays


def masks_of(L, bsize, cb):
    """(softmax_mask_np [H, blocks, bs], kernel layout [H, bs, blocks]) or (None, None)"""
    return O.build_masks(L, bsize, cb) if cb is not None else (None, None)


@functools.lru_cache(maxsize=None)
def forward_case(bsize, kind, amp, xdt):
    """Scores and the unrounded float64 softmax of one forward configuration (computed once, shared, read-only)."""
    lay, heads, cb = layout_of(kind, bsize)
    L = O.build_luts(lay)
    X = draw((batch_of(bsize), heads, L["blocks"], bsize, bsize), amp, 7000 + 10 * bsize + amp + (1 if kind == "shared" else 0), xdt)
    mask_np, _ = masks_of(L, bsize, cb)
    Y = O.masked_softmax(L, X, bsize, SCALE, mask_np)
    _frozen(X, Y, mask_np)
    return dict(lay=lay, L=L, heads=heads, cb=cb, X=X, Y=Y, mask_np=mask_np)


@functools.lru_cache(maxsize=None)
def backward_case(bsize, amp, dt):
    """dy, probabilities (the once-rounded oracle softmax of scores of amplitude `amp` under the head mask) and the unrounded float64 gradient."""
    lay, heads, cb = layout_of("per_head", bsize)
    L = O.build_luts(lay)
    shape = (batch_of(bsize), heads, L["blocks"], bsize, bsize)
    X = draw(shape, amp, 8000 + 10 * bsize + amp, dt)
    mask_np, _ = masks_of(L, bsize, cb)
    Yp = R.round_to(O.masked_softmax(L, X, bsize, SCALE, mask_np), dt)
    DY = draw(shape, 1, 9000 + 10 * bsize + amp, dt)
    DX = O.masked_softmax_grad(L, DY, Yp, SCALE)
    _frozen(Yp, DY, DX)
    return dict(lay=lay, L=L, heads=heads, Yp=Yp, DY=DY, DX=DX)


# ---- masks of test_long_row_masks -----------------------------------------------------------------------------------------------------
MASKED_ROW, ONE_KEY_ROW, ONE_KEY_COL = 3, 5, 1      # inside the longest row-block; the lone visible key sits in that row's LAST block


def longest_row(lay, h):
    return int(np.argmax(np.asarray(lay)[h].sum(axis=1)))


def row_mask_cb(bsize):
    """G.head_cb with, in the 2N + 3 row-block of either head, query row 3 masked completely and query row 5 left exactly one visible key, in the
    row's last block; and one more completely masked row (7) in the N + 1 row-block."""
    lay = long_rows(bsize)
    Kb = lay.shape[2]
    qlong = [longest_row(lay, h) for h in range(2)]
    qnext = [int(np.nonzero(lay[h].sum(axis=1) == cache_entries(bsize) + 1)[0][0]) for h in range(2)]

    def cb(shape, h, q, k, b):
        m = G.head_cb(shape, h, q, k, b)
        if q == qlong[h]:
            m[MASKED_ROW, :] = False
            m[ONE_KEY_ROW, :] = False
            if k == Kb - 1:
                m[ONE_KEY_ROW, ONE_KEY_COL] = True
        if q == qnext[h]:
            m[7, :] = False
        return m
    return cb, qlong, qnext


@functools.lru_cache(maxsize=None)
def mask_case(bsize, amp, dt):
    lay = long_rows(bsize)
    L = O.build_luts(lay)
    cb, qlong, qnext = row_mask_cb(bsize)
    X = draw((batch_of(bsize), 2, L["blocks"], bsize, bsize), amp, 6000 + 10 * bsize + amp, dt)
    mask_np, mask_k = masks_of(L, bsize, cb)
    Y = O.masked_softmax(L, X, bsize, SCALE, mask_np)
    _frozen(X, Y, mask_np)
    return dict(lay=lay, L=L, heads=2, cb=cb, qlong=qlong, qnext=qnext, X=X, Y=Y, mask_np=mask_np)


def ar_key(bsize):
    """a key inside the last block of the longest row"""
    return (2 * cache_entries(bsize) + 2) * bsize + bsize // 2 + 1


@functools.lru_cache(maxsize=None)
def ar_case(bsize, amp, dt):
    """masked_softmax(x, autoregress_at_key=ar_key): the head mask with keys from ar_key on made causal (all masked here: every query precedes them)."""
    c = forward_case(bsize, "per_head", amp, dt)
    L = c["L"]
    _, mask_k = masks_of(L, bsize, c["cb"])
    ar_k = O.partial_autoregressive_mask(mask_k, L["nt_lut"], bsize, ar_key(bsize))
    ar_np = np.ascontiguousarray(ar_k.transpose(0, 2, 1))
    Y = O.masked_softmax(L, c["X"], bsize, SCALE, ar_np)
    _frozen(Y, ar_np)
    return dict(c, Y=Y, mask_np=ar_np, mask_kernel=ar_k)


# ---- float32 model of the two kernels' arithmetic --------------------------------------------------------------------------------------
def model_softmax(L, x, bsize, scale, mask_np, ydt):
    """bst_softmax_kernel in NumPy float32: x * (scale * log2 e), -FLT_MAX for masked entries, max, exp2, fp32 sum, one reciprocal, product, one
    rounding to the output type."""
    f = np.float32
    x = np.asarray(x, dtype=f)
    sc2 = f(f(scale) * f(1.4426950408889634))
    neg = f(-3.402823466e+38)
    y = np.zeros_like(x)
    with np.errstate(under="ignore"):
        for h in range(x.shape[1]):
            hl = h if L["lut_heads"] > 1 else 0
            for ent in L["nn_list"][hl]:
                if not ent:
                    continue
                ids = [b for b, _ in ent]
                v = x[:, h, ids] * sc2
                if mask_np is not None:
                    keep = O.unpack_mask(mask_np[hl if mask_np.shape[0] > 1 else 0, ids], bsize)
                    v = np.where(keep[None], v, neg)
                mx = v.max(axis=(1, 3), keepdims=True)
                ex = np.exp2(v - mx, dtype=f)
                rcp = f(1.0) / ex.sum(axis=(1, 3), keepdims=True, dtype=f)
                y[:, h, ids] = ex * rcp
    return R.round_to(y, ydt)


def model_softmax_grad(L, dy, y, scale, dt):
    """bst_softmax_grad_kernel in NumPy float32: fp32 sum(dy * y), then (dy - s) * y * scale, one rounding."""
    f = np.float32
    dy, y = np.asarray(dy, dtype=f), np.asarray(y, dtype=f)
    dx = np.zeros_like(dy)
    for h in range(dy.shape[1]):
        hl = h if L["lut_heads"] > 1 else 0
        for ent in L["nn_list"][hl]:
            if not ent:
                continue
            ids = [b for b, _ in ent]
            d, v = dy[:, h, ids], y[:, h, ids]
            s = (d * v).sum(axis=(1, 3), keepdims=True, dtype=f)
            dx[:, h, ids] = (d - s) * v * f(scale)
    return R.round_to(dx, dt)


# ---- the criterion, per unit -----------------------------------------------------------------------------------------------------------
def check_units(got, want64, L, dtype, ctx=""):
    """_parity.assert_blocks (groups=1) on every unit = the blocks of one (batch, head, query row-block).  Every unit is examined before anything is
    raised; returns the worst figure of each statement and the row lengths examined.  `got` and `want64` are [batch, heads, blocks, bs, bs]."""
    got, want64 = np.asarray(got), np.asarray(want64)
    assert got.shape == want64.shape, (ctx, got.shape, want64.shape)
    worst = dict(tensor_l2=0.0, group_l2=0.0, elem_flips=0, elem_bad=0, units=0)
    fails, lengths = [], set()
    for h in range(got.shape[1]):
        hl = h if L["lut_heads"] > 1 else 0
        for q, ent in enumerate(L["nn_list"][hl]):
            if not ent:
                continue
            ids = [b for b, _ in ent]
            lengths.add(len(ids))
            for n in range(got.shape[0]):
                rep = P.block_report(got[n, h, ids], want64[n, h, ids], dtype, 1)
                worst["tensor_l2"] = max(worst["tensor_l2"], rep["tensor_l2"])
                worst["group_l2"] = max(worst["group_l2"], rep["block_l2"])
                worst["elem_flips"] += rep["elem_flips"]
                worst["elem_bad"] += rep["elem_bad"]
                worst["units"] += 1
                try:
                    P.assert_blocks(got[n, h, ids], want64[n, h, ids], dtype, 1, ctx="%s batch %d head %d query block %d (%d blocks)" % (ctx, n, h, q, len(ids)))
                except AssertionError as err:
                    fails.append((len(ids), str(err)))
    worst["lengths"] = sorted(lengths)
    print("FIGURES %s: tensor_l2 %.3e group_l2 %.3e elem_flips %d elem_bad %d over %d units, rows of %s blocks" %
          (ctx, worst["tensor_l2"], worst["group_l2"], worst["elem_flips"], worst["elem_bad"], worst["units"], worst["lengths"]))
    assert not fails, ("%s: %d of %d units fail, in rows of %s blocks\n  " % (ctx, len(fails), worst["units"], sorted(set(n for n, _ in fails))) +
                       "\n  ".join(msg for _, msg in fails[:6]))
    return worst
