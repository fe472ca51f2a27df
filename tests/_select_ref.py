"""Definitions the row-selection tests lean on (include/bsmm_select.h), independent of blocksparse_amd/select.py:

  * ``order`` / ``selected``      the pinned total order straight from the values by ``np.lexsort`` (no keys);
  * ``rect`` / ``topk_softmax`` / ``softmax_grad`` / ``sparse_relu``      float64 helpers; the scores that decide a selection are the fp32
    products (x * m) * scale the header pins, everything after the selection is float64;
  * ``model_select``              an integer model of the algorithm the kernels run -- keys, the search of at most 32 steps for the k-th key, the tie
    prefix as (earlier waves) + (earlier chunks) + (lower lanes over the chunk's V ballots) + (lower j) on the kernels' element-to-lane
    map -- with switches that each break one rule (the mutants of tests/test_select_host.py);
  * ``named_cases`` and the data sets of the GPU tests.
"""
import numpy as np

from oracle import bsmm_oracle as orc

THRESHOLDS = (512, 1024, 2048)          # BSMM_SELECT_WAVE8_MAX, _WAVE16_MAX, _GROUP2_MAX
MAX_K = 4096
TINY = {"f32": 2.0 ** -126, "f16": 2.0 ** -14, "bf16": 2.0 ** -126}     # the smallest normal of the storage types


# ---- the pinned order from the values -------------------------------------------------------------------------------------------------
def order(v, masked=None):
    """Row-wise (last axis) permutation: value descending, index ascending, -0 == +0, NaN above +inf, masked below all by index."""
    v = np.asarray(v, dtype=np.float64)
    v2 = v.reshape(-1, v.shape[-1])
    m2 = np.zeros(v2.shape, dtype=bool) if masked is None else np.broadcast_to(masked, v.shape).reshape(v2.shape)
    out = np.empty(v2.shape, dtype=np.int64)
    idx = np.arange(v2.shape[1])
    for r in range(v2.shape[0]):
        nan = np.isnan(v2[r])
        val = np.where(nan | m2[r], 0.0, v2[r]) + 0.0            # (-0.0 + 0.0 = +0.0)
        out[r] = np.lexsort((idx, -val, ~nan | m2[r], m2[r]))     # the last key is the primary one
    return out.reshape(v.shape)


def selected(v, k, masked=None):
    o = order(v, masked)
    S = np.zeros(o.shape, dtype=bool)
    np.put_along_axis(S, o[..., :k], True, axis=-1)
    return S


def scores(x, mask, scale):
    """(fp32 scores, masked) as the header pins them."""
    x = np.asarray(x, dtype=np.float32)
    if mask is None:
        return x * np.float32(scale), np.zeros(x.shape, dtype=bool)
    m = np.broadcast_to(np.asarray(mask, dtype=np.float32), x.shape)
    return (x * m) * np.float32(scale), m == 0


# ---- float64 helpers ----------------------------------------------------------------------------------------------------------------------
def rect(x, k, rebase=True):
    v = np.asarray(x, dtype=np.float64)
    o = order(v)
    S = selected(v, k)
    vk = np.take_along_axis(v, o[..., k - 1:k], axis=-1)
    base = np.where(vk > 0, vk, 0.0) if rebase else np.zeros(vk.shape)
    with np.errstate(invalid="ignore"):
        return np.where(S, np.where(v < base, base, v) - base, 0.0)


def topk_softmax(x, k, mask=None, scale=1.0):
    """(y, S): float64 probabilities and the selected set (masked members included)."""
    v32, masked = scores(x, mask, scale)
    S = selected(v32, k, masked)
    live = S & ~masked
    v = v32.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        vmax = np.max(np.where(masked, -np.inf, v), axis=-1, keepdims=True, initial=-np.inf)
        e = np.where(live, np.exp(np.where(live, v - vmax, 0.0)), 0.0)
        s = e.sum(axis=-1, keepdims=True)
        return np.where(live, e / np.where(live.any(axis=-1, keepdims=True), s, 1.0), 0.0), S


def softmax_grad(dy, y, mask=None, scale=1.0):
    dy, y = np.asarray(dy, dtype=np.float64), np.asarray(y, dtype=np.float64)
    m = 1.0 if mask is None else np.asarray(mask, dtype=np.float64)
    return (dy - (dy * y).sum(axis=-1, keepdims=True)) * y * m * float(np.float32(scale))


def sparse_relu(x, alpha=1.0):
    """(y, cut, sigma) in float64: the population variance around the mean."""
    x = np.asarray(x, dtype=np.float64)
    mean = x.mean(axis=-1, keepdims=True)
    sigma = np.sqrt(np.square(x - mean).mean(axis=-1, keepdims=True))
    cut = mean + float(np.float32(alpha)) * sigma
    return np.maximum(x - cut, 0.0), cut, sigma


def relu_rule(dz, y):
    return np.where(np.asarray(y) > 0, np.asarray(dz, dtype=np.float64), 0.0)


# ---- the kernels' algorithm on integers -----------------------------------------------------------------------------------------------
def geometry(K, dtype):
    """(elements per lane, V, waves per team) of the path for rows of K."""
    V = 4 if dtype == "f32" else 8
    if K <= THRESHOLDS[0]:
        return 8, V, 1
    if K <= THRESHOLDS[1]:
        return 16, V, 1
    return (16, V, 2) if K <= THRESHOLDS[2] else (16, V, 4)


def path_name(K, dtype, aligned=True):
    EL, V, NW = geometry(K, dtype)
    name = ("wave%d" % EL) if NW == 1 else ("group%d" % NW)
    return name + ("-wide" if aligned and K % V == 0 else "")


def model_keys(v, masked=None, neg_zero_below=False, masked_by_value=False):
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    mag = b & 0x7fffffff
    key = np.where(b & 0x80000000, (~b) & 0xffffffff, b | 0x80000000)
    if not neg_zero_below:
        key = np.where(mag == 0, 0x80000000, key)
    key = np.where(mag > 0x7f800000, 0xffffffff, key)
    if masked is not None and not masked_by_value:
        key = np.where(masked, 0, key)
    return key


def model_select(v, k, masked=None, EL=8, V=8, NW=1, tie_reversed=False, strict=False, neg_zero_below=False, masked_by_value=False):
    """The selected set of ONE row as the kernels find it.  The switches are the mutants: each breaks one rule of the contract."""
    v = np.asarray(v, dtype=np.float32)
    K = v.shape[0]
    C = EL // V
    assert K <= NW * 64 * EL and 1 <= k <= K
    key = np.zeros(NW * 64 * EL, dtype=np.int64)                 # padding: key 0
    key[:K] = model_keys(v, masked, neg_zero_below, masked_by_value)
    # reg[w, c, lane, j] = key[w * 64 * EL + (c * 64 + lane) * V + j]
    reg = key.reshape(NW, C, 64, V)
    T = 0
    for bit in range(31, -1, -1):
        cand = T | (1 << bit)
        per_wave = [(int((reg[w] > cand).sum()) if strict else int((reg[w] >= cand).sum())) for w in range(NW)]   # EL ballots + popcounts each
        if sum(per_wave) >= k:
            T = cand
        if sum(per_wave) == k:                                   # exactly k keys at or above: the search ends, T is a lower bound of the k-th
            break
    above = int((reg > T).sum())
    need = k - above
    eq = reg == T
    pick = np.zeros(reg.shape, dtype=bool)
    for w in range(NW):
        front = int(eq[:w].sum())                                # the waves before this one, through LDS
        for c in range(C):
            ballots = eq[w, c]                                   # [lane, j]: V ballots of 64 lanes
            below = np.concatenate(([0], np.cumsum(ballots.sum(axis=1))[:-1]))      # sum over j of mbcnt(ballot j)
            for j in range(V):
                pos = front + below + ballots[:, :j].sum(axis=1)
                if tie_reversed:
                    pos = int(eq.sum()) - 1 - pos
                pick[w, c, :, j] = (reg[w, c, :, j] > T) | (ballots[:, j] & (pos < need))
            front += int(ballots.sum())
    return pick.reshape(-1)[:K]


# ---- data ---------------------------------------------------------------------------------------------------------------------------------
def named_cases():
    """name -> (v fp32 [K], k, masked or None): the rows the host tests name."""
    rng = np.random.default_rng(7)
    K = 40
    distinct = rng.permutation(K).astype(np.float32) - 13.0
    tie = np.array([1.0, 0.5, 2.0, 0.25, -1.0], dtype=np.float32)[rng.integers(0, 5, K)]
    tie[[3, 9, 17, 30]] = 2.0
    tie[[1, 5, 12, 22, 35]] = 1.0                                  # four 2s, then 1s across the 6th position
    zero = np.where(np.arange(K) % 2 == 0, -0.0, 0.0).astype(np.float32)
    zero[[4, 11]] = -3.0
    zero[7] = 5.0                                                  # one positive, then +-0 ties by index alone
    mval = rng.normal(size=K).astype(np.float32)
    masked = np.ones(K, dtype=bool)
    masked[[2, 8, 21]] = False                                     # three unmasked, k = 6: three masked ones by index
    mval[[0, 1, 3]] = -50.0                                        # the first masked elements hold the smallest values
    special = rng.normal(size=K).astype(np.float32)
    special[[6, 19]] = np.nan
    special[25] = np.inf
    special[31] = -np.inf
    return {"distinct": (distinct, 6, None), "tie_across_kth": (tie, 6, None), "pm_zero": (zero, 6, None), "many_masked": (mval, 6, masked),
            "nan_inf": (special, 4, None)}


def round_in(a, dtype):
    return orc.round_to(np.asarray(a, dtype=np.float32), dtype).astype(np.float32)


def pool(dtype):
    """Distinct storage-type values inside (-1, 1), enough for a row of MAX_K: every value of a few binades below 1, both signs."""
    if dtype == "bf16":
        mag = (np.arange(0x3700, 0x3f80, dtype=np.uint32) << 16).view(np.float32)          # 2^-17 .. 1: 17 binades of 128
    elif dtype == "f16":
        mag = np.arange(0x3000, 0x3c00, dtype=np.uint16).view(np.float16).astype(np.float32)   # 2^-3 .. 1: 3 binades of 1024
    else:
        mag = (np.arange(1, 4097, dtype=np.float32) / np.float32(4097.0)).astype(np.float32)
    out = np.concatenate((mag, -mag))
    assert len(np.unique(out)) == len(out) >= MAX_K and np.array_equal(round_in(out, dtype), out)
    return out


def distinct_rows(R, K, dtype, rng):
    """Rows of K distinct values of the storage type inside (-1, 1)."""
    p = pool(dtype)
    return np.stack([rng.choice(p, K, replace=False) for _ in range(R)]).astype(np.float32)


def _filled(R, K, k, rng, top, mid, rest):
    """Rows with (k - 1) // 2 elements of ``top``, then enough of ``mid`` (drawn from that list) to reach past the k-th position, the
    others drawn from ``rest``; shuffled.  k < K: the k-th and the (k + 1)-th element of the order hold a value of ``mid``."""
    rows = np.empty((R, K), dtype=np.float32)
    for r in range(R):
        n_top = (k - 1) // 2
        n_mid = min(K - n_top, k - n_top + 1 + int(rng.integers(0, 3)))
        row = np.concatenate((np.full(n_top, top), rng.choice(mid, n_mid), rng.choice(rest, K - n_top - n_mid))).astype(np.float32)
        rows[r] = rng.permutation(row)
    return rows


def tied_rows(R, K, k, rng):
    """Five 16-bit-representable values; the tie across the k-th position (k < K) is one of 1.0."""
    return _filled(R, K, k, rng, 1.5, [1.0], [0.5, -0.25, -1.0])


def zero_rows(R, K, k, rng):
    """+0 and -0 across the k-th position, 1 above and -1 below."""
    return _filled(R, K, k, rng, 1.0, [0.0, -0.0], [-1.0])


def sparse_mask(R, K, k, rng):
    """fp32 (R, K) of zeros and non-zero floats with fewer than k unmasked elements in every row: more than K - k are masked."""
    m = np.zeros((R, K), dtype=np.float32)
    for r in range(R):
        keep = rng.choice(K, (k - 1) // 2 if r % 2 else k - 1, replace=False)
        m[r, keep] = rng.choice(np.array([1.0, 0.5, 2.0], dtype=np.float32), len(keep))
    return m
