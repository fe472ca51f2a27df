"""Float64 helpers and seeded inputs of the tests of include/bsmm_ends.h (softmax cross-entropy, embedding lookup).  Inputs are pre-rounded
to the storage type, so the device and the float64 definitions below see the same numbers; nothing here touches a device."""
import functools

import numpy as np

import _parity as P
from oracle import bsmm_oracle as orc

F16_SCALE = 32768.0
CHUNK = 128                     # BSMM_EMBED_CHUNK (tests/test_ends_host.py holds it against the header)


def rounded(a, dtype):
    """float32 array holding values of the storage type"""
    a = np.asarray(a, dtype=np.float32)
    return a if dtype == "f32" else orc.round_to(a, dtype).astype(np.float32)


# ---- softmax cross-entropy -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def xent_inputs(N, K, dtype, dist, seed=0):
    """(X float32 (N, K) of storage values, labels int64 [N], dy float32 [N]).  dist: 'normal' = N(0, 1), 'uniform' = U(-20, 20).  The last
    row has every logit equal and the one before it a single +60 outlier (when there are that many rows); from four rows on, every seventh
    row is ignored: its label is -1 or K in turn."""
    rng = np.random.RandomState(1000 * seed + 7 * N + K)
    X = rng.standard_normal((N, K)) if dist == "normal" else rng.uniform(-20.0, 20.0, (N, K))
    if N >= 2:
        X[N - 1, :] = X[N - 1, 0]
    if N >= 3:
        X[N - 2, rng.randint(K)] += 60.0
    labels = rng.randint(0, K, size=N).astype(np.int64)
    if N >= 4:
        ign = np.arange(3, N, 7)
        labels[ign] = np.where(np.arange(ign.size) % 2 == 0, -1, K)
    dy = rounded(rng.uniform(0.5, 2.0, N) * np.where(rng.rand(N) < 0.5, -1.0, 1.0), "f32")
    X, dy = rounded(X, dtype), np.asarray(dy, dtype=np.float32)
    X.setflags(write=False), labels.setflags(write=False), dy.setflags(write=False)
    return X, labels, dy


MASKS = ("head", "tail", "stripes", "unit0", "single", "only_label")
MASKED_LABEL_ROW = MASKS.index("stripes")            # the row of xent_masked_inputs whose label names a masked class


@functools.lru_cache(maxsize=None)
def xent_masked_inputs(K, dtype, seed=0):
    """(X float32 (6, K) of storage values, labels int64 [6]): U(-20, 20) rows, row i with the pattern MASKS[i] of classes set to -inf (a
    class of probability 0).  head: [0, 8 * 1024) clipped to K - 1 so that one class stays finite -- the first unit of every lane of the
    streamed kernel on both access widths; tail: the last third; stripes: every other run of 8; unit0: 0 .. 7; single: 5; only_label:
    all but the label.  Every label names a finite class, except the one of row MASKED_LABEL_ROW, which names a masked one."""
    rng = np.random.RandomState(500 * seed + 3 * K + 1)
    X = rng.uniform(-20.0, 20.0, (len(MASKS), K))
    k = np.arange(K)
    masked = {"head": k < min(8 * 1024, K - 1), "tail": k >= K - K // 3, "stripes": (k // 8) % 2 == 0, "unit0": k < min(8, K - 1),
              "single": k == min(5, K - 2)}
    labels = np.zeros(len(MASKS), dtype=np.int64)
    for i, name in enumerate(MASKS):
        if name == "only_label":
            labels[i] = rng.randint(K)
            off = k != labels[i]
        else:
            off = masked[name]
            pool = np.nonzero(off if i == MASKED_LABEL_ROW else ~off)[0]
            labels[i] = pool[rng.randint(pool.size)]
        X[i, off] = -np.inf
    X = rounded(X, dtype)
    X.setflags(write=False), labels.setflags(write=False)
    return X, labels


def xent_ref(X, labels):
    """(loss, g, p, dist) in float64 by the log-sum-exp identity: g = softmax - onehot UNSCALED, zero on ignored rows; p = softmax; dist =
    |x - max| per element (the growth term of the fp32 bound).  A -inf logit is a class of probability 0 (its dist is +inf); a label on
    it gives loss +inf; a row with no finite logit, with +inf or with NaN is NaN."""
    x = np.asarray(X, dtype=np.float64)
    N, K = x.shape
    labels = np.asarray(labels, dtype=np.int64)
    live = (labels >= 0) & (labels < K)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = x.max(axis=1)
        lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
        p = np.exp(x - lse[:, None])
        onehot = np.zeros((N, K))
        onehot[np.nonzero(live)[0], labels[live]] = 1.0
        xl = x[np.arange(N), np.where(live, labels, 0)]      # (indexed: x * onehot would make NaN of a masked class)
        loss = np.where(live, lse - xl, 0.0)
        g = np.where(live[:, None], p - onehot, 0.0)
        return loss, g, p, np.abs(x - m[:, None])


def xent_long_model_f32(X, labels, V, skip_masked=True, lanes=1024):
    """loss [N] as xent_long_kernel computes it, every operation in float32: lane t of `lanes` visits the units t, t + lanes, ... of V
    elements, keeps a running maximum m and the sum of exp2((x - m) log2 e) without the label's term, rescales the sum when m grows, and
    the lanes merge at the row maximum.  skip_masked=False is the recurrence without the rule that a -inf logit adds 0."""
    f = np.float32
    log2e = f(1.44269504088896340736)
    X = np.asarray(X, dtype=f)
    N, K = X.shape
    units = -(-K // V)
    strips = -(-units // lanes)
    out = np.zeros(N, dtype=f)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(N):
            pad = np.full(strips * lanes * V, np.nan, dtype=f)
            pad[:K] = X[n]
            is_label = np.zeros(pad.size, dtype=bool)
            is_label[labels[n]] = True
            v, lab = pad.reshape(strips, lanes, V), is_label.reshape(strips, lanes, V)
            have = (np.arange(strips * lanes) < units).reshape(strips, lanes)
            m, others = np.full(lanes, -np.inf, dtype=f), np.zeros(lanes, dtype=f)
            for i in range(strips):
                vi = np.where(have[i][:, None], v[i], f(-np.inf))
                mu = np.fmax.reduce(vi, axis=1)
                up = have[i] & (mu > m)
                others = np.where(up, others * np.exp2((m - mu) * log2e), others).astype(f)
                m = np.where(up, mu, m)
                for e in range(V):
                    term = np.exp2((vi[:, e] - m) * log2e).astype(f)
                    zero = lab[i][:, e] | ((vi[:, e] == -np.inf) if skip_masked else False) | ~have[i]
                    others = (others + np.where(zero, f(0), term)).astype(f)
            M = np.fmax.reduce(m)
            others = np.where(m == -np.inf, f(0), others * np.exp2((m - M) * log2e)).astype(f)
            xl = X[n, labels[n]]
            s = f(others.sum(dtype=f) + np.exp2((xl - M) * log2e))
            out[n] = f(np.log(s)) + (M - xl)
    return out


def stash_scale(dtype):
    return F16_SCALE if dtype == "f16" else 1.0


def check_16bit(got, want64, dtype, ctx, finite=None):
    """The criterion for a 16-bit g or dx.  `got`: float32 array of storage values; `want64`: the float64 value BEFORE the one rounding (with
    the fp16 scale applied).  Every element equal or adjacent to the once-rounded value, at most 1 % adjacent, tensor L2 <= the bar.
    `finite`: a mask of the elements whose logit is finite -- the criterion is over those (the caller holds the others to exact values)."""
    got = np.asarray(got, dtype=np.float32)
    want64 = np.asarray(want64, dtype=np.float64)
    if finite is not None:
        got, want64 = got[finite], want64[finite]
    want_r = orc.round_to(want64, dtype).astype(np.float32)
    assert np.isfinite(got).all(), (ctx, "non-finite")
    steps = np.abs(P._ordinal(got, dtype) - P._ordinal(want_r, dtype))
    worst = int(steps.max())
    flips = float((steps == 1).mean())
    l2, _ = P.errors(got, want_r)
    print("%s: worst step %d, adjacent share %.2e, L2 %.2e" % (ctx, worst, flips, l2))
    assert worst <= 1, (ctx, "elements two or more steps off", int((steps > 1).sum()), int(np.argmax(steps)))
    assert flips <= 0.01, (ctx, "adjacent share", flips)
    assert l2 <= P.L2_BAR[dtype], (ctx, "tensor L2", l2)


def f32_g_ratio(got, g64, p64, dist, finite=None):
    """`finite`: a mask of the elements whose logit is finite; the maximum is over those (a masked class has p = 0 and |x - m| = inf,
    whose product is no bound: the caller holds those elements to exact values), and the index is into the selected elements.  max over the elements of |got - want| / ((4 + 2 |x - m|) 2^-22 p + 2^-23 |want| + 2^-149), and the flat index of that element.  The
    last term is one step of the fp32 subnormals: the first two are relative to p, and no fp32 number is that close to a p below 2^-126 (the
    row with the +60 outlier has such p: x - max reaches -100).  Without it the first device run measured 9.8 on a p of 1.466e-42 that was
    stored as the nearest subnormal."""
    got = np.asarray(got, dtype=np.float64)
    if finite is not None:
        got, g64, p64, dist = got[finite], g64[finite], p64[finite], dist[finite]
    err = np.abs(got - g64)
    bound = (4.0 + 2.0 * dist) * 2.0 ** -22 * p64 + 2.0 ** -23 * np.abs(g64) + 2.0 ** -149
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    at = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[at]), at


def check_f32_dx(got, g_stored, dy, ctx):
    """An fp32 dx is ONE fp32 product of two fp32 numbers: within half an ulp of the exact product, |got - want| <= 2^-24 |want| (2^-149: the
    spacing of the subnormals, where the relative statement ends)."""
    want = np.asarray(g_stored, dtype=np.float64) * np.asarray(dy, dtype=np.float64)[:, None]
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    bad = err > 2.0 ** -24 * np.abs(want) + 2.0 ** -149
    assert not bad.any(), (ctx, "fp32 dx is not the rounded product", int(bad.sum()), int(np.argmax(bad)))


# ---- embedding ------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("permutation", "tiled", "equal", "skew", "straddle", "outside")


@functools.lru_cache(maxsize=None)
def embed_indices(C, nIdx, pattern, seed=0):
    """int64 indices; a pattern may choose its own length (it says so below)"""
    rng = np.random.RandomState(77 * seed + 13 * C + nIdx)
    if pattern == "permutation":                     # all distinct: as many as the table has rows, at most nIdx
        idx = rng.permutation(C)[:min(C, nIdx)]
    elif pattern == "tiled":                         # arange tiled: equal counts, far apart
        idx = np.arange(nIdx) % C
    elif pattern == "equal":                         # one run across four chunks
        idx = np.full(3 * CHUNK + 5, C - 1)
    elif pattern == "skew":                          # one index holds half
        idx = np.where(rng.rand(nIdx) < 0.5, C // 2, rng.randint(0, C, nIdx))
    elif pattern == "straddle":                      # sorted: [a] * 100, [b] * 60 (over the border at 128), [c] * 200 (over 256), [d] * 50
        a, b, c, d = (np.arange(4) * max(C // 4, 1)) % C
        idx = rng.permutation(np.concatenate([np.full(100, a), np.full(60, b), np.full(200, c), np.full(50, d)]))
    elif pattern == "outside":                       # -1, C and 2^30 mixed in
        idx = rng.randint(0, C, max(nIdx, 8))
        idx[rng.permutation(idx.size)[:max(idx.size // 3, 3)]] = np.resize(np.array([-1, C, 1 << 30]), max(idx.size // 3, 3))
    else:
        raise ValueError(pattern)
    idx = np.asarray(idx, dtype=np.int64)
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def embed_values(C, K, n, dtype, seed=0):
    """(W (C, K), DY (n, K), DYX (n, K)) float32 of storage values; DYX: multiples of 1 / 32 below 4, whose fp32 sums are exact"""
    rng = np.random.RandomState(31 * seed + C + 3 * K + 5 * n)
    W = rounded(rng.standard_normal((C, K)), dtype)
    DY = rounded(rng.standard_normal((n, K)), dtype)
    DYX = (rng.randint(-127, 128, (n, K)) / 32.0).astype(np.float32)
    for a in (W, DY, DYX):
        a.setflags(write=False)
    return W, DY, DYX


def embed_fwd_ref(W, idx):
    out = np.zeros((idx.size, W.shape[1]), dtype=W.dtype)
    live = (idx >= 0) & (idx < W.shape[0])
    out[live] = W[idx[live]]
    return out


def embed_grad_ref(DY, idx, C):
    """dw (C, K) in float64 and the mask of the rows an index names"""
    dw = np.zeros((C, DY.shape[1]), dtype=np.float64)
    live = (idx >= 0) & (idx < C)
    np.add.at(dw, idx[live], np.asarray(DY, dtype=np.float64)[live])
    named = np.zeros(C, dtype=bool)
    named[idx[live]] = True
    return dw, named


def check_dw(got, want64, named, ctx):
    """dw at the fp32 bars over the rows an index names, and exactly zero elsewhere.  The bars are taken over the named rows only: MAX_BAR
    divides by the mean |want|, and the zero rows of a table whose indices name one row in fifty would dilute that mean fifty times (the
    first device run measured 3.1e-5 against 2e-5 that way on 389 rows summed into one of 50; over the named row it is 6e-7)."""
    got = np.asarray(got, dtype=np.float64)
    assert not got[~named].any(), (ctx, "rows no index names")
    if named.any():
        l2, mx = P.errors(got[named], want64[named])
        print("%s: dw L2 %.2e max %.2e" % (ctx, l2, mx))
        assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (ctx, "dw", l2, mx)


def stable_order(idx):
    return np.argsort(np.asarray(idx, dtype=np.int64), kind="stable").astype(np.int32)
