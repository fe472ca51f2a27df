"""Float64 reference of the layer norm tests (include/bsmm_norm.h): forward, statistics and the three gradients, vectorised over segments
and independent of the package's NumPy functions; below it, float32 models of the same formulas (what an fp32 kernel can reach on an input,
and the shifted variance form that the kernels once used) and the seeded inputs with an outlier feature.  x is (K, N) for axis 0 and (N, K) for axis 1 (higher ranks are flattened the way the
operator flattens them); g, b have K elements; mean / rstd come back as [S, N]."""
import numpy as np


def _view(a, K, axis, S, dtype=np.float64):
    """axis 0: (S, Ks, N), features on dim 1;  axis 1: (S, Ks, N) too, by moving (N, S, Ks) around -- one layout for all the formulas."""
    a = np.asarray(a, dtype=dtype)
    if axis == 0:
        return a.reshape(S, K // S, -1)
    return a.reshape(-1, S, K // S).transpose(1, 2, 0)


def _unview(a, shape, axis):
    return (a.reshape(shape) if axis == 0 else a.transpose(2, 0, 1).reshape(shape))


def _axis01(x, axis):
    x = np.asarray(x)
    axis = axis + x.ndim if axis < 0 else axis
    assert axis in (0, x.ndim - 1)
    return (0 if axis == 0 else 1), x.shape[axis]


def stats(x, axis=1, segments=1, epsilon=1e-6):
    """(mean, rstd), each [S, N], biased variance as the mean of squared deviations."""
    ax, K = _axis01(x, axis)
    xs = _view(x, K, ax, segments)
    mean = xs.mean(axis=1)
    var = ((xs - mean[:, None, :]) ** 2).mean(axis=1)
    return mean, 1.0 / np.sqrt(var + epsilon)


def pre_activation(x, g, b, axis=1, segments=1, epsilon=1e-6):
    """xhat * g + b in the shape of x (what ReLU is applied to and what masks dy)."""
    ax, K = _axis01(x, axis)
    xs = _view(x, K, ax, segments)
    mean, rstd = stats(x, axis, segments, epsilon)
    gs = np.asarray(g, dtype=np.float64).reshape(segments, K // segments, 1)
    bs = np.asarray(b, dtype=np.float64).reshape(segments, K // segments, 1)
    return _unview((xs - mean[:, None, :]) * rstd[:, None, :] * gs + bs, np.asarray(x).shape, ax)


def forward(x, g, b, axis=1, segments=1, epsilon=1e-6, relu=False):
    y = pre_activation(x, g, b, axis, segments, epsilon)
    return np.maximum(y, 0.0) if relu else y


def backward(dy, x, g, b, axis=1, segments=1, epsilon=1e-6, relu=False):
    """(dx like x, dg [K], db [K])."""
    ax, K = _axis01(x, axis)
    Ks = K // segments
    xs, dys = _view(x, K, ax, segments), _view(dy, K, ax, segments)
    mean, rstd = stats(x, axis, segments, epsilon)
    gs = np.asarray(g, dtype=np.float64).reshape(segments, Ks, 1)
    bs = np.asarray(b, dtype=np.float64).reshape(segments, Ks, 1)
    xhat = (xs - mean[:, None, :]) * rstd[:, None, :]
    if relu:
        dys = np.where(xhat * gs + bs > 0.0, dys, 0.0)
    dg = (dys * xhat).sum(axis=2).reshape(K)
    db = dys.sum(axis=2).reshape(K)
    dyg = dys * gs
    sum1 = (xhat * dyg).sum(axis=1, keepdims=True)
    sum2 = dyg.sum(axis=1, keepdims=True)
    dx = (dyg - (xhat * sum1 + sum2) / Ks) * rstd[:, None, :]
    return _unview(dx, np.asarray(x).shape, ax), dg, db


# ---- float32 models: every operation rounds to float32; NumPy sums pairwise where a kernel's lane sums serially ---------------------------
F32 = np.float32


def stats_f32_two_pass(x, axis=1, segments=1, epsilon=1e-6):
    """(mean, rstd) float32 [S, N]: the mean first, then the mean of squared deviations from it -- what the kernels compute."""
    ax, K = _axis01(x, axis)
    xs = _view(x, K, ax, segments, F32)
    Ks = F32(K // segments)
    mean = xs.sum(axis=1, dtype=F32) / Ks
    d = xs - mean[:, None, :]
    var = (d * d).sum(axis=1, dtype=F32) / Ks
    return mean, F32(1.0) / np.sqrt(var + F32(epsilon))


def stats_f32_shifted(x, axis=1, segments=1, epsilon=1e-6, accumulators=4):
    """(mean, rstd) float32 [S, N] by the form the streamed kernels used before: var = sum (x - c)^2 / Ks - (mean - c)^2 with c = the
    segment's FIRST feature, the squares in serial accumulators (features k, k + accumulators, ...): 4 as the four waves of the axis-0
    kernel kept them, 256 for the lanes of the streamed axis-1 row."""
    ax, K = _axis01(x, axis)
    xs = _view(x, K, ax, segments, F32)
    Ks = F32(K // segments)
    mean = xs.sum(axis=1, dtype=F32) / Ks
    c = xs[:, 0, :]
    d = xs - c[:, None, :]
    sq = d * d
    s2 = np.zeros_like(mean)
    for w in range(accumulators):
        s2 = s2 + np.cumsum(sq[:, w::accumulators, :], axis=1, dtype=F32)[:, -1, :]
    md = mean - c
    var = np.maximum(s2 / Ks - md * md, F32(0))
    return mean, F32(1.0) / np.sqrt(var + F32(epsilon))


def forward_f32(x, g, b, mean, rstd, axis=1, segments=1):
    """y float32 like x from float32 statistics [S, N]: (x - mean) rstd g + b."""
    ax, K = _axis01(x, axis)
    xs = _view(x, K, ax, segments, F32)
    gs = np.asarray(g, dtype=F32).reshape(segments, K // segments, 1)
    bs = np.asarray(b, dtype=F32).reshape(segments, K // segments, 1)
    mean, rstd = np.asarray(mean, dtype=F32), np.asarray(rstd, dtype=F32)
    return _unview((xs - mean[:, None, :]) * rstd[:, None, :] * gs + bs, np.asarray(x).shape, ax)


def backward_f32(dy, x, g, mean, rstd, axis=1, segments=1):
    """(dx like x, dg [K], db [K]) float32 from GIVEN float32 statistics, by the formulas of include/bsmm_norm.h without ReLU."""
    ax, K = _axis01(x, axis)
    Ks = K // segments
    xs, dys = _view(x, K, ax, segments, F32), _view(dy, K, ax, segments, F32)
    gs = np.asarray(g, dtype=F32).reshape(segments, Ks, 1)
    mean, rstd = np.asarray(mean, dtype=F32), np.asarray(rstd, dtype=F32)
    xhat = (xs - mean[:, None, :]) * rstd[:, None, :]
    dg = (dys * xhat).sum(axis=2, dtype=F32).reshape(K)
    db = dys.sum(axis=2, dtype=F32).reshape(K)
    dyg = dys * gs
    sum1 = (xhat * dyg).sum(axis=1, keepdims=True, dtype=F32)
    sum2 = dyg.sum(axis=1, keepdims=True, dtype=F32)
    dx = (dyg - (xhat * sum1 + sum2) * (F32(1.0) / F32(Ks))) * rstd[:, None, :]
    return _unview(dx, np.asarray(x).shape, ax), dg, db


def backward_given_stats(dy, x, g, mean, rstd, axis=1, segments=1):
    """The float64 evaluation of the same formulas from given statistics (no ReLU)."""
    ax, K = _axis01(x, axis)
    Ks = K // segments
    xs, dys = _view(x, K, ax, segments), _view(dy, K, ax, segments)
    gs = np.asarray(g, dtype=np.float64).reshape(segments, Ks, 1)
    mean, rstd = np.asarray(mean, dtype=np.float64), np.asarray(rstd, dtype=np.float64)
    xhat = (xs - mean[:, None, :]) * rstd[:, None, :]
    dyg = dys * gs
    sum1 = (xhat * dyg).sum(axis=1, keepdims=True)
    sum2 = dyg.sum(axis=1, keepdims=True)
    dx = (dyg - (xhat * sum1 + sum2) / Ks) * rstd[:, None, :]
    return _unview(dx, np.asarray(x).shape, ax), (dys * xhat).sum(axis=2).reshape(K), dys.sum(axis=2).reshape(K)


# ---- an outlier in one feature of every segment: the massive-activation dimension of a trained transformer ---------------------------------
# (K, N, axis, S): axis 0 on the 16-byte path, the element path, rows cut into slices, segments, a long column; axis 1 streamed rows on both
# access widths
OUTLIER_CASES = [(512, 8, 0, 1), (512, 5, 0, 1), (1031, 24, 0, 1), (96, 37, 0, 2), (8200, 8, 0, 1), (8193, 3, 1, 1), (8200, 3, 1, 1)]
OUTLIER_SIZES = (30.0, 1000.0)       # (not 1e4: the two-pass float32 model itself reaches 2.8e-5 there)
OUTLIER_MARGIN = 8.0                 # NumPy's pairwise sums against the kernels' lane-serial sums: a margin over the MODEL's error
_outlier_cache = {}


def outlier_dtypes(case):
    return ("f32", "f16", "bf16") if case[0] >= 8193 else ("f32",)


def tie_clearance(want64, dtype, max_bar):
    """Over the elements of a 16-bit result whose flip to the adjacent value would alone exceed the max bar (one step / mean |want| >
    max_bar: the outlier's own elements): the smallest distance of the float64 value from the midpoint of two representable values,
    relative to the value.  inf when there is no such element."""
    from oracle import bsmm_oracle as orc
    w = np.asarray(want64, dtype=np.float64).reshape(-1)
    r = orc.round_to(w, dtype).astype(np.float64)
    bits = 8 if dtype == "bf16" else 11
    step = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(r), 2.0 ** -14))) - (bits - 1))
    big = step / np.abs(w).mean() > max_bar
    if not big.any():
        return np.inf
    return float(((step[big] / 2 - np.abs(w[big] - r[big])) / np.abs(w[big])).min())


def _outlier_attempt(K, N, axis, S, dtype, A, at, attempt):
    from oracle import bsmm_oracle as orc
    rng = np.random.RandomState(31 * K + 7 * N + axis + 1 + 7919 * attempt)
    shape = (K, N) if axis == 0 else (N, K)
    f16 = lambda a: a.astype(np.float16).astype(np.float32)
    X = orc.round_to(f16(rng.normal(0.0, 1.0, shape)), dtype).astype(np.float32)
    E = orc.round_to(f16(rng.normal(0.0, 1.0, shape)), dtype).astype(np.float32)
    G, B = f16(rng.normal(0.0, 1.0, K)), f16(rng.normal(0.0, 1.0, K))
    feats = np.arange(S) * (K // S) + at
    signed = np.where(np.arange(N) % 2 == 0, A, -A).astype(np.float32)
    if axis == 0:
        X[feats, :] = signed[None, :]
    else:
        X[:, feats] = signed[:, None]
    assert np.array_equal(orc.round_to(X, dtype).astype(np.float32), X)
    ax = 0 if axis == 0 else -1
    c = dict(X=X, E=E, G=G, B=B, Y=forward(X, G, B, ax, S))
    c["MEAN"], c["RSTD"] = stats(X, ax, S)
    c["MEAN32"], c["RSTD32"] = c["MEAN"].astype(np.float32), c["RSTD"].astype(np.float32)
    c["DX"], c["DG"], c["DB"] = backward_given_stats(E, X, G, c["MEAN32"], c["RSTD32"], ax, S)
    c["M_MEAN"], c["M_RSTD"] = stats_f32_two_pass(X, ax, S)
    c["M_Y"] = forward_f32(X, G, B, c["M_MEAN"], c["M_RSTD"], ax, S)
    c["M_DX"], c["M_DG"], c["M_DB"] = backward_f32(E, X, G, c["MEAN32"], c["RSTD32"], ax, S)
    return c


def outlier_clearance_needed(c):
    """How far, relative to its value, a 16-bit y or dx of the outlier must stay from a rounding tie: OUTLIER_MARGIN x the largest rstd
    error of the float32 model on this input (the outlier's y is (x - mean) rstd g + b with a negligible b: it moves with rstd) plus
    2^-21, four fp32 roundings of the value itself.  An fp32 evaluation within that rounds to the value that float64 rounds to."""
    return OUTLIER_MARGIN * rel_errors(c["M_RSTD"], c["RSTD"])[1] * np.abs(c["RSTD"]).mean() / np.abs(c["RSTD"]).min() + 2.0 ** -21


def outlier_case(K, N, axis, S, dtype, A, at):
    """Seeded N(0, 1) inputs (through fp16, then the storage type) with x[feature `at` of every segment, n] = +A / -A in turn, the float64
    results, and the float32 two-pass model's results (`M_` keys).  The backward takes the float64 statistics rounded to fp32 (`MEAN32`,
    `RSTD32`), so that it does not depend on the forward under test; its float64 results follow from the same rounded statistics.
    A 16-bit y or dx of the outlier is 30 to 90 times the mean |y|, so ONE step of its storage type is more than the max bar of the dtype:
    where the float64 value lies closer to a rounding tie than fp32 arithmetic can resolve (outlier_clearance_needed), no fp32 kernel can
    be held to the bar.  Such inputs are passed over -- the first seed clear of that is taken (`ATTEMPT`), a condition on the float64
    results alone, as make_case of tests/test_layer_norm_gpu.py does for the ReLU mask."""
    key = (K, N, axis, S, dtype, A, at)
    if key in _outlier_cache:
        return _outlier_cache[key]
    from _parity import MAX_BAR
    for attempt in range(64):
        c = _outlier_attempt(K, N, axis, S, dtype, A, at, attempt)
        if dtype == "f32" or min(tie_clearance(c["Y"], dtype, MAX_BAR[dtype]), tie_clearance(c["DX"], dtype, MAX_BAR[dtype])) >= outlier_clearance_needed(c):
            break
    else:
        raise AssertionError(("no seed clear of a rounding tie", key))
    c["ATTEMPT"] = np.array(attempt)
    for a in c.values():
        a.setflags(write=False)
    _outlier_cache[key] = c
    return c


def rel_errors(got, ref):
    """(L2-relative error, max |diff| / mean |ref|): the two figures of tests/_parity.py errors()"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    d = np.abs(got - ref)
    return np.sqrt((d ** 2).sum()) / max(np.sqrt((ref ** 2).sum()), 1e-30), d.max() / max(np.abs(ref).mean(), 1e-30)


def outlier_bars(c, name, l2_floor, max_floor):
    """The fp32 bars of one result of an outlier case: the project's fp32 bars, or OUTLIER_MARGIN x the float32 model's own error against
    float64 on this very input where that is more.  Returns (l2 bar, max bar, the model's l2, the model's max)."""
    ml2, mmx = rel_errors(c["M_" + name], c[name])
    return max(l2_floor, OUTLIER_MARGIN * ml2), max(max_floor, OUTLIER_MARGIN * mmx), ml2, mmx
