"""Two restatements of include/bsmm_adafactor.h for the Adafactor tests, from the same fp32 / 16-bit inputs the device sees.

``dense`` / ``blocks`` (and their ``*_loop`` twins, which spell the definitions out element by element and are used only by
tests/test_adafactor_host.py): the float64 definitions of the 2-d, the 1-d and the block form, with ``pre``, gate and the skip sentinel.

``model_dense`` / ``model_blocks``: a float32 model that adds in the kernels' own order (blocksparse_amd/csrc/bsmm_adafactor_kernels.h):
lane partials, the wave's xor tree, the four waves in order, slots, the fixed-order final sum -- for the 16-byte path (``vec=True``) and
the element path.  ``x2_chain=True`` is the mutant the host tier needs: every other sum as the kernels do it, the sum of x^2 as ONE
sequential fp32 chain.  An fma is modelled as the float64 product and sum rounded once to fp32.

All functions return ``(param, cv, rv, rms)``: flat arrays (``rv`` is ``None`` for the 1-d form) and the RMS of x the clip compares with
``clip_thresh``."""
import math

import numpy as np

from _optimize_ref import pre

DEFAULTS = dict(lr=5e-4, decay=0.999, epsilon=1e-30, clip_thresh=1.0, grad_scale=1.0, norm_scale=1.0, saturate=0.0, zero_infs=False,
                zero_nans=False)
F = np.float32
SLAB, THREADS, X2_SLOTS, RV_SLOTS, BLK_SLOTS = 32, 256, 2048, 256, 1024


def _opts(kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def decay_loop(t, beta2, zero_init_variables=False):
    """The two accumulators multiplied out call by call: decay1_power holds beta2^t, decay2_power beta2^(2t); both start at 0 and stay
    there with zero_init_variables."""
    b = 0.0 if zero_init_variables else beta2
    d1, d2 = b, b * b
    for _ in range(t - 1):
        d1, d2 = d1 * beta2, d2 * beta2 * beta2
    return beta2 * (1.0 - d1) / (1.0 - d2)


# ---------------------------------------------------------------------------------------------------------------- float64 definitions
def _scaled64(g, o):
    return pre(np.asarray(g), o["zero_infs"], o["zero_nans"], o["saturate"]) * (np.float64(F(o["grad_scale"])) * np.float64(F(o["norm_scale"])))


def _f64(o, *names):
    return [np.float64(F(o[n])) for n in names]


def _rate64(x, o):
    lr, clip = _f64(o, "lr", "clip_thresh")
    rms = math.sqrt(float((x * x).mean()))
    return lr / max(rms / clip, 1.0), rms


def dense(p, cv, rv, g, rows, cols, **kw):
    """The 2-d form (rows > 1) or the 1-d form (rows == 1, rv ignored) in float64."""
    o = _opts(kw)
    p, cv = np.array(p, dtype=np.float64).reshape(-1), np.array(cv, dtype=np.float64).reshape(-1)
    rv = None if rows == 1 else np.array(rv, dtype=np.float64).reshape(-1)
    if o["norm_scale"] == 0.0:
        return p, cv, rv, 0.0
    d, eps = _f64(o, "decay", "epsilon")
    gs = _scaled64(g, o).reshape(rows, cols)
    s = gs * gs + eps
    if rows == 1:
        cv2 = d * cv + (1.0 - d) * s[0]
        x = gs / np.sqrt(cv2)[None, :]
        rv2 = None
    else:
        rv2 = d * rv + (1.0 - d) * s.mean(axis=1)
        cv2 = d * cv + (1.0 - d) * s.mean(axis=0)
        m = rv2.mean()
        x = gs * ((1.0 / np.sqrt(rv2 / m))[:, None] * (1.0 / np.sqrt(cv2))[None, :])
    rate, rms = _rate64(x, o)
    return p - rate * x.reshape(-1), cv2, rv2, rms


def blocks(p, cv, rv, g, nblocks, bs, gate=None, **kw):
    """The block form in float64: every live block a 2-d problem of its own, one rate over the live blocks."""
    o = _opts(kw)
    p, cv, rv = (np.array(a, dtype=np.float64).reshape(-1) for a in (p, cv, rv))
    live = np.ones(nblocks, dtype=bool) if gate is None else np.asarray(gate) != 0
    if o["norm_scale"] == 0.0 or not live.any():
        return p, cv, rv, 0.0
    d, eps = _f64(o, "decay", "epsilon")
    gs = _scaled64(np.where(np.repeat(live, bs * bs), np.asarray(g, dtype=np.float64).reshape(-1), 0.0), o).reshape(nblocks, bs, bs)
    s = gs * gs + eps
    rv2 = d * rv.reshape(nblocks, bs) + (1.0 - d) * s.mean(axis=2)
    cv2 = d * cv.reshape(nblocks, bs) + (1.0 - d) * s.mean(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):     # (gated-off blocks: whatever their slots hold; masked below)
        m = rv2.mean(axis=1)
        x = gs * ((1.0 / np.sqrt(rv2 / m[:, None]))[:, :, None] * (1.0 / np.sqrt(cv2))[:, None, :])
    rate, rms = _rate64(x[live], o)
    le, lm = np.repeat(live, bs * bs), np.repeat(live, bs)
    return (np.where(le, p - rate * x.reshape(-1), p), np.where(lm, cv2.reshape(-1), cv), np.where(lm, rv2.reshape(-1), rv), rms)


def _pre_loop(x, o):
    if o["zero_infs"] and math.isinf(x):
        x = 0.0
    if o["zero_nans"] and math.isnan(x):
        x = 0.0
    if o["saturate"] != 0.0:
        s = o["saturate"]
        x = s if math.isnan(x) else max(min(x, s), -s)
    return x * (float(F(o["grad_scale"])) * float(F(o["norm_scale"])))


def _matrix_loop(p, cv, rv, g, C, K, o):
    """One C x K problem element by element; returns the new moments and x (lists), not yet the step."""
    d, eps = float(F(o["decay"])), float(F(o["epsilon"]))
    gs = [[_pre_loop(float(g[c * K + k]), o) for k in range(K)] for c in range(C)]
    if C == 1:
        cv2 = [d * cv[k] + (1.0 - d) * (gs[0][k] ** 2 + eps) for k in range(K)]
        return cv2, None, [gs[0][k] / math.sqrt(cv2[k]) for k in range(K)]
    rv2 = [d * rv[c] + (1.0 - d) * sum(gs[c][k] ** 2 + eps for k in range(K)) / K for c in range(C)]
    cv2 = [d * cv[k] + (1.0 - d) * sum(gs[c][k] ** 2 + eps for c in range(C)) / C for k in range(K)]
    m = sum(rv2) / C
    x = [gs[c][k] * ((1.0 / math.sqrt(rv2[c] / m)) * (1.0 / math.sqrt(cv2[k]))) for c in range(C) for k in range(K)]
    return cv2, rv2, x


def dense_loop(p, cv, rv, g, rows, cols, **kw):
    o = _opts(kw)
    p, cv = [float(v) for v in np.asarray(p).reshape(-1)], [float(v) for v in np.asarray(cv).reshape(-1)]
    rv = None if rows == 1 else [float(v) for v in np.asarray(rv).reshape(-1)]
    if o["norm_scale"] == 0.0:
        return np.array(p), np.array(cv), None if rv is None else np.array(rv), 0.0
    cv2, rv2, x = _matrix_loop(p, cv, rv, np.asarray(g).reshape(-1), rows, cols, o)
    rms = math.sqrt(sum(v * v for v in x) / len(x))
    rate = float(F(o["lr"])) / max(rms / float(F(o["clip_thresh"])), 1.0)
    return np.array([p[i] - rate * x[i] for i in range(len(p))]), np.array(cv2), None if rv2 is None else np.array(rv2), rms


def blocks_loop(p, cv, rv, g, nblocks, bs, gate=None, **kw):
    o = _opts(kw)
    p, cv, rv = ([float(v) for v in np.asarray(a).reshape(-1)] for a in (p, cv, rv))
    g = np.asarray(g).reshape(-1)
    live = [b for b in range(nblocks) if gate is None or gate[b] != 0]
    if o["norm_scale"] == 0.0 or not live:
        return np.array(p), np.array(cv), np.array(rv), 0.0
    bb, xs, total = bs * bs, {}, 0.0
    for b in live:
        cv2, rv2, x = _matrix_loop(None, cv[b * bs:(b + 1) * bs], rv[b * bs:(b + 1) * bs], g[b * bb:(b + 1) * bb], bs, bs, o)
        cv[b * bs:(b + 1) * bs], rv[b * bs:(b + 1) * bs], xs[b] = cv2, rv2, x
        total += sum(v * v for v in x)
    rms = math.sqrt(total / (len(live) * bb))
    rate = float(F(o["lr"])) / max(rms / float(F(o["clip_thresh"])), 1.0)
    for b in live:
        for i in range(bb):
            p[b * bb + i] -= rate * xs[b][i]
    return np.array(p), np.array(cv), np.array(rv), rms


# ---------------------------------------------------------------------------------------------------------------- the float32 model
def _fma(a, b, c):
    return (np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64) + np.asarray(c, dtype=np.float64)).astype(F)


def _chain(t, axis):
    """One sequential fp32 chain along ``axis``, first term first."""
    t = np.moveaxis(np.asarray(t, dtype=F), axis, 0)
    acc = t[0].copy()
    for i in range(1, t.shape[0]):
        acc = acc + t[i]
    return acc


def _tree(v, masks):
    """The xor tree over the last axis (lanes): v += v[lane ^ m] for every m, in the order given; every lane ends with the same bits."""
    lanes = np.arange(v.shape[-1])
    for m in masks:
        v = v + v[..., lanes ^ m]
    return v


def _wave_sum(v):
    return _tree(np.asarray(v, dtype=F), (32, 16, 8, 4, 2, 1))[..., 0]


def _four(w):
    """((w0 + w1) + w2) + w3 over the last axis: the four waves of a workgroup."""
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def _group_sum(v):
    """256 lanes (last axis): wave_sum per 64, then the four waves in order."""
    return _four(_wave_sum(v.reshape(v.shape[:-1] + (4, 64))))


def _pad(a, axis, multiple):
    n = a.shape[axis]
    extra = (-n) % multiple
    if not extra:
        return a
    width = [(0, 0)] * a.ndim
    width[axis] = (0, extra)
    return np.pad(a, width)


def _slot_sum(slots):
    """adf_slot_sum: lane t adds slots t, t + 256, ..., then the workgroup's sum."""
    s = _pad(np.asarray(slots, dtype=F), 0, THREADS).reshape(-1, THREADS)
    return _group_sum(_chain(s, 0))


def _strided(terms, G):
    """Terms (axis 0) dealt to G owners in turn (owner = index % G); each owner's chain -> [G, ...]."""
    t = _pad(terms, 0, G)
    return _chain(t.reshape((-1, G) + t.shape[1:]), 0)


def _sum_sq(x):
    """adf_sum_sq over the last axis: x0 * x0, then fma(xj, xj, q)."""
    q = x[..., 0] * x[..., 0]
    for j in range(1, x.shape[-1]):
        q = _fma(x[..., j], x[..., j], q)
    return q


def _scaled32(g, o):
    gs = F(o["grad_scale"]) * F(o["norm_scale"])
    with np.errstate(invalid="ignore", over="ignore"):
        return (pre(np.asarray(g, dtype=F), o["zero_infs"], o["zero_nans"], o["saturate"]).astype(F) * gs).astype(F)


def _moment(old, mean, o):
    d = F(o["decay"])
    return _fma(d, old, (F(1.0) - d) * mean)


def _rsqrt(v):
    return F(1.0) / np.sqrt(v, dtype=F)


def _rate32(total, inv_n, o):
    rms = np.sqrt(F(total) * F(inv_n), dtype=F)
    return F(o["lr"]) / max(rms / F(o["clip_thresh"]), F(1.0)), float(rms)


def _seq(x):
    """The mutant's sum: every x^2 of the tensor in one sequential fp32 chain, in memory order."""
    x = np.asarray(x, dtype=F).reshape(-1)
    return np.cumsum(x * x, dtype=F)[-1]


def model_dense(p, cv, rv, g, rows, cols, vec=True, x2_chain=False, **kw):
    o = _opts(kw)
    p, cv = np.array(p, dtype=F).reshape(-1), np.array(cv, dtype=F).reshape(-1)
    rv = None if rows == 1 else np.array(rv, dtype=F).reshape(-1)
    if o["norm_scale"] == 0.0:
        return p, cv, rv, 0.0
    vec = bool(vec) and cols % 4 == 0
    V = 4 if vec else 1
    gs = _scaled32(g, o).reshape(rows, cols)
    eps = F(o["epsilon"])
    if rows == 1:
        return _model_1d(p, cv, gs[0], V, eps, x2_chain, o)
    C, K, CW = rows, cols, THREADS * V
    nslabs, nchunks = -(-C // SLAB), -(-K // CW)
    tiles = lambda a: _pad(_pad(a, 0, SLAB), 1, CW).reshape(nslabs, SLAB, nchunks, THREADS, V)
    s = tiles(_fma(gs, gs, eps))
    # adf2_partial: a lane's chain over the slab's rows per column; a row's V values, the wave, the four waves
    colpart = _chain(s, 1).reshape(nslabs, nchunks * CW)[:, :K]
    rowpart = _group_sum(_chain(s, 4)).reshape(nslabs * SLAB, nchunks)[:C]
    # adf2_finalize
    inv_c, inv_k, inv_n = F(1.0 / C), F(1.0 / K), F(1.0 / (float(C) * float(K)))
    cv2 = _moment(cv, _four(np.moveaxis(_strided(colpart, 4), 0, -1)) * inv_c, o)
    rv2 = _moment(rv, _wave_sum(np.moveaxis(_strided(rowpart.T, 64), 0, -1)) * inv_k, o)
    nrvwg = min(-(-C // 4), RV_SLOTS)
    rvslots = _four(_strided(rv2, nrvwg * 4).reshape(nrvwg, 4))
    m = _slot_sum(rvslots) * inv_c
    # adf2_x2
    x = gs * (_rsqrt(rv2 / m)[:, None] * _rsqrt(cv2)[None, :])
    if x2_chain:
        total = _seq(x)
    else:
        tacc = _chain(_sum_sq(tiles(x)), 1).reshape(nslabs * nchunks, THREADS)
        total = _slot_sum(_group_sum(_strided(tacc, min(nslabs * nchunks, X2_SLOTS))))
    rate, rms = _rate32(total, inv_n, o)
    return _fma(-rate, x.reshape(-1), p), cv2, rv2, rms


def _model_1d(p, cv, gs, V, eps, x2_chain, o):
    K = gs.size
    cv2 = _moment(cv, _fma(gs, gs, eps), o)
    x = gs / np.sqrt(cv2, dtype=F)
    if x2_chain:
        total = _seq(x)
    else:
        units = _sum_sq(x.reshape(-1, V))
        G = min(-(-units.size // THREADS), X2_SLOTS)
        total = _slot_sum(_group_sum(_strided(units, G * THREADS).reshape(G, THREADS)))
    rate, rms = _rate32(total, F(1.0 / K), o)
    return _fma(-rate, x, p), cv2, None, rms


def model_blocks(p, cv, rv, g, nblocks, bs, gate=None, vec=True, x2_chain=False, **kw):
    o = _opts(kw)
    p, cv, rv = (np.array(a, dtype=F).reshape(-1) for a in (p, cv, rv))
    live = np.ones(nblocks, dtype=bool) if gate is None else np.asarray(gate) != 0
    if o["norm_scale"] == 0.0 or not live.any():
        return p, cv, rv, 0.0
    V, bb = (4 if vec else 1), bs * bs
    LPR, ACTIVE = bs // V, min(bb // V, 64)
    STEPS, RPS = bb // (ACTIVE * V), ACTIVE // LPR
    row_masks = [m for m in (32, 16, 8, 4, 2, 1) if m < LPR]
    group_masks = [m for m in (1, 2, 4, 8, 16, 32) if LPR <= m < ACTIVE]
    inv, eps = F(1.0 / bs), F(o["epsilon"])
    gs = _scaled32(np.where(np.repeat(live, bb), np.asarray(g, dtype=F).reshape(-1), F(0)), o).reshape(nblocks, STEPS, ACTIVE, V)
    s = _fma(gs, gs, eps)
    lanes = np.arange(ACTIVE)
    rows = np.arange(STEPS)[:, None] * RPS + (lanes // LPR)[None, :]                      # [STEPS, ACTIVE]
    q = _tree(_chain(s, 3), row_masks)                                                    # the row's sum in every lane of the row
    rnew = _moment(rv.reshape(nblocks, bs)[:, rows], q * inv, o)                          # [nblocks, STEPS, ACTIVE]
    cacc = np.moveaxis(_tree(np.moveaxis(_chain(s, 1), 1, 2), group_masks), 2, 1)         # [nblocks, ACTIVE, V]
    racc = _tree(_chain(rnew, 1), group_masks)
    mb = racc[:, 0] * inv
    cols = ((lanes % LPR) * V)[:, None] + np.arange(V)[None, :]                           # [ACTIVE, V]
    cnew = _moment(cv.reshape(nblocks, bs)[:, cols], cacc * inv, o)                       # [nblocks, ACTIVE, V]
    cv2 = cnew[:, :LPR, :].reshape(nblocks, bs)
    rv2 = rnew[:, :, ::LPR].reshape(nblocks, bs)
    with np.errstate(invalid="ignore", divide="ignore"):     # (gated-off blocks are masked below)
        x = gs * (_rsqrt(rnew / mb[:, None, None])[..., None] * _rsqrt(cnew)[:, None, :, :])
    if x2_chain:
        total = _seq(x[live])
    else:
        per_block = _wave_sum(_pad(_chain(_sum_sq(x), 1), 1, 64))
        per_block = np.where(live, per_block, F(0))
        G = min(-(-nblocks // 4), BLK_SLOTS)
        total = _slot_sum(_four(_strided(per_block, G * 4).reshape(G, 4)))
    rate, rms = _rate32(total, F(1.0) / (F(int(live.sum())) * F(bb)), o)
    le, lm = np.repeat(live, bb), np.repeat(live, bs)
    p2 = _fma(-rate, x.reshape(-1), p)
    return np.where(le, p2, p), np.where(lm, cv2.reshape(-1), cv), np.where(lm, rv2.reshape(-1), rv), rms
