"""float64 restatement of include/bsmm_optim.h for the optimizer tests: the Adam step, the moving average, the sum of squares and the clip,
from the same fp32 / 16-bit inputs the device sees.  Vectorised NumPy; the ``*_loop`` twins spell the same definitions out element by
element and are used only by tests/test_optimize_host.py to pin the vectorised forms."""
import math

import numpy as np

ADAM_DEFAULTS = dict(beta1=0.9, beta2=0.999, epsilon=1e-8, grad_scale=1.0, norm_scale=1.0, clip_sigma=0.0, saturate=0.0, zero_infs=False,
                     zero_nans=False)


def pre(g, zero_infs=False, zero_nans=False, saturate=0.0):
    """+-Inf -> 0, NaN -> 0, clamp to +-saturate, in this order (a NaN that is not zeroed meets fminf / fmaxf, which return the other
    operand: it becomes +saturate)."""
    g = np.array(g, dtype=np.float64)
    if zero_infs:
        g[np.isinf(g)] = 0.0
    if zero_nans:
        g[np.isnan(g)] = 0.0
    if saturate != 0.0:
        g = np.fmax(np.fmin(g, saturate), -saturate)
    return g


def _live(n, gate, bsize):
    """Per-element mask of the blocks that take part."""
    if gate is None:
        return np.ones(n, dtype=bool)
    return np.repeat(np.asarray(gate) != 0, bsize * bsize)


def adam(p, m, v, g, lr, gate=None, bsize=0, lr_select=None, lr_new=None, **kw):
    """One step; returns new (p, m, v) as flat float64 arrays.  Gated-off blocks and a norm_scale of 0 leave everything as it was."""
    o = dict(ADAM_DEFAULTS)
    o.update(kw)
    p, m, v = (np.array(a, dtype=np.float64).reshape(-1) for a in (p, m, v))
    if o["norm_scale"] == 0.0:
        return p, m, v
    g = pre(np.asarray(g).reshape(-1), o["zero_infs"], o["zero_nans"], o["saturate"])
    g = g * (np.float64(np.float32(o["grad_scale"])) * np.float64(np.float32(o["norm_scale"])))
    b1, b2, eps = (np.float64(np.float32(o[k])) for k in ("beta1", "beta2", "epsilon"))
    with np.errstate(invalid="ignore", over="ignore"):          # (planted Inf / NaN gradients that no flag zeroes)
        v2 = b2 * v + (1.0 - b2) * g * g
        sigma = np.sqrt(v2)
        if o["clip_sigma"] != 0.0:
            clip = np.float64(np.float32(o["clip_sigma"])) * sigma
            g = np.minimum(np.maximum(g, -clip), clip)
        m2 = b1 * m + (1.0 - b1) * g
        step = np.full(p.shape, np.float64(np.float32(lr)))
        if lr_select is not None:
            step[np.repeat(np.asarray(lr_select) != 0, bsize * bsize)] = np.float64(np.float32(lr_new))
        p2 = p - step * m2 / (sigma + eps)
    live = _live(p.size, gate, bsize)
    return np.where(live, p2, p), np.where(live, m2, m), np.where(live, v2, v)


def adam_loop(p, m, v, g, lr, gate=None, bsize=0, lr_select=None, lr_new=None, **kw):
    o = dict(ADAM_DEFAULTS)
    o.update(kw)
    f = lambda x: float(np.float32(x))
    p, m, v = ([float(x) for x in np.asarray(a).reshape(-1)] for a in (p, m, v))
    g = [float(x) for x in np.asarray(g).reshape(-1)]
    if o["norm_scale"] == 0.0:
        return np.array(p), np.array(m), np.array(v)
    bb = bsize * bsize
    for i in range(len(p)):
        if gate is not None and gate[i // bb] == 0:
            continue
        x = g[i]
        if o["zero_infs"] and math.isinf(x):
            x = 0.0
        if o["zero_nans"] and math.isnan(x):
            x = 0.0
        if o["saturate"] != 0.0:
            s = o["saturate"]
            x = s if math.isnan(x) else max(min(x, s), -s)
        x *= f(o["grad_scale"]) * f(o["norm_scale"])
        v[i] = f(o["beta2"]) * v[i] + (1.0 - f(o["beta2"])) * x * x
        sigma = math.sqrt(v[i])
        if o["clip_sigma"] != 0.0:
            c = f(o["clip_sigma"]) * sigma
            x = min(max(x, -c), c)
        m[i] = f(o["beta1"]) * m[i] + (1.0 - f(o["beta1"])) * x
        rate = f(lr_new) if lr_select is not None and lr_select[i // bb] != 0 else f(lr)
        p[i] -= rate * m[i] / (sigma + f(o["epsilon"]))
    return np.array(p), np.array(m), np.array(v)


def ema(e, p, decay, gate=None, bsize=0):
    """e - (1 - decay)(e - p), flat float64; (1 - decay) is the fp32 difference the host hands to the kernel."""
    e, p = (np.array(a, dtype=np.float64).reshape(-1) for a in (e, p))
    rate = np.float64(np.float32(1.0) - np.float32(decay))
    return np.where(_live(e.size, gate, bsize), e - rate * (e - p), e)


def ema_loop(e, p, decay, gate=None, bsize=0):
    e = [float(x) for x in np.asarray(e).reshape(-1)]
    p = [float(x) for x in np.asarray(p).reshape(-1)]
    rate = float(np.float32(1.0) - np.float32(decay))
    for i in range(len(e)):
        if gate is None or gate[i // (bsize * bsize)] != 0:
            e[i] = e[i] - rate * (e[i] - p[i])
    return np.array(e)


def sum_squared(x, grad_scale=1.0, saturate=0.0, zero_infs=False, zero_nans=False):
    s = pre(np.asarray(x).reshape(-1), zero_infs, zero_nans, saturate) * np.float64(np.float32(grad_scale))
    with np.errstate(over="ignore", invalid="ignore"):
        return float((s * s).sum())


def clip(sums, clip_norm):
    """(norm, scale) from the tensors' sums of squares."""
    total = float(np.sum(np.asarray(sums, dtype=np.float64)))
    norm = math.sqrt(total) if total == total and total >= 0 else float("nan")
    if not math.isfinite(norm):
        return norm, 0.0
    return norm, float(clip_norm) / max(norm, float(clip_norm))


def lr_correction_loop(t, beta1, beta2, zero_init_variables=False):
    """The reference's beta-power accumulators multiplied out call by call (blocksparse/optimize.py:45-57, 104-110): they start at beta --
    or at 0 with zero_init_variables, and 0 times beta stays 0."""
    p1, p2 = (0.0, 0.0) if zero_init_variables else (beta1, beta2)
    for _ in range(t - 1):
        p1, p2 = p1 * beta1, p2 * beta2
    return math.sqrt(1.0 - p2) / (1.0 - p1)


def gate_pattern(blocks, rng):
    """The suite's gate: blocks 0 and the last one off, block 4 on, the rest on with probability 0.6."""
    g = (rng.rand(blocks) < 0.6).astype(np.float32)
    g[0], g[4], g[blocks - 1] = 0.0, 1.0, 0.0
    return g
