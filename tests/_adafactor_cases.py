"""The named cases of the Adafactor tiers and the assertions both tiers make on them: tests/test_adafactor_gpu.py runs the kernels on
them, tests/test_adafactor_host.py the float32 model of tests/_adafactor_ref.py (and its mutant).  A case's host side -- inputs, gate and
the float64 state after every step -- is computed once and never written again.

Inputs are those of test_optimize_gpu._inputs: g ~ N(0, 0.1) rounded to the grad type with every 97th element x 50, p ~ N(0, 0.01),
slots uniform in [0, 1e-2) or zeros where the case says so; the 2-d cases have one row and one column of zero gradients."""
import functools

import numpy as np

import _adafactor_ref as AR
import _optimize_ref as OR
import _parity as P
from oracle import bsmm_oracle as orc

STEPS, BETA2, LR, NORM_SCALE, BLOCKS = 3, 0.999, 1e-3, 0.7, 37
SETTINGS = dict(grad_scale=0.5, saturate=2.0)
UPDATE_BAR = 1e-5            # L2 of p_new - p_old against float64: the Adam tests' bar
MOMENT_BAR = 2e-5            # rv, cv per element, relative: sums of non-negative terms, nothing cancels (the project's fp32 max bar)

# name -> (form, rows, cols / bsize, grad type, misalign, zero slots, gated)
# 2-d: the kernels' tiles are 32 rows x 1024 columns on the 16-byte path and 32 x 256 on the element path, so (33, 1028) and (33, 257) are
# the shapes one past both boundaries of either path; (300, 520) has 10 slabs but one chunk on the 16-byte path, three when misaligned.
CASES = {
    "2d-2x5": ("2d", 2, 5, "f32", 0, False, False),
    "2d-3x8": ("2d", 3, 8, "f16", 0, False, False),
    "2d-67x131-element": ("2d", 67, 131, "bf16", 0, False, False),
    "2d-67x136-zero-slots": ("2d", 67, 136, "f32", 0, True, False),
    "2d-300x520-clip": ("2d", 300, 520, "bf16", 0, False, False),
    "2d-300x520-misaligned": ("2d", 300, 520, "f32", 1, True, False),
    "2d-33x1028": ("2d", 33, 1028, "f32", 0, False, False),
    "2d-33x257": ("2d", 33, 257, "f16", 0, False, False),
    "2d-5x4104": ("2d", 5, 4104, "f32", 0, False, False),
    "2d-4099x3": ("2d", 4099, 3, "f16", 0, False, False),
    "1d-1": ("1d", 1, 1, "f32", 0, False, False),
    "1d-63-zero-slots": ("1d", 1, 63, "bf16", 0, True, False),
    "1d-4097": ("1d", 1, 4097, "f16", 0, False, False),
    "1d-4096": ("1d", 1, 4096, "f32", 0, False, False),
    "1d-4096-misaligned": ("1d", 1, 4096, "bf16", 1, False, False),
    "block-8": ("block", BLOCKS, 8, "f32", 0, False, True),
    "block-16": ("block", BLOCKS, 16, "f16", 0, False, True),
    "block-32": ("block", BLOCKS, 32, "bf16", 0, True, True),
    "block-64": ("block", BLOCKS, 64, "bf16", 0, False, True),
    "block-32-ungated": ("block", BLOCKS, 32, "f32", 0, False, False),
    "block-16-misaligned": ("block", BLOCKS, 16, "bf16", 1, True, True),
}
# Clip coverage, asserted on the float64 RMS of x: above clip_thresh = 1 in every step / below it in every step.  No block case stays
# below for three steps (per-block factoring puts the RMS near 1 and it rises as the moments decay towards the gradient's own
# mean), so for that form the case below is one whose FIRST step is not clipped.
CLIP_ACTIVE = ("2d-300x520-misaligned", "1d-63-zero-slots", "block-32")
CLIP_INACTIVE = ("2d-5x4104", "1d-4097")
CLIP_INACTIVE_FIRST_STEP = ("block-16",)


class Case(object):
    pass


def shape_of(c):
    return (c.rows, c.bs, c.bs) if c.form == "block" else ((c.cols,) if c.form == "1d" else (c.rows, c.cols))


def decay(t):
    from blocksparse_amd.optimize import adafactor_decay
    return adafactor_decay(t, BETA2)


def step_ref(c, fn_dense, fn_blocks, state, t, **extra):
    """One step of either restatement from ``state`` = (p, cv, rv); returns (p, cv, rv, rms)."""
    kw = dict(lr=LR, decay=decay(t), norm_scale=NORM_SCALE, **SETTINGS)
    kw.update(extra)
    if c.form == "block":
        return fn_blocks(state[0], state[1], state[2], c.g, c.rows, c.bs, gate=c.gate, **kw)
    return fn_dense(state[0], state[1], state[2], c.g, c.rows, c.cols, **kw)


@functools.lru_cache(maxsize=None)
def case(name):
    c = Case()
    c.name = name
    c.form, c.rows, second, c.gdt, c.misalign, c.zero_slots, gated = CASES[name]
    c.bs = second if c.form == "block" else 0
    c.cols = second * second if c.form == "block" else second
    seed = sum(ord(ch) for ch in name)
    rng = np.random.RandomState(seed)
    n = c.rows * c.cols
    g = rng.normal(0.0, 0.1, n).astype(np.float32)
    g[::97] *= 50.0
    if c.form == "2d":
        g = g.reshape(c.rows, c.cols)
        g[c.rows // 2, :] = 0.0
        g[:, c.cols // 3] = 0.0
        g = g.reshape(-1)
    c.g = orc.round_to(g, c.gdt).astype(np.float32)
    c.p = rng.normal(0.0, 0.01, n).astype(np.float32)
    ncv = c.rows * c.bs if c.bs else c.cols
    nrv = c.rows * c.bs if c.bs else (c.rows if c.form == "2d" else 0)
    slot = lambda k: (np.zeros(k) if c.zero_slots else rng.uniform(0.0, 1e-2, k)).astype(np.float32)
    c.cv, c.rv = slot(ncv), (slot(nrv) if nrv else None)
    c.gate = OR.gate_pattern(c.rows, np.random.RandomState(seed + 1)) if gated else None
    c.live = np.repeat(c.gate != 0, c.cols) if gated else np.ones(n, dtype=bool)
    c.live_slots = np.repeat(c.gate != 0, c.bs) if gated else np.ones(ncv, dtype=bool)
    state, c.rms = (c.p, c.cv, c.rv), []
    for t in range(1, STEPS + 1):
        out = step_ref(c, AR.dense, AR.blocks, state, t)
        state = out[:3]
        c.rms.append(out[3])
    c.ref_p, c.ref_cv, c.ref_rv = state
    for a in (c.g, c.p, c.cv, c.rv, c.gate, c.ref_p, c.ref_cv, c.ref_rv):
        if a is not None:
            a.setflags(write=False)
    return c


def model_steps(c, **extra):
    """STEPS steps of the float32 model on the access path the case's alignment selects."""
    state = (c.p, c.cv, c.rv)
    for t in range(1, STEPS + 1):
        state = step_ref(c, AR.model_dense, AR.model_blocks, state, t, vec=not c.misalign, **extra)[:3]
    return state


def figures(c, p, cv, rv):
    """The measured figures of one result (flat host arrays) against the case's float64 state."""
    live = c.live
    l2, mx = P.errors(np.asarray(p)[live], c.ref_p[live])
    upd, _ = P.errors(np.asarray(p, dtype=np.float64)[live] - c.p[live], c.ref_p[live] - c.p[live])
    mask = lambda ref: c.live_slots if c.bs else np.ones(ref.size, dtype=bool)
    rel = lambda got, ref: float(np.max(np.abs(np.asarray(got, dtype=np.float64)[mask(ref)] - ref[mask(ref)]) / ref[mask(ref)]))
    return {"param_l2": l2, "param_max": mx, "update_l2": upd, "cv_rel": rel(cv, c.ref_cv), "rv_rel": rel(rv, c.ref_rv) if rv is not None else 0.0}


def failures(fig):
    """The bars a result misses (an empty list: it passes)."""
    bars = {"param_l2": P.L2_BAR["f32"], "param_max": P.MAX_BAR["f32"], "update_l2": UPDATE_BAR, "cv_rel": MOMENT_BAR, "rv_rel": MOMENT_BAR}
    return [(k, fig[k], bars[k]) for k in sorted(bars) if not fig[k] <= bars[k]]


def check(c, p, cv, rv, what):
    fig = figures(c, p, cv, rv)
    print("adafactor %s %s: " % (what, c.name) + "  ".join("%s %.3e" % (k, fig[k]) for k in sorted(fig))
          + "  rms " + " ".join("%.3f" % r for r in c.rms))
    assert np.isfinite(np.asarray(p)).all() and np.isfinite(np.asarray(cv)).all()
    assert not failures(fig), (c.name, what, failures(fig))
    return fig
