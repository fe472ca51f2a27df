"""Simulated float formats: run a tensor as if it were stored with ``ebits`` exponent bits and ``fbits`` fraction bits, and the statistics
that tune such a format (saturation share, flush-to-zero share, max, mean and deviation).

The reference's names and arguments (blocksparse/quantize.py) over the C ABI of include/bsmm_quant.h:

    spec = QuantizeSpec(ebits=4, fbits=3, stochastic=2, frequency=1024)        # the reference's constructor + nearest_even, group
    y = quantize(x, spec, b_qspec=QuantizeSpec(5, 2), name="act0")             # forward rounds x, backward rounds dy (straight-through)
    y = log_stats(x, step, logfile="stats.txt", name="act0")                   # identity; logs on the powers of two, then every freq steps
    y = quantize_fwd(x, spec, emax=None | int | device int32 tensor)           # no autograd, no schedule
    quantize_update_emax(x, spec, emax_dev)                                    # statistics -> the device exponent, no host sync
    s = tensor_stats(x)                                                        # device float32 [8]

The package re-exports every name but the operator itself: ``blocksparse_amd.quantize`` stays this module, the operator is
``blocksparse_amd.quantize.quantize`` (``from blocksparse_amd.quantize import quantize``, as with the reference).

``x`` is fp32, or bf16 with ``fbits <= 7`` (the reference's storage types; the statistics also take fp16).  The rounding is defined to the
bit in include/bsmm_quant.h and ``quantize_test`` is that definition in NumPy integer arithmetic: nearest with ties away from zero (the
reference's default), nearest with ties to even (``nearest_even=True``, what the hardware formats do) or stochastic
(``stochastic`` 1 or 2: both mean the Philox stream of ``ewops.entropy_state``; every generating call enqueues ``offset += 1`` afterwards,
so a captured step draws fresh bits on every replay).  PyTorch is plumbing (memory, streams, autograd); there is no CPU fallback.

The top exponent comes from the spec (``emax=int``), from a device int32 (``emax=tensor``: a ``quantize_update_emax`` earlier on the same
stream may have written it) or, with ``group=32``, from every run of 32 consecutive elements (block-scaled: the shared power-of-two scale
of the MX formats when ``bias_pad=0``).

``quantize`` keeps the reference's schedule (src/quantize_op.cc:137-147): with ``frequency > 0`` the call collects statistics and updates
the exponent at intervals that start at 1 and double after every four collections until they reach ``frequency``.  The decision to collect
is HOST state (``QuantizeState``): a captured step replays the decision it was captured with.  A captured step that wants a live exponent
calls ``quantize_update_emax`` itself.  With a ``logfile`` the collecting call appends the reference's line (``quant_headers``); that costs
a sync, so it raises during capture.
"""
import ctypes
import math

import numpy as np

from . import _lib
from . import ewops

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

GROUP = _lib.QUANT_GROUP

quant_headers = ["sat_pct", "ftz_pct", "exp_max", "exp_min", "max", "mean", "stdv", "mean+stdv5", "max_stat_lo", "max_stat_hi", "count", "name"]
stat_headers = ["sat_pct", "ftz_pct", "max", "mean", "stdv", "mean+stdv5", "max_stat_lo", "max_stat_hi", "count", "name"]
_log_init = set()


class QuantizeSpec(object):
    """The reference's constructor (blocksparse/quantize.py:20-46) plus ``nearest_even`` and ``group``."""

    def __init__(self, ebits=4, fbits=3, emax=None, stochastic=0, denorm=True, frequency=1024, mode=0, bias_pad=2, stdv_mul=4.0, logfile="",
                 copy=None, nearest_even=False, group=0):
        if copy is not None:
            ebits, fbits, emax, stochastic, denorm, frequency = copy.ebits, copy.fbits, copy.emax, copy.stoch, copy.denorm, copy.freq
            mode, bias_pad, stdv_mul, logfile = copy.mode, copy.bias_pad, copy.stdv_mul, copy.logfile or logfile
            nearest_even, group = copy.nearest_even, copy.group
        if emax is None:
            emax = (1 << (ebits - 1)) - 1          # default symmetric
        self.ebits, self.fbits, self.emax, self.stoch, self.denorm = int(ebits), int(fbits), int(emax), int(stochastic), bool(denorm)
        self.freq, self.mode, self.bias_pad, self.stdv_mul, self.logfile = int(frequency), int(mode), int(bias_pad), float(stdv_mul), logfile
        self.nearest_even, self.group = bool(nearest_even), int(group)
        if not (1 <= self.ebits <= 8 and 0 <= self.fbits <= 23):
            raise ValueError("QuantizeSpec: 1 <= ebits <= 8 and 0 <= fbits <= 23, got (%d, %d)" % (self.ebits, self.fbits))
        if self.stoch not in (0, 1, 2) or self.mode not in (0, 1) or self.group not in (0, GROUP) or abs(self.bias_pad) > 256:
            raise ValueError("QuantizeSpec: stochastic in (0, 1, 2), mode in (0, 1), group in (0, %d), |bias_pad| <= 256" % GROUP)
        if self.stoch and self.nearest_even:
            raise ValueError("QuantizeSpec: stochastic and nearest_even exclude each other")

    @property
    def round_mode(self):
        return _lib.QUANT_STOCHASTIC if self.stoch else (_lib.QUANT_NEAREST_EVEN if self.nearest_even else _lib.QUANT_NEAREST_AWAY)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def _check_tensor(x, what, fp16_ok=False):
    if torch is None:
        raise RuntimeError("blocksparse_amd needs PyTorch-ROCm for device memory")
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise RuntimeError("blocksparse_amd: %s must be a tensor on a ROCm device (no CPU fallback)" % what)
    code = _lib.dtype_code(x.dtype)
    if code is None or (code == _lib.F16 and not fp16_ok):
        raise ValueError("quantize: %s must be float32 or bfloat16%s, got %s" % (what, " or float16" if fp16_ok else "", x.dtype))
    if x.numel() == 0 or x.numel() >= 2 ** 31:
        raise ValueError("quantize: %s must have between 1 and 2^31 - 1 elements, got shape %s" % (what, tuple(x.shape)))
    return code


def _check_spec(spec, code, numel):
    if not isinstance(spec, QuantizeSpec):
        raise TypeError("quantize: spec must be a QuantizeSpec")
    if code == _lib.BF16 and spec.fbits > 7:
        raise ValueError("quantize: bfloat16 only holds up to 7 fraction bits, got fbits = %d" % spec.fbits)
    if spec.group and numel % spec.group:
        raise ValueError("quantize: group = %d needs a multiple of %d elements, got %d" % (spec.group, spec.group, numel))


def _args(spec, code, device, emax=None, workspace=None):
    a = _lib.BsmmQuantArgs(ebits=spec.ebits, fbits=spec.fbits, emax=spec.emax if emax is None else int(emax), denorm=int(spec.denorm),
                           round_mode=spec.round_mode, group=spec.group, bias_pad=spec.bias_pad, stat_mode=spec.mode, dtype=code,
                           stdv_mul=spec.stdv_mul, workspace=None, workspace_bytes=0, stream=_lib.raw_stream(device))
    if workspace is not None:
        a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel() * 8
    return a


def _workspace(x):
    need = int(_lib.load().bsmm_quant_workspace_bytes(x.numel()))
    return torch.empty(need // 8, dtype=torch.float64, device=x.device)


def _check_emax_dev(t, x):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.numel() != 1 or t.device != x.device:
        raise ValueError("quantize: a device exponent must be an int32 tensor of one element on the device of x")
    return t


def emax_tensor(value, device=None):
    """A device exponent: int32 [1] holding ``value``."""
    return torch.tensor([int(value)], dtype=torch.int32, device="cuda" if device is None else device)


# ---- the low-level forms (no autograd) ------------------------------------------------------------------------------------------------
def quantize_fwd(x, spec, emax=None, out=None):
    """y = Q(x), like x (bsmm_quantize, one launch).  ``emax``: None (the spec's), an int, or a device int32 [1] tensor that the kernel
    reads.  ``out``: a contiguous tensor like x to write, ``x`` itself for in place.  A stochastic spec reads the device's {seed, offset}
    and advances the offset."""
    code = _check_tensor(x, "x")
    _check_spec(spec, code, x.numel())
    x = x.contiguous()
    if out is None:
        out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    elif not isinstance(out, torch.Tensor) or out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise ValueError("quantize_fwd: out must be a contiguous tensor with the shape, dtype and device of x")
    dev = _check_emax_dev(emax, x) if isinstance(emax, torch.Tensor) else None
    a = _args(spec, code, x.device, None if dev is not None else emax)
    st = ewops.entropy_state(x.device) if spec.stoch else None
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.load().bsmm_quantize(x.data_ptr(), out.data_ptr(), ptr(st), ptr(dev), x.numel(), ctypes.byref(a)), "bsmm_quantize")
    _lib.wrote(out)
    if st is not None:
        ewops._advance(st)
    return out


def quantize_update_emax(x, spec, emax_dev, stats_out=None):
    """Statistics of x at the format's current exponent, then ``emax_dev <- clamp(e(M) + bias_pad)`` on the device, M = max|x|
    (``spec.mode`` 0) or mean + stdv_mul * stdv (1); unchanged when M is 0 or nothing was finite.  No host sync.  Returns the float32 [8]
    statistics tensor (bsmm_quant_update_emax)."""
    code = _check_tensor(x, "x", fp16_ok=True)
    _check_spec(spec, code, 0)
    x = x.contiguous()
    _check_emax_dev(emax_dev, x)
    if stats_out is None:
        stats_out = torch.empty(8, dtype=torch.float32, device=x.device)
    ws = _workspace(x)
    a = _args(spec, code, x.device, workspace=ws)
    _lib.check(_lib.load().bsmm_quant_update_emax(x.data_ptr(), x.numel(), ctypes.byref(a), emax_dev.data_ptr(), stats_out.data_ptr()),
               "bsmm_quant_update_emax")
    _lib.wrote(emax_dev, stats_out)
    return stats_out


def tensor_stats(x, sat_val=65504.0, ftz_val=2.0 ** -24):
    """Device float32 [8]: mean|x|, stdv, max|x|, the share with |x| >= sat_val or non-finite, the share with x != 0 and |x| < ftz_val, the
    non-finite count, n, 0 (bsmm_tensor_stats)."""
    code = _check_tensor(x, "x", fp16_ok=True)
    x = x.contiguous()
    out = torch.empty(8, dtype=torch.float32, device=x.device)
    ws = _workspace(x)
    _lib.check(_lib.load().bsmm_tensor_stats(x.data_ptr(), x.numel(), code, float(sat_val), float(ftz_val), out.data_ptr(), ws.data_ptr(),
                                             ws.numel() * 8, _lib.raw_stream(x.device)), "bsmm_tensor_stats")
    _lib.wrote(out)
    return out


# ---- the schedule and its state ---------------------------------------------------------------------------------------------------------
class _Schedule(object):
    """The reference's counters (src/quantize_op.cc:60, 137-147, 187): count_, pow2_, pow2_count_; freq2 = 4."""

    def __init__(self):
        self.count, self.pow2, self.pow2_count = 1, 1, 0

    def step(self, frequency):
        """Does this call collect?  Advances the counters."""
        collect = bool(frequency) and (self.count & (self.pow2 - 1)) == 0
        if collect and (self.pow2 << 1) <= frequency:
            if self.pow2_count == 4:
                self.pow2 <<= 1
                self.pow2_count = 0
            self.pow2_count += 1
        self.count += 1
        return collect


class QuantizeState(object):
    """What one ``quantize`` site keeps: the two device exponents (forward, backward) and the host call counters of the schedule."""

    def __init__(self, qspec, b_qspec=None, device=None, name="quantize"):
        b_qspec = qspec if b_qspec is None else b_qspec
        self.name = name
        self.emax_f, self.emax_b = emax_tensor(qspec.emax, device), emax_tensor(b_qspec.emax, device)
        self.sched_f, self.sched_b = _Schedule(), _Schedule()
        self.max_stat = {"f": [float("inf"), 0.0], "b": [float("inf"), 0.0]}      # max_stat_lo, max_stat_hi of the log line


_states = {}


def reset_quantize_states():
    """Forget every state ``quantize`` found by name."""
    _states.clear()
    _log_state.clear()


def _state_for(x, qspec, b_qspec, name):
    key = (ewops._device_index(x.device), name)
    if key not in _states:
        _states[key] = QuantizeState(qspec, b_qspec, x.device, name)
    return _states[key]


def _exp_of(v):
    return (int(np.float32(v).view(np.int32)) >> 23 & 0xff) - 127


def _open_log(logfile, headers):
    if logfile not in _log_init:
        with open(logfile, "w") as log:
            log.write("\t".join(headers) + "\n")
        _log_init.add(logfile)


def _quantize_dir(x, spec, state, which):
    """One direction of ``quantize``: collect on the schedule, then round with the state's exponent."""
    emax_dev = state.emax_f if which == "f" else state.emax_b
    sched = state.sched_f if which == "f" else state.sched_b
    count = sched.count
    if sched.step(spec.freq):
        if spec.logfile and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("quantize: a logfile needs the statistics on the host (a sync): not inside a stream capture")
        stats = quantize_update_emax(x, spec, emax_dev)
        if spec.logfile:
            s, e_hi = stats.cpu().numpy(), int(emax_dev.cpu()[0])
            f = _format(spec.ebits, spec.fbits, e_hi, spec.denorm)
            lo_hi = state.max_stat[which]
            lo_hi[0], lo_hi[1] = min(lo_hi[0], float(s[2])), max(lo_hi[1], float(s[2]))
            _open_log(spec.logfile, quant_headers)
            with open(spec.logfile, "a") as log:
                log.write("%.3f\t%.3f\t%3d\t%3d\t%3d\t%3d\t%3d\t%3d\t%3d\t%3d\t%d\t%s\n" % (
                    100.0 * s[3], 100.0 * s[4], int(f[0]), int(f[1]), _exp_of(s[2]), _exp_of(s[0]), _exp_of(s[1]), _exp_of(s[0] + 5.0 * s[1]),
                    _exp_of(lo_hi[0]), _exp_of(lo_hi[1]), count, state.name))
    return quantize_fwd(x, spec, emax_dev)


_log_state = {}


def _log_steps(freq, bfreq):
    return [1 << p for p in range(int(round(math.log2(freq or bfreq))))] if (freq or bfreq) else []


def _log_stats_dir(x, step, sat_val, ftz_val, freq, first_steps, logfile, name, which):
    if not freq:
        return
    st = _log_state.setdefault((name, which), {"prev": -1, "lo": float("inf"), "hi": 0.0, "stats": None})
    if step == st["prev"]:
        return
    st["prev"] = step
    if not (step in first_steps if step < freq else (step & (freq - 1)) == 0):
        return
    st["stats"] = tensor_stats(x, sat_val, ftz_val)
    if logfile:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("log_stats: a logfile needs the statistics on the host (a sync): not inside a stream capture")
        s = st["stats"].cpu().numpy()
        st["lo"], st["hi"] = min(st["lo"], float(s[2])), max(st["hi"], float(s[2]))
        _open_log(logfile, stat_headers)
        with open(logfile, "a") as log:
            log.write("%.6f\t%.6f\t%3d\t%3d\t%3d\t%3d\t%3d\t%3d\t%d\t%s\n" % (
                100.0 * s[3], 100.0 * s[4], _exp_of(s[2]), _exp_of(s[0]), _exp_of(s[1]), _exp_of(s[0] + 5.0 * s[1]), _exp_of(st["lo"]),
                _exp_of(st["hi"]), step, name))


def last_logged_stats(name="log_stats", backward=False):
    """The device statistics tensor of the most recent logging step of ``log_stats(name=...)``, or None."""
    st = _log_state.get((name, "b" if backward else "f"))
    return None if st is None else st["stats"]


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
if torch is not None:
    class _Quantize(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, qspec, b_qspec, state):
            ctx.cfg = (b_qspec, state)
            return _quantize_dir(x, qspec, state, "f")

        @staticmethod
        def backward(ctx, dy):
            b_qspec, state = ctx.cfg
            return _quantize_dir(dy, b_qspec, state, "b"), None, None, None

    class _LogStats(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, step, cfg):
            ctx.cfg = (step, cfg)
            sat_val, ftz_val, freq, bfreq, first_steps, logfile, name = cfg
            _log_stats_dir(x, step, sat_val, ftz_val, freq, first_steps, logfile, name, "f")
            return x.view_as(x)

        @staticmethod
        def backward(ctx, dy):
            step, (sat_val, ftz_val, freq, bfreq, first_steps, logfile, name) = ctx.cfg
            _log_stats_dir(dy, step, sat_val, ftz_val, bfreq, first_steps, logfile, name, "b")
            return dy, None, None


def quantize(x, qspec, b_qspec=None, name=None, state=None):
    """y = Q(x) under ``qspec``; the backward is ``Q(dy)`` under ``b_qspec`` (default: qspec) with an exponent of its own.  ``state``: a
    ``QuantizeState``; without it the state is found in a per-device registry under ``name`` (default "quantize")."""
    b_qspec = qspec if b_qspec is None else b_qspec
    code = _check_tensor(x, "x")
    for spec in (qspec, b_qspec):
        _check_spec(spec, code, x.numel())
    if state is None:
        state = _state_for(x, qspec, b_qspec, "quantize" if name is None else name)
    return _Quantize.apply(x, qspec, b_qspec, state)


def log_stats(x, step, sat_val=65504.0, ftz_val=2.0 ** -24, freq=512, bfreq=512, logfile="", name=None):
    """The identity in both directions; collects ``tensor_stats`` of x (backward: of dy, with ``bfreq``) on the reference's steps -- the
    powers of two below ``freq``, then every ``freq``-th step -- and appends a line of ``stat_headers`` to ``logfile`` if one is given.
    ``step`` is a host integer."""
    for f in (freq, bfreq):
        if f and (f & (f - 1)):
            raise ValueError("log_stats: freq and bfreq must be 0 or powers of two")
    _check_tensor(x, "x", fp16_ok=True)
    cfg = (float(sat_val), float(ftz_val), int(freq), int(bfreq), _log_steps(freq, bfreq), logfile, name or "log_stats")
    return _LogStats.apply(x, int(step), cfg)


# ---- the NumPy definitions ------------------------------------------------------------------------------------------------------------
def _format(ebits, fbits, emax, denorm):
    """(e_hi, s_min, e_lo, max_bits) of include/bsmm_quant.h; ``emax`` may be an array."""
    emax = np.asarray(emax, dtype=np.int64)
    nexp = 254 if ebits == 8 else (1 << ebits) - 1
    e_hi = np.clip(emax, nexp - 127, 127)
    sub = fbits if denorm else 0
    s_min = np.maximum(e_hi - nexp + 1 - sub, -125)
    max_bits = ((e_hi + 127) << 23) | (0x7fffff & ~((1 << (23 - fbits)) - 1))
    return e_hi, s_min, s_min + sub, max_bits


def random_words(n, seed, offset):
    """uint32 [n]: element i's random word, word i % 4 of Philox4x32-10(counter = (i / 4, 0, offset), key = seed)."""
    n, seed, offset = int(n), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    calls = np.arange((n + 3) // 4, dtype=np.uint64)
    w = ewops.philox4x32_10((calls, 0, offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=1).reshape(-1)[:n]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.int64)


def _round_bits(bits, spec, emax, r=None):
    """Q on int64 arrays of fp32 bit patterns; ``emax``: scalar or array like bits."""
    fbits, mode = spec.fbits, spec.round_mode
    _, _, e_lo, max_bits = _format(spec.ebits, fbits, emax, spec.denorm)
    e_lo, max_bits = np.broadcast_to(e_lo, bits.shape), np.broadcast_to(max_bits, bits.shape)
    sign, a = bits & 0x80000000, bits & 0x7fffffff
    ef = a >> 23
    M = np.where(ef != 0, (a & 0x7fffff) | 0x800000, a)
    e = ef - 127
    ev = np.where(ef != 0, e, -126)
    E = np.maximum(e, e_lo)
    sh = 23 - fbits + (E - ev)
    shc = np.minimum(sh, 25)
    lo, rem = M >> shc, M & ((np.int64(1) << shc) - 1)
    twice, full = rem << 1, np.int64(1) << shc
    if mode == _lib.QUANT_NEAREST_AWAY:
        up = twice >= full
    elif mode == _lib.QUANT_NEAREST_EVEN:
        up = (twice > full) | ((twice == full) & ((lo & 1) == 1))
    else:
        thr = (rem << 32) >> np.minimum(sh, 62)               # floor(frac * 2^32); rem < 2^24: zero from sh = 56 on
        up = np.asarray(r, dtype=np.int64).reshape(bits.shape) < thr
    q = lo + up
    if not spec.denorm:
        q = np.where(q < (1 << fbits), 0, q)
    qs = np.maximum(q, 1)
    p = np.zeros(bits.shape, dtype=np.int64)                  # the position of q's top bit
    for k in (16, 8, 4, 2, 1):
        big = (qs >> (p + k)) != 0
        p = np.where(big, p + k, p)
    mag = ((E - fbits + p + 126) << 23) + (((qs << (31 - p)) & 0xffffffff) >> 8)
    mag = np.where(q == 0, 0, np.minimum(mag, max_bits))
    out = np.where(a >= max_bits, sign | max_bits, sign | mag)
    return np.where(a > 0x7f800000, bits, out)


def group_emax_test(x, spec, emax=None):
    """int64 [n / 32]: the top exponent (before the clamp) the block-scaled mode gives every run of 32 elements."""
    a = (_bits(x) & 0x7fffffff).reshape(-1, GROUP)
    amax = np.where(a < 0x7f800000, a, 0).max(axis=1)
    base = spec.emax if emax is None else int(emax)
    return np.where(amax != 0, (amax >> 23) - 127 + spec.bias_pad, base)


def quantize_test(x, spec, emax=None, seed=0, offset=0):
    """Q(x) as float32, like x: the definition of include/bsmm_quant.h in integer arithmetic on the fp32 bit patterns.  ``x``: float32
    values (a bf16 tensor: its upcast).  ``emax``: None = the spec's."""
    x = np.asarray(x, dtype=np.float32)
    bits = _bits(x).reshape(-1)
    em = spec.emax if emax is None else int(emax)
    if spec.group:
        if bits.size % GROUP:
            raise ValueError("quantize_test: group = %d needs a multiple of %d elements" % (GROUP, GROUP))
        em = np.repeat(group_emax_test(x, spec, emax), GROUP)
    r = random_words(bits.size, seed, offset) if spec.stoch else None
    return _round_bits(bits, spec, em, r).astype(np.uint32).view(np.float32).reshape(x.shape)


def tensor_stats_test(x, sat_val=65504.0, ftz_val=2.0 ** -24):
    """float64 [8]: the statistics of include/bsmm_quant.h."""
    v = np.abs(np.asarray(x, dtype=np.float64).reshape(-1))
    n, finite = v.size, np.isfinite(v)
    f = np.where(finite, v, 0.0)
    mean = f.sum() / n
    stdv = math.sqrt(max((f * f).sum() / n - mean * mean, 0.0))
    sat = ((f >= sat_val) | ~finite).sum()
    ftz = (finite & (f != 0) & (f < ftz_val)).sum()
    return np.array([mean, stdv, f.max(), sat / n, ftz / n, (~finite).sum(), n, 0.0])


def quantize_emax_test(x, spec, emax):
    """The exponent ``quantize_update_emax`` leaves on the device, from the float64 statistics."""
    s = tensor_stats_test(x)
    M = np.float32(s[0] + spec.stdv_mul * s[1] if spec.mode else s[2])
    if not (M > 0) or s[5] == s[6]:
        return int(emax)
    e = _exp_of(min(M, np.float32(np.inf)))
    return int(_format(spec.ebits, spec.fbits, e + spec.bias_pad, spec.denorm)[0])


def quantize_schedule_test(frequency, calls):
    """The 1-based numbers of the calls among the first ``calls`` that collect statistics."""
    s = _Schedule()
    return [i for i in range(1, int(calls) + 1) if s.step(int(frequency))]
