"""The epilogue of a block-sparse layer: bias + ReLU / fast-GELU, a counter-based dropout with a 1-bit mask, and both as one launch each way,
in both activation layouts of the matmul.

The reference's names and arguments (blocksparse/ewops.py:300-420) over the C ABI of include/bsmm_ew.h:

    y = bias_relu(x, b, axis=0, relu=True)                       # x (C, N): the layout of feature_axis=0 matmuls
    y = bias_relu(x, b, fast_gelu=True)                          # x (..., C): z * sigmoid(1.702 z)
    y, mask = dropout(x, keep_prob=0.9)                          # mask: int32 [ceil(numel / 32)], 1 bit per element
    y, _ = dropout(x, keep_prob=0.9, mask=mask)                  # the recomputed forward reuses it
    y, mask = bias_dropout(x, b, 0.9, axis=0, fast_gelu=True, residual=r)     # bias -> activation -> dropout -> + residual, one launch

``x`` is fp32, fp16 or bf16 of any rank: ``axis=0`` takes the leading dimension as the features (the others are flattened into N),
``axis=-1`` or ``rank - 1`` the last one.  ``b`` is fp32 with K elements in any shape; its gradient is fp32 in every dtype and is summed
without floating-point read-modify-write: the same inputs give the same bits.  All arithmetic is fp32, every result is rounded once.
PyTorch is plumbing (memory, streams, autograd); there is no CPU fallback.

The dropout mask is a pure function of (seed, offset, keep_prob, numel) -- ``dropout_mask_test`` is its NumPy definition -- and does not
depend on the dtype, the layout or the launch.  ``seed`` and ``offset`` live on the device, one int64 [2] tensor per device
(``entropy_state``), set by ``set_entropy``: every call that generates a mask reads the tensor as it stands and then enqueues
``offset += 1`` on the current stream, so a captured training step draws a fresh mask on every replay.

``bias_relu_test`` / ``bias_relu_grad_test`` / ``dropout_mask_test`` / ``bias_dropout_test`` / ``bias_dropout_grad_test`` are the NumPy
definitions (the reference has none for these operators; its tests compare against TensorFlow's CPU ops).
"""
import ctypes

import numpy as np

from . import _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

FAST_GELU_ALPHA = 1.702


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def _act_code(relu, fast_gelu):
    if relu and fast_gelu:
        raise ValueError("bias_relu: relu and fast_gelu exclude each other")
    return _lib.ACT_RELU if relu else (_lib.ACT_FAST_GELU if fast_gelu else _lib.ACT_NONE)


def _keep(keep_prob):
    """(threshold, scale) of a keep probability in (0, 1]."""
    keep_prob = float(keep_prob)
    if not (0.0 < keep_prob <= 1.0):
        raise ValueError("dropout: keep_prob must lie in (0, 1], got %r" % (keep_prob,))
    return int(round(keep_prob * 65536.0)), float(np.float32(1.0 / keep_prob))


def _dtype_code(x, what):
    if torch is None:
        raise RuntimeError("blocksparse_amd needs PyTorch-ROCm for device memory")
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise RuntimeError("blocksparse_amd: %s must be a tensor on a ROCm device (no CPU fallback)" % what)
    code = _lib.dtype_code(x.dtype)
    if code is None:
        raise ValueError("ewops: %s must be float32, float16 or bfloat16, got %s" % (what, x.dtype))
    if x.numel() == 0 or x.numel() >= 2 ** 31:
        raise ValueError("ewops: %s must have between 1 and 2^31 - 1 elements, got shape %s" % (what, tuple(x.shape)))
    return code


def _problem(x, b, axis):
    """Validate and return (axis as 0 / 1, K, N, dtype code); the axis is resolved as norms._problem resolves it.  Raises before any launch."""
    code = _dtype_code(x, "x")
    if x.dim() < 1:
        raise ValueError("ewops: x must have at least one dimension")
    axis = int(axis)
    if axis < 0:
        axis += x.dim()
    if axis != 0 and axis != x.dim() - 1:
        raise ValueError("ewops: axis must be 0 or the last dimension of x (rank %d), got %d" % (x.dim(), axis))
    K = int(x.shape[axis])
    if b is not None:
        if not isinstance(b, torch.Tensor) or b.device.type != "cuda":
            raise RuntimeError("blocksparse_amd: b must be a tensor on a ROCm device (no CPU fallback)")
        if b.dtype != torch.float32 or b.numel() != K or b.device != x.device:
            raise ValueError("ewops: b must be a float32 tensor with %d elements on the device of x" % K)
    return (0 if axis == 0 else 1), K, x.numel() // K, code


def _like(t, x, what):
    if not isinstance(t, torch.Tensor) or t.shape != x.shape or t.dtype != x.dtype or t.device != x.device:
        raise ValueError("ewops: %s must have the shape, dtype and device of x" % what)
    return t.contiguous()


def _mask_words(n):
    return (int(n) + 31) // 32


def _check_mask(mask, x):
    if not isinstance(mask, torch.Tensor) or mask.dtype != torch.int32 or mask.numel() != _mask_words(x.numel()) or mask.device != x.device:
        raise ValueError("dropout: mask must be an int32 tensor of ceil(numel / 32) = %d words on the device of x" % _mask_words(x.numel()))
    return mask.contiguous()


def _args(device, ax, K, N, code, act=0, generate=0, threshold=0, scale=1.0, which=_lib.EW_BIAS_ACT):
    """The argument struct and the workspace tensor it points into (torch's allocator, per call)."""
    a = _lib.BsmmEwArgs(K=K, N=N, axis=ax, dtype=code, act=act, generate=generate, threshold=threshold, scale=scale, workspace=None,
                        workspace_bytes=0, stream=_lib.raw_stream(device))
    need = int(_lib.load().bsmm_ew_workspace_bytes(ctypes.byref(a), which))
    ws = None
    if need:
        ws = torch.empty(need // 4, dtype=torch.float32, device=device)
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
    return a, ws


# ---- the stream state -----------------------------------------------------------------------------------------------------------------
_entropy = {}


def _device_index(device):
    if device is None:
        return torch.cuda.current_device()
    device = torch.device(device)
    return torch.cuda.current_device() if device.index is None else device.index


def entropy_state(device=None):
    """The int64 [2] tensor {seed, offset} of ``device`` that every generating call reads; created from ``torch.initial_seed()`` at first
    use.  Create it (or call ``set_entropy``) before a stream capture begins."""
    if torch is None:
        raise RuntimeError("blocksparse_amd needs PyTorch-ROCm for device memory")
    idx = _device_index(device)
    if idx not in _entropy:
        seed = int(torch.initial_seed()) & (2 ** 63 - 1)
        _entropy[idx] = torch.tensor([seed, 0], dtype=torch.int64, device="cuda:%d" % idx)
    return _entropy[idx]


def set_entropy(seed, device=None, offset=0):
    """Restart the dropout stream of ``device``: {seed, offset} (seed taken modulo 2^64).  Written in place, so a captured graph that reads
    the state follows it."""
    as_i64 = lambda v: ((int(v) & (2 ** 64 - 1)) ^ (1 << 63)) - (1 << 63)
    st = entropy_state(device)
    st.copy_(torch.tensor([as_i64(seed), as_i64(offset)], dtype=torch.int64))
    return st


def _advance(st):
    st[1:].add_(1)            # ordinary device work on the current stream: a replayed capture advances the offset as well


# ---- the low-level forms (no autograd) ------------------------------------------------------------------------------------------------
def bias_relu_fwd(x, b, axis=-1, relu=False, fast_gelu=False):
    """y = act(x + b), like x (bsmm_bias_act)."""
    act = _act_code(relu, fast_gelu)
    ax, K, N, code = _problem(x, b, axis)
    x, b = x.contiguous(), b.contiguous()
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    a, ws = _args(x.device, ax, K, N, code, act)
    _lib.check(_lib.load().bsmm_bias_act(x.data_ptr(), b.data_ptr(), y.data_ptr(), ctypes.byref(a)), "bsmm_bias_act")
    _lib.wrote(y)
    return y


def bias_relu_bwd(dy, x_or_y, b, axis=-1, relu=False, fast_gelu=False, need_dx=True):
    """(dx, db) of ``bias_relu_fwd``: ``x_or_y`` is the stored y for ReLU, x for fast-GELU and unused (may be None) for the plain bias,
    where dx is dy itself (returned as it came) and only db is computed.  db is fp32 in the shape of b (bsmm_bias_act_grad)."""
    act = _act_code(relu, fast_gelu)
    ax, K, N, code = _problem(dy, b, axis)
    dy, b = dy.contiguous(), b.contiguous()
    db = torch.empty(b.shape, dtype=torch.float32, device=dy.device)
    a, ws = _args(dy.device, ax, K, N, code, act, which=_lib.EW_BIAS_ACT_GRAD)
    if act == _lib.ACT_NONE:
        dx, xy_ptr, dx_ptr = dy, None, None
    else:
        xy = _like(x_or_y, dy, "x_or_y")
        dx = torch.empty(dy.shape, dtype=dy.dtype, device=dy.device)
        xy_ptr, dx_ptr = xy.data_ptr(), dx.data_ptr()
    _lib.check(_lib.load().bsmm_bias_act_grad(dy.data_ptr(), xy_ptr, b.data_ptr(), dx_ptr, db.data_ptr(), ctypes.byref(a)), "bsmm_bias_act_grad")
    _lib.wrote(db, None if dx is dy else dx)
    return dx, db


def dropout_mask(numel, keep_prob, device=None):
    """A fresh mask for ``numel`` elements: int32 [ceil(numel / 32)] from the device's {seed, offset}; advances the offset
    (bsmm_dropout_mask)."""
    threshold, _ = _keep(keep_prob)
    numel = int(numel)
    if not (1 <= numel < 2 ** 31):
        raise ValueError("dropout_mask: numel must lie in 1 .. 2^31 - 1, got %d" % numel)
    st = entropy_state(device)
    mask = torch.empty(_mask_words(numel), dtype=torch.int32, device=st.device)
    _lib.check(_lib.load().bsmm_dropout_mask(mask.data_ptr(), st.data_ptr(), numel, threshold, _lib.raw_stream(st.device)), "bsmm_dropout_mask")
    _lib.wrote(mask)
    _advance(st)
    return mask


def apply_dropout_mask(x, mask, keep_prob):
    """y = kept ? x / keep_prob : 0, like x; the forward and the backward of a dropout (bsmm_dropout_apply)."""
    _, scale = _keep(keep_prob)
    code = _dtype_code(x, "x")
    x, mask = x.contiguous(), _check_mask(mask, x)
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _lib.check(_lib.load().bsmm_dropout_apply(x.data_ptr(), mask.data_ptr(), y.data_ptr(), x.numel(), scale, code, _lib.raw_stream(x.device)),
               "bsmm_dropout_apply")
    _lib.wrote(y)
    return y


def bias_dropout_fwd(x, b, keep_prob, axis=-1, relu=False, fast_gelu=False, residual=None, mask=None):
    """(y, mask) of the fused forward: y = dropout(act(x + b)) [+ residual].  ``mask=None``: the launch makes the bits from the device's
    {seed, offset}, writes the mask and the offset advances; a given mask is read instead (the recompute path).  ``b=None`` (no activation):
    a plain dropout in one launch (bsmm_bias_act_dropout)."""
    act = _act_code(relu, fast_gelu)
    threshold, scale = _keep(keep_prob)
    ax, K, N, code = _problem(x, b, axis)
    if b is None and act != _lib.ACT_NONE:
        raise ValueError("bias_dropout_fwd: an activation needs a bias")
    x = x.contiguous()
    b = None if b is None else b.contiguous()
    residual = None if residual is None else _like(residual, x, "residual")
    generate = mask is None
    st = entropy_state(x.device) if generate else None
    mask = torch.empty(_mask_words(x.numel()), dtype=torch.int32, device=x.device) if generate else _check_mask(mask, x)
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    a, ws = _args(x.device, ax, K, N, code, act, 1 if generate else 0, threshold, scale, _lib.EW_BIAS_ACT_DROPOUT)
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.load().bsmm_bias_act_dropout(x.data_ptr(), ptr(b), ptr(residual), ptr(st), mask.data_ptr(), y.data_ptr(), ctypes.byref(a)),
               "bsmm_bias_act_dropout")
    _lib.wrote(y, mask if generate else None)
    if generate:
        _advance(st)
    return y, mask


def bias_dropout_bwd(dy, x, b, mask, keep_prob, axis=-1, relu=False, fast_gelu=False):
    """(dx, db) of the fused forward; the gradient of the residual is dy itself (bsmm_bias_act_dropout_grad)."""
    act = _act_code(relu, fast_gelu)
    threshold, scale = _keep(keep_prob)
    ax, K, N, code = _problem(x, b, axis)
    dy, x, b, mask = _like(dy, x, "dy"), x.contiguous(), b.contiguous(), _check_mask(mask, x)
    dx = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    db = torch.empty(b.shape, dtype=torch.float32, device=x.device)
    a, ws = _args(x.device, ax, K, N, code, act, 0, threshold, scale, _lib.EW_BIAS_ACT_DROPOUT_GRAD)
    _lib.check(_lib.load().bsmm_bias_act_dropout_grad(dy.data_ptr(), x.data_ptr(), b.data_ptr(), mask.data_ptr(), dx.data_ptr(), db.data_ptr(),
                                                      ctypes.byref(a)), "bsmm_bias_act_dropout_grad")
    _lib.wrote(dx, db)
    return dx, db


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
if torch is not None:
    class _BiasRelu(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, b, axis, relu, fast_gelu):
            y = bias_relu_fwd(x, b, axis, relu, fast_gelu)
            ctx.cfg = (axis, relu, fast_gelu)
            if relu:                                     # y for ReLU (x can be freed), x for fast-GELU, nothing for the plain bias
                ctx.save_for_backward(b, y)
            elif fast_gelu:
                ctx.save_for_backward(b, x)
            else:
                ctx.save_for_backward(b)
            return y

        @staticmethod
        def backward(ctx, dy):
            axis, relu, fast_gelu = ctx.cfg
            b = ctx.saved_tensors[0]
            kept = ctx.saved_tensors[1] if len(ctx.saved_tensors) > 1 else None
            dx, db = bias_relu_bwd(dy.to(kept.dtype) if kept is not None else dy, kept, b, axis, relu, fast_gelu)
            return dx, db, None, None, None

    class _Dropout(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, keep_prob, mask):
            if mask is None:
                y, mask = bias_dropout_fwd(x, None, keep_prob, axis=0)
            else:
                y = apply_dropout_mask(x, mask, keep_prob)
            ctx.save_for_backward(mask)
            ctx.keep_prob = keep_prob
            ctx.mark_non_differentiable(mask)
            return y, mask

        @staticmethod
        def backward(ctx, dy, _dmask):
            (mask,) = ctx.saved_tensors
            return apply_dropout_mask(dy, mask, ctx.keep_prob), None, None

    class _BiasDropout(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, b, residual, keep_prob, axis, relu, fast_gelu, mask):
            y, mask = bias_dropout_fwd(x, b, keep_prob, axis, relu, fast_gelu, residual, mask)
            ctx.save_for_backward(x, b, mask)
            ctx.cfg = (keep_prob, axis, relu, fast_gelu, residual is not None)
            ctx.mark_non_differentiable(mask)
            return y, mask

        @staticmethod
        def backward(ctx, dy, _dmask):
            x, b, mask = ctx.saved_tensors
            keep_prob, axis, relu, fast_gelu, has_residual = ctx.cfg
            dy = dy.to(x.dtype)
            dx, db = bias_dropout_bwd(dy, x, b, mask, keep_prob, axis, relu, fast_gelu)
            return dx, db, (dy if has_residual else None), None, None, None, None, None


def bias_relu(x, b, axis=-1, relu=False, fast_gelu=False, atomics=True):
    """y = x + b along ``axis``, then ReLU or fast-GELU if asked; differentiable in x and b.  ``atomics`` is accepted for the reference's
    signature and ignored: the bias gradient is always summed in a fixed order, without atomics."""
    _act_code(relu, fast_gelu)
    _problem(x, b, axis)
    return _BiasRelu.apply(x, b, int(axis), bool(relu), bool(fast_gelu))


def fast_gelu(x):
    """x * sigmoid(1.702 x); differentiable (the fused bias + fast-GELU with a zero bias)."""
    _dtype_code(x, "x")
    flat = x.reshape(1, -1)
    return bias_relu(flat, torch.zeros(1, dtype=torch.float32, device=x.device), axis=0, fast_gelu=True).reshape(x.shape)


def dropout(x, keep_prob, mask=None, mask_shape=None):
    """(y, mask): y = kept ? x / keep_prob : 0.  ``mask=None`` draws a fresh mask (int32, ceil(numel / 32) words, 1 bit per element), a given
    mask is applied as it is; the backward applies the same mask to dy.  Broadcast masks (``mask_shape``) are not implemented."""
    if mask_shape is not None:
        raise NotImplementedError("dropout: broadcast masks (mask_shape) are not implemented")
    _keep(keep_prob)
    _dtype_code(x, "x")
    if mask is not None:
        _check_mask(mask, x)
    return _Dropout.apply(x, float(keep_prob), mask)


def bias_dropout(x, b, keep_prob, axis=-1, relu=False, fast_gelu=False, residual=None, mask=None):
    """(y, mask): y = dropout(act(x + b)) [+ residual] as one launch, and one launch for the gradients of x and b; the gradient of
    ``residual`` is dy.  ``mask`` as in ``dropout``."""
    _act_code(relu, fast_gelu)
    _keep(keep_prob)
    _problem(x, b, axis)
    if b is None:
        raise ValueError("bias_dropout: b is required (dropout() is the form without a bias)")
    return _BiasDropout.apply(x, b, residual, float(keep_prob), int(axis), bool(relu), bool(fast_gelu), mask)


# ---- the NumPy definitions ------------------------------------------------------------------------------------------------------------
_PHILOX_M0, _PHILOX_M1, _PHILOX_W0, _PHILOX_W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 over arrays: counter = four uint32 arrays (or scalars), key = two; returns four uint32 arrays."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & 0xFFFFFFFF for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (int(v) & 0xFFFFFFFF for v in key)
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(_PHILOX_M0) * c[0], np.uint64(_PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + _PHILOX_W0) & 0xFFFFFFFF, (k1 + _PHILOX_W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def _keep_bits(n, seed, offset, threshold):
    """bool [n]: element i is kept."""
    n, seed, offset = int(n), int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1)
    calls = np.arange((n + 7) // 8, dtype=np.uint64)
    w = philox4x32_10((calls & 0xFFFFFFFF, calls >> np.uint64(32), offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    r = np.empty((calls.size, 8), dtype=np.uint32)
    for j in range(4):
        r[:, 2 * j] = w[j] & np.uint32(0xFFFF)
        r[:, 2 * j + 1] = w[j] >> np.uint32(16)
    return (r.reshape(-1)[:n] < np.uint32(threshold)) if threshold < 65536 else np.ones(n, dtype=bool)


def _pack(bits):
    n = bits.size
    padded = np.zeros(_mask_words(n) * 32, dtype=np.uint8)
    padded[:n] = bits
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32).view(np.int32)


def unpack_mask(mask, n):
    """bool [n] from the packed words."""
    words = np.ascontiguousarray(np.asarray(mask).reshape(-1)).view(np.uint32).astype("<u4")
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:int(n)].astype(bool)


def dropout_mask_test(n, seed, offset, keep_prob):
    """The mask of ``n`` elements as int32 [ceil(n / 32)]: the definition in include/bsmm_ew.h, in NumPy."""
    threshold, _ = _keep(keep_prob)
    return _pack(_keep_bits(n, seed, offset, threshold))


def _bias_shape(x, axis):
    axis = axis + x.ndim if axis < 0 else axis
    return tuple(x.shape[d] if d == axis else 1 for d in range(x.ndim))


def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-FAST_GELU_ALPHA * z))


def bias_relu_test(x, b, axis=-1, relu=False, fast_gelu=False):
    x = np.asarray(x)
    z = x + np.asarray(b).reshape(_bias_shape(x, axis))
    y = np.maximum(z, 0.0) if relu else (z * _sigmoid(z) if fast_gelu else z)
    return y.astype(x.dtype, copy=False)


def bias_relu_grad_test(dy, x, b, axis=-1, relu=False, fast_gelu=False):
    """(dx, db) from x (not from the stored y: for ReLU both give the same mask)."""
    dy, x, b = np.asarray(dy), np.asarray(x), np.asarray(b)
    z = x + b.reshape(_bias_shape(x, axis))
    if relu:
        dx = dy * (z > 0.0)
    elif fast_gelu:
        s = _sigmoid(z)
        dx = dy * (s + FAST_GELU_ALPHA * z * s * (1.0 - s))
    else:
        dx = dy
    ax = axis + x.ndim if axis < 0 else axis
    db = dx.sum(axis=tuple(d for d in range(x.ndim) if d != ax))
    return dx.astype(dy.dtype, copy=False), db.astype(b.dtype, copy=False).reshape(b.shape)


def bias_dropout_test(x, b, mask, keep_prob, axis=-1, relu=False, fast_gelu=False, residual=None):
    x = np.asarray(x)
    _, scale = _keep(keep_prob)
    kept = unpack_mask(mask, x.size).reshape(x.shape)
    y = np.where(kept, bias_relu_test(x, b, axis, relu, fast_gelu) * x.dtype.type(scale), x.dtype.type(0))
    if residual is not None:
        y = y + np.asarray(residual)
    return y.astype(x.dtype, copy=False)


def bias_dropout_grad_test(dy, x, b, mask, keep_prob, axis=-1, relu=False, fast_gelu=False):
    dy = np.asarray(dy)
    _, scale = _keep(keep_prob)
    kept = unpack_mask(mask, dy.size).reshape(dy.shape)
    g = np.where(kept, dy * dy.dtype.type(scale), dy.dtype.type(0))
    return bias_relu_grad_test(g, x, b, axis, relu, fast_gelu)
