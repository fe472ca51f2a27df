"""Fused row selection: activation sparsity along the last axis of a tensor, one launch each way.

The reference's names and arguments (blocksparse/transformer.py:494-656, blocksparse/lstm.py:103-117) over the C ABI of include/bsmm_select.h:

    y = rectified_top_k(x, k, rebase=True)                # the k largest of a row, less max(k-th value, 0); 0 elsewhere
    y = masked_top_k_softmax(x, k, mask=None, scale=1.0)  # the softmax over the k largest scores (x * mask) * scale; 0 elsewhere
    y = masked_softmax(x, mask=None, scale=1.0)           # k = K
    y = softmax(x, scale=1.0)
    y = sparse_relu(x, alpha=1.0)                         # max(x - (mean + alpha * sigma), 0), mean and sigma of the row

``x`` is a contiguous fp32, fp16 or bf16 tensor of any rank >= 1 on a ROCm device; rows run along the last axis (K = ``x.shape[-1]`` up to
4096, R = ``numel / K``).  ``mask`` is fp32 -- a float that multiplies, 0 marks a masked element -- with the rank of ``x``; every dimension
equals ``x``'s or is 1 and the 1s form a leading run: ``(1, 1, 1, K)``, ``(1, 1, T, K)`` and ``(1, H, T, K)`` for ``(B, H, T, K)``.

ONE total order decides every selection: value descending, then index ascending; -0.0 counts as +0.0, a NaN ranks above +inf (the rule of
``torch.topk``), masked elements rank below every unmasked one, by index among themselves.  The result is a function of the arguments only:
same arguments, same bits, also on ties (``torch.topk`` + ``scatter`` + ``softmax`` leave ties to the launch).  All arithmetic is fp32,
every stored value is rounded once.  A row without an unmasked element gives zeros (the reference would give 1 / k).  The gradients:
``dx = dz * (y > 0)`` for ``rectified_top_k`` and ``sparse_relu`` (the base and the cutoff count as constants, as in the reference),
``dx = (dy - sum(dy * y)) * y * mask * scale`` from the stored y for the three softmaxes.  PyTorch is plumbing (memory, streams, autograd);
there is no CPU fallback.

``select_path(K, dtype, aligned)`` names the kernel path a call takes.  The ``*_test`` / ``*_grad_test`` functions are the NumPy definitions.

Not here: a sorted ``top_k`` that returns values and indices (``torch.topk`` covers it; it is the only op of the family that needs a
sort), ``transpose_2d`` and ``transpose_0213`` (torch views).
"""
import ctypes

import numpy as np

from . import _lib
from . import ewops

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

MAX_K = _lib.SELECT_MAX_K
_CODES = {"f32": _lib.F32, "f16": _lib.F16, "bf16": _lib.BF16}


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def select_path(K, dtype, aligned=True):
    """The kernel path for rows of K elements: "wave8", "wave16" (a wave per row, 8 / 16 elements per lane), "group2", "group4" (a workgroup
    of two / four waves per row), with "-wide" when 16-byte accesses run: ``aligned`` (every pointer 16-byte aligned) and K a multiple of
    8 (4 in fp32).  ``dtype``: a torch dtype or "f32" / "f16" / "bf16" (bsmm_select_path)."""
    code = _CODES.get(dtype) if isinstance(dtype, str) else _lib.dtype_code(dtype)
    if code is None:
        raise ValueError("select_path: dtype must be float32, float16 or bfloat16, got %s" % (dtype,))
    rc = _lib.load().bsmm_select_path(int(K), code, 1 if aligned else 0)
    if rc < 0:
        raise ValueError("select_path: K must lie in 1 .. %d, got %d" % (MAX_K, K))
    return _lib.SELECT_PATHS[rc]


def _rows(x, who, k=None):
    """Validate and return (R, K, dtype code).  Raises before any launch."""
    code = ewops._dtype_code(x, "x")
    if x.dim() < 1:
        raise ValueError("%s: x must have at least one dimension" % who)
    if not x.is_contiguous():
        raise ValueError("%s: x must be contiguous" % who)
    K = int(x.shape[-1])
    if K > MAX_K:
        raise ValueError("%s: rows of up to %d elements are served, got K = %d" % (who, MAX_K, K))
    if k is not None and not (1 <= int(k) <= K):
        raise ValueError("%s: k must lie in 1 .. K = %d, got %s" % (who, K, k))
    return x.numel() // K, K, code


def _mask_rows(x, mask, who):
    """Rows of a valid mask (1 .. R); raises for any other pattern."""
    if not isinstance(mask, torch.Tensor) or mask.device != x.device:
        raise RuntimeError("blocksparse_amd: mask must be a tensor on the device of x (no CPU fallback)")
    if mask.dtype != torch.float32 or not mask.is_contiguous():
        raise ValueError("%s: mask must be a contiguous float32 tensor" % who)
    xs, ms = tuple(x.shape), tuple(mask.shape)
    lead = 0
    while lead < len(ms) and ms[lead] == 1:
        lead += 1
    if len(ms) != len(xs) or ms[-1] != xs[-1] or ms[lead:] != xs[lead:]:
        raise ValueError("%s: mask %s must have the rank of x %s, every dimension x's or 1, the 1s a leading run and the last one K" % (who, ms, xs))
    return mask.numel() // xs[-1]


def _like(t, x, who, what):
    if not isinstance(t, torch.Tensor) or t.shape != x.shape or t.dtype != x.dtype or t.device != x.device:
        raise ValueError("%s: %s must have the shape, dtype and device of x" % (who, what))
    return t.contiguous()


def _args(x, R, K, code, k=1, mask_rows=1, rebase=True, scale=1.0, alpha=1.0):
    return _lib.BsmmSelectArgs(R=R, K=K, k=int(k), mask_rows=int(mask_rows), dtype=code, rebase=1 if rebase else 0, scale=float(scale),
                               alpha=float(alpha), stream=_lib.raw_stream(x.device))


# ---- the low-level forms (no autograd) ------------------------------------------------------------------------------------------------
def rectified_top_k_fwd(x, k, rebase=True):
    """y like x (bsmm_rectified_top_k)."""
    R, K, code = _rows(x, "rectified_top_k", k)
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    a = _args(x, R, K, code, k=k, rebase=rebase)
    _lib.check(_lib.load().bsmm_rectified_top_k(x.data_ptr(), y.data_ptr(), ctypes.byref(a)), "bsmm_rectified_top_k")
    _lib.wrote(y)
    return y


def relu_rule_bwd(dz, y):
    """dx = dz * (y > 0), like y: the gradient of ``rectified_top_k`` and ``sparse_relu`` from the stored y (bsmm_select_relu_grad)."""
    R, K, code = _rows(y, "relu_rule_bwd")
    dz = _like(dz, y, "relu_rule_bwd", "dz")
    dx = torch.empty(y.shape, dtype=y.dtype, device=y.device)
    a = _args(y, R, K, code)
    _lib.check(_lib.load().bsmm_select_relu_grad(dz.data_ptr(), y.data_ptr(), dx.data_ptr(), ctypes.byref(a)), "bsmm_select_relu_grad")
    _lib.wrote(dx)
    return dx


rectified_top_k_bwd = relu_rule_bwd
sparse_relu_bwd = relu_rule_bwd


def masked_top_k_softmax_fwd(x, k, mask=None, scale=1.0):
    """y like x (bsmm_masked_top_k_softmax); k = K is the plain softmax."""
    R, K, code = _rows(x, "masked_top_k_softmax", k)
    rows = 1 if mask is None else _mask_rows(x, mask, "masked_top_k_softmax")
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    a = _args(x, R, K, code, k=k, mask_rows=rows, scale=scale)
    _lib.check(_lib.load().bsmm_masked_top_k_softmax(x.data_ptr(), None if mask is None else mask.data_ptr(), y.data_ptr(), ctypes.byref(a)),
               "bsmm_masked_top_k_softmax")
    _lib.wrote(y)
    return y


def masked_softmax_fwd(x, mask=None, scale=1.0):
    """``masked_top_k_softmax_fwd`` with k = K."""
    R, K, _ = _rows(x, "masked_softmax")
    return masked_top_k_softmax_fwd(x, K, mask, scale)


def masked_softmax_bwd(dy, y, mask=None, scale=1.0):
    """dx like y from the stored y of any of the three softmaxes (bsmm_masked_softmax_grad)."""
    R, K, code = _rows(y, "masked_softmax_bwd")
    dy = _like(dy, y, "masked_softmax_bwd", "dy")
    rows = 1 if mask is None else _mask_rows(y, mask, "masked_softmax_bwd")
    dx = torch.empty(y.shape, dtype=y.dtype, device=y.device)
    a = _args(y, R, K, code, mask_rows=rows, scale=scale)
    _lib.check(_lib.load().bsmm_masked_softmax_grad(dy.data_ptr(), y.data_ptr(), None if mask is None else mask.data_ptr(), dx.data_ptr(),
                                                    ctypes.byref(a)), "bsmm_masked_softmax_grad")
    _lib.wrote(dx)
    return dx


masked_top_k_softmax_bwd = masked_softmax_bwd


def sparse_relu_fwd(x, alpha=1.0):
    """y like x (bsmm_sparse_relu)."""
    R, K, code = _rows(x, "sparse_relu")
    y = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    a = _args(x, R, K, code, alpha=alpha)
    _lib.check(_lib.load().bsmm_sparse_relu(x.data_ptr(), y.data_ptr(), ctypes.byref(a)), "bsmm_sparse_relu")
    _lib.wrote(y)
    return y


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
if torch is not None:
    class _RectifiedTopK(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, k, rebase):
            y = rectified_top_k_fwd(x, k, rebase)
            ctx.save_for_backward(y)
            return y

        @staticmethod
        def backward(ctx, dz):
            (y,) = ctx.saved_tensors
            return relu_rule_bwd(dz.to(y.dtype), y), None, None

    class _TopKSoftmax(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, k, mask, scale):
            y = masked_top_k_softmax_fwd(x, k, mask, scale)
            ctx.scale = scale
            ctx.save_for_backward(y, *(() if mask is None else (mask,)))
            return y

        @staticmethod
        def backward(ctx, dy):
            y = ctx.saved_tensors[0]
            mask = ctx.saved_tensors[1] if len(ctx.saved_tensors) > 1 else None
            return masked_softmax_bwd(dy.to(y.dtype), y, mask, ctx.scale), None, None, None

    class _SparseRelu(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, alpha):
            y = sparse_relu_fwd(x, alpha)
            ctx.save_for_backward(y)
            return y

        @staticmethod
        def backward(ctx, dz):
            (y,) = ctx.saved_tensors
            return relu_rule_bwd(dz.to(y.dtype), y), None


def rectified_top_k(x, k, rebase=True):
    """The k largest elements of every row less ``max(k-th value, 0)`` (``rebase``) and rectified, 0 elsewhere; differentiable in x."""
    _rows(x, "rectified_top_k", k)
    return _RectifiedTopK.apply(x, int(k), bool(rebase))


def masked_top_k_softmax(x, k, mask=None, scale=1.0):
    """The softmax over the k largest scores ``(x * mask) * scale`` of every row, exactly 0 elsewhere; differentiable in x."""
    _rows(x, "masked_top_k_softmax", k)
    if mask is not None:
        _mask_rows(x, mask, "masked_top_k_softmax")
    return _TopKSoftmax.apply(x, int(k), mask, float(scale))


def masked_softmax(x, mask=None, scale=1.0):
    """``masked_top_k_softmax`` with k = K."""
    R, K, _ = _rows(x, "masked_softmax")
    return masked_top_k_softmax(x, K, mask, scale)


def softmax(x, scale=1.0):
    """``masked_softmax`` without a mask."""
    return masked_softmax(x, None, scale)


def sparse_relu(x, alpha=1.0):
    """``max(x - (mean + alpha * sigma), 0)`` with the mean and the population sigma of every row; differentiable in x."""
    _rows(x, "sparse_relu")
    return _SparseRelu.apply(x, float(alpha))


# ---- the NumPy definitions ------------------------------------------------------------------------------------------------------------
def select_keys(v, masked=None):
    """The pinned order as unsigned keys, the integers the kernels compare: a larger key ranks first, equal keys go by index.  ``v``: fp32
    scores; ``masked``: a boolean array like v or None."""
    b = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    mag = b & np.uint32(0x7fffffff)
    key = np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))
    key = np.where(mag == 0, np.uint32(0x80000000), key)                 # -0 counts as +0
    key = np.where(mag > 0x7f800000, np.uint32(0xffffffff), key)         # a NaN above +inf
    if masked is not None:
        key = np.where(masked, np.uint32(0), key)                        # below -inf (0x007fffff)
    return key.astype(np.uint32)


def select_top_k(v, k, masked=None):
    """(S, v_k): the boolean array of the first k elements of every row (last axis) in the pinned order, and the k-th key of every row."""
    key = select_keys(v, masked)
    order = np.argsort(-key.astype(np.int64), axis=-1, kind="stable")    # key descending, then index ascending
    S = np.zeros(key.shape, dtype=bool)
    np.put_along_axis(S, order[..., :k], True, axis=-1)
    return S, np.take_along_axis(key, order[..., k - 1:k], axis=-1)


def _scores(x, mask, scale):
    """fp32 scores (x * m) * scale in that order and the masked elements."""
    x = np.asarray(x, dtype=np.float32)
    if mask is None:
        return x * np.float32(scale), np.zeros(x.shape, dtype=bool)
    m = np.broadcast_to(np.asarray(mask, dtype=np.float32), x.shape)
    return (x * m) * np.float32(scale), m == 0


def rectified_top_k_test(x, k, rebase=True):
    """fp32 y, in fp32 arithmetic (bit for bit what the kernels store in fp32)."""
    v = np.asarray(x, dtype=np.float32)
    S, kth = select_top_k(v, k)
    base = np.zeros(kth.shape, dtype=np.float32)
    if rebase:
        vk = np.take_along_axis(v, np.argmax(S & (select_keys(v) == kth), axis=-1)[..., None], axis=-1)
        base = np.where(vk > 0, vk, np.float32(0)).astype(np.float32)          # (a NaN counts as 0)
    with np.errstate(invalid="ignore"):
        return np.where(S, np.where(v < base, base, v) - base, np.float32(0)).astype(np.float32)


def rectified_top_k_grad_test(dz, y):
    return np.where(np.asarray(y) > 0, np.asarray(dz), 0).astype(np.asarray(dz).dtype)


sparse_relu_grad_test = rectified_top_k_grad_test


def masked_top_k_softmax_test(x, k, mask=None, scale=1.0):
    """fp32 y in fp32 arithmetic; the sum in NumPy's order."""
    v, masked = _scores(x, mask, scale)
    S, _ = select_top_k(v, k, masked)
    S &= ~masked
    with np.errstate(invalid="ignore", over="ignore"):
        vmax = np.max(np.where(masked, -np.inf, v), axis=-1, keepdims=True, initial=-np.inf)
        e = np.where(S, np.exp(np.where(S, v - vmax, 0)), 0).astype(np.float32)
        s = e.sum(axis=-1, keepdims=True, dtype=np.float32)
        return np.where(S, e / np.where(S.any(axis=-1, keepdims=True), s, 1), 0).astype(np.float32)


def masked_softmax_test(x, mask=None, scale=1.0):
    return masked_top_k_softmax_test(x, np.asarray(x).shape[-1], mask, scale)


def softmax_test(x, scale=1.0):
    return masked_softmax_test(x, None, scale)


def masked_softmax_grad_test(dy, y, mask=None, scale=1.0):
    dy, y = np.asarray(dy, dtype=np.float32), np.asarray(y, dtype=np.float32)
    m = np.float32(1) if mask is None else np.asarray(mask, dtype=np.float32)
    return ((dy - np.sum(dy * y, axis=-1, keepdims=True)) * y * m * np.float32(scale)).astype(np.float32)


masked_top_k_softmax_grad_test = masked_softmax_grad_test


def sparse_relu_test(x, alpha=1.0):
    """fp32 y: the cutoff from the mean and the population variance around it."""
    x = np.asarray(x, dtype=np.float32)
    mean = x.mean(axis=-1, keepdims=True, dtype=np.float32)
    var = np.square(x - mean).mean(axis=-1, keepdims=True, dtype=np.float32)
    return np.maximum(x - (mean + np.float32(alpha) * np.sqrt(var)), np.float32(0)).astype(np.float32)
