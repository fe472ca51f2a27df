"""Fused softmax cross-entropy for the last layer of a model: one read of the logits, the loss in fp32, and ``softmax - onehot`` kept in the
logits' dtype so that the backward is one scaled copy.

The reference's name and arguments (blocksparse/transformer.py:685-700) over the C ABI of include/bsmm_ends.h:

    loss = softmax_cross_entropy(logits=y, labels=t)                # y (..., K) fp32 / fp16 / bf16, t integer (...): loss fp32 (...)
    loss, g = softmax_cross_entropy_fwd(y, t)                       # the low-level pair: g like y
    loss, g = softmax_cross_entropy_fwd(y, t, out=y)                # ... in place over the logits
    dx = softmax_cross_entropy_bwd(g, dloss)                        # dx like g; out=g writes over the stash

``labels`` may be uint8, int16, int32 or int64; a label outside [0, K) marks an ignored row (padding): its loss and its gradient are zero.
The loss is ``log(sum exp(x - max)) + max - x[label]`` in fp32 -- not clipped like the reference's ``-log(max(p, 2^-24))``.  A logit of
``-inf`` is a class of probability 0 (a masked class): its ``g`` is exactly 0, and a label on it gives the loss ``+inf`` and ``g[label] = -1``;
a row with no finite logit, or with ``+inf`` or NaN in it, gives NaN in that row only.  An fp16 stash
holds ``XENT_F16_SCALE * (p - onehot)``; the backward undoes the scale.  The autograd function saves the stash, not the logits, and never
works in place.  PyTorch is plumbing (memory, streams, autograd); there is no CPU fallback.

``softmax_cross_entropy_test`` / ``softmax_cross_entropy_grad_test`` are the NumPy definitions, evaluated in float64.
"""
import ctypes

import numpy as np

from . import _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

XENT_F16_SCALE = _lib.XENT_F16_SCALE


def _label_types():
    return (torch.uint8, torch.int16, torch.int32, torch.int64)


def _problem(logits, what):
    if torch is None:
        raise RuntimeError("blocksparse_amd needs PyTorch-ROCm for device memory")
    if not isinstance(logits, torch.Tensor) or logits.device.type != "cuda":
        raise RuntimeError("blocksparse_amd: %s must be a tensor on a ROCm device (no CPU fallback)" % what)
    code = _lib.dtype_code(logits.dtype)
    if code is None:
        raise ValueError("softmax_cross_entropy: %s must be float32, float16 or bfloat16, got %s" % (what, logits.dtype))
    if logits.dim() < 1 or logits.numel() == 0:
        raise ValueError("softmax_cross_entropy: %s must have at least one dimension and one element, got shape %s" % (what, tuple(logits.shape)))
    K = int(logits.shape[-1])
    return logits.numel() // K, K, code


def _labels32(labels, logits, N):
    if not isinstance(labels, torch.Tensor) or labels.device != logits.device or labels.dtype not in _label_types():
        raise ValueError("softmax_cross_entropy: labels must be a uint8, int16, int32 or int64 tensor on the device of the logits")
    if labels.numel() != N:
        raise ValueError("softmax_cross_entropy: %d labels for %d rows of logits" % (labels.numel(), N))
    if labels.dtype == torch.int64:          # (a label beyond int32 names no class: it stays out of range)
        labels = labels.clamp(-1, 2 ** 31 - 1)
    return labels.reshape(-1).to(torch.int32).contiguous()


def xent_path(logits, out=None):
    """The BSMM_XENT_* path the forward takes for these tensors (bsmm_xent_path: host arithmetic)."""
    N, K, code = _problem(logits, "logits")
    a = _lib.BsmmXentArgs(x=logits.data_ptr(), g=(logits if out is None else out).data_ptr(), N=N, K=K, dtype=code)
    return int(_lib.load().bsmm_xent_path(ctypes.byref(a)))


def softmax_cross_entropy_fwd(logits, labels, out=None):
    """(loss, g): loss fp32 shaped like the labels' rows, g = softmax - onehot like the logits (bsmm_xent_fwd).  ``out``: where g goes --
    a contiguous tensor like the logits, which may be the logits themselves (the forward in place)."""
    N, K, code = _problem(logits, "logits")
    lab = _labels32(labels, logits, N)
    if out is None:
        x = logits.contiguous()
        g = torch.empty_like(x)
    else:
        x = logits
        g = out
        if not isinstance(g, torch.Tensor) or g.shape != x.shape or g.dtype != x.dtype or g.device != x.device:
            raise ValueError("softmax_cross_entropy_fwd: out must have the shape, dtype and device of the logits")
        if not x.is_contiguous() or not g.is_contiguous():
            raise ValueError("softmax_cross_entropy_fwd: with out=, the logits and out must be contiguous")
    loss = torch.empty(tuple(logits.shape[:-1]), dtype=torch.float32, device=x.device)
    a = _lib.BsmmXentArgs(x=x.data_ptr(), labels=lab.data_ptr(), loss=loss.data_ptr(), g=g.data_ptr(), N=N, K=K, dtype=code,
                          stream=_lib.raw_stream(x.device))
    _lib.check(_lib.load().bsmm_xent_fwd(ctypes.byref(a)), "bsmm_xent_fwd")
    _lib.wrote(loss, g)
    return loss, g


def softmax_cross_entropy_bwd(g, dy, out=None):
    """dx = unscale(g) * dy per row, like g (bsmm_xent_bwd).  dy: fp32 with one element per row.  ``out`` may be g."""
    N, K, code = _problem(g, "g")
    if not isinstance(dy, torch.Tensor) or dy.device != g.device or dy.numel() != N:
        raise ValueError("softmax_cross_entropy_bwd: dy must be a tensor with %d elements on the device of g" % N)
    dy = dy.reshape(-1).to(torch.float32).contiguous()
    if out is None:
        g = g.contiguous()
        dx = torch.empty_like(g)
    else:
        dx = out
        if not isinstance(dx, torch.Tensor) or dx.shape != g.shape or dx.dtype != g.dtype or dx.device != g.device:
            raise ValueError("softmax_cross_entropy_bwd: out must have the shape, dtype and device of g")
        if not g.is_contiguous() or not dx.is_contiguous():
            raise ValueError("softmax_cross_entropy_bwd: with out=, g and out must be contiguous")
    a = _lib.BsmmXentArgs(g=g.data_ptr(), dy=dy.data_ptr(), dx=dx.data_ptr(), N=N, K=K, dtype=code, stream=_lib.raw_stream(g.device))
    _lib.check(_lib.load().bsmm_xent_bwd(ctypes.byref(a)), "bsmm_xent_bwd")
    _lib.wrote(dx)
    return dx


if torch is not None:
    class _SoftmaxCrossEntropy(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, labels):
            loss, g = softmax_cross_entropy_fwd(logits, labels)
            ctx.save_for_backward(g)
            return loss

        @staticmethod
        def backward(ctx, dy):
            g, = ctx.saved_tensors
            return softmax_cross_entropy_bwd(g, dy), None


def softmax_cross_entropy(logits=None, labels=None):
    """loss[n] = -log softmax(logits[n])[labels[n]] in fp32; differentiable in the logits."""
    _problem(logits, "logits")
    return _SoftmaxCrossEntropy.apply(logits, labels)


# ---- the NumPy definitions ------------------------------------------------------------------------------------------------------------
def softmax_cross_entropy_test(logits, labels):
    """(loss, g) in float64: g = softmax - onehot, UNSCALED; a label outside [0, K) gives loss 0 and a row of zeros."""
    x = np.asarray(logits, dtype=np.float64)
    K = x.shape[-1]
    x2 = x.reshape(-1, K)
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    live = (lab >= 0) & (lab < K)
    safe = np.where(live, lab, 0)
    m = x2.max(axis=1, keepdims=True)
    e = np.exp(x2 - m)
    s = e.sum(axis=1, keepdims=True)
    rows = np.arange(x2.shape[0])
    loss = np.log(s[:, 0]) + m[:, 0] - x2[rows, safe]
    g = e / s
    g[rows, safe] -= 1.0
    loss = np.where(live, loss, 0.0)
    g = np.where(live[:, None], g, 0.0)
    return loss.reshape(x.shape[:-1]), g.reshape(x.shape)


def softmax_cross_entropy_grad_test(g, dy):
    """dx in float64 from the UNSCALED g and dy (one value per row)."""
    g = np.asarray(g, dtype=np.float64)
    return g * np.asarray(dy, dtype=np.float64).reshape(g.shape[:-1] + (1,))
