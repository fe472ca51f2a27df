"""Layer norm between block-sparse layers, in both activation layouts of the matmul, with the fused ReLU and fp32 gain / bias gradients.

The reference's name and arguments (blocksparse/norms.py:23-67; its TF-only ``atomics``, ``bench`` and ``use_tf`` are gone) over the C ABI
of include/bsmm_norm.h:

    y = layer_norm(x, g, b, axis=0)                              # x (C, N): the layout of feature_axis=0 matmuls; torch has no such op
    y = layer_norm(x, g, b, axis=1, segments=4, relu=True)       # x (N, C): four runs of C / 4 features normalised alone, then ReLU
    y, mean, rstd = layer_norm_fwd(x, g, b, axis=0)              # the low-level pair: mean / rstd are fp32 [segments, N]
    dx, dg, db = layer_norm_bwd(dy, x, g, b, mean, rstd, axis=0)

``x`` is fp32, fp16 or bf16 of any rank: ``axis=0`` normalises the leading dimension (the others are flattened into N), ``axis=-1`` or
``rank - 1`` the last one.  ``g`` and ``b`` are fp32 with K elements in any shape; their gradients are fp32 in every dtype.  All statistics
and the ReLU are fp32, the result is rounded once.  PyTorch is plumbing (memory, streams, autograd); there is no CPU fallback.

``layer_norm_test`` / ``layer_norm_grad_test`` are the NumPy definitions with the reference's names and argument order
(blocksparse/norms.py:103-180), written here vectorised over the segments.
"""
import ctypes

import numpy as np

from . import _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def _problem(x, g, b, axis, segments):
    """Validate and return (axis as 0 / 1, K, N, segments, dtype code).  Raises before anything is launched."""
    if torch is None:
        raise RuntimeError("blocksparse_amd needs PyTorch-ROCm for device memory")
    for t, what in ((x, "x"), (g, "g"), (b, "b")):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError("blocksparse_amd: %s must be a tensor on a ROCm device (no CPU fallback)" % what)
    code = _lib.dtype_code(x.dtype)
    if code is None:
        raise ValueError("layer_norm: x must be float32, float16 or bfloat16, got %s" % x.dtype)
    if x.dim() < 1 or x.numel() == 0:
        raise ValueError("layer_norm: x must have at least one dimension and one element, got shape %s" % (tuple(x.shape),))
    axis = int(axis)
    if axis < 0:
        axis += x.dim()
    if axis != 0 and axis != x.dim() - 1:
        raise ValueError("layer_norm: axis must be 0 or the last dimension of x (rank %d), got %d" % (x.dim(), axis))
    K = int(x.shape[axis])
    N = x.numel() // K
    segments = int(segments)
    if segments < 1 or K % segments != 0:
        raise ValueError("layer_norm: segments (%d) must be >= 1 and divide the %d features" % (segments, K))
    for t, what in ((g, "g"), (b, "b")):
        if t.dtype != torch.float32 or t.numel() != K or t.device != x.device:
            raise ValueError("layer_norm: %s must be a float32 tensor with %d elements on the device of x" % (what, K))
    return (0 if axis == 0 else 1), K, N, segments, code


def _args(device, ax, K, N, S, code, epsilon, relu, backward):
    """The argument struct and the workspace tensor it points into (torch's allocator, per call)."""
    a = _lib.BsmmLnArgs(K=K, N=N, segments=S, axis=ax, dtype=code, relu=1 if relu else 0, epsilon=float(epsilon), workspace=None,
                        workspace_bytes=0, stream=_lib.raw_stream(device))
    need = int(_lib.load().bsmm_layer_norm_workspace_bytes(ctypes.byref(a), backward))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    return a, ws


def layer_norm_fwd(x, g, b, axis=1, segments=1, epsilon=1e-6, relu=False):
    """(y, mean, rstd): y like x; mean and rstd fp32 [segments, N] (bsmm_layer_norm)."""
    ax, K, N, S, code = _problem(x, g, b, axis, segments)
    x, g, b = x.contiguous(), g.contiguous(), b.contiguous()
    y = torch.empty_like(x)
    mean = torch.empty((S, N), dtype=torch.float32, device=x.device)
    rstd = torch.empty((S, N), dtype=torch.float32, device=x.device)
    a, ws = _args(x.device, ax, K, N, S, code, epsilon, relu, 0)
    _lib.check(_lib.load().bsmm_layer_norm(x.data_ptr(), g.data_ptr(), b.data_ptr(), y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ctypes.byref(a)),
               "bsmm_layer_norm")
    _lib.wrote(y, mean, rstd)
    return y, mean, rstd


def layer_norm_bwd(dy, x, g, b, mean, rstd, axis=1, segments=1, epsilon=1e-6, relu=False):
    """(dx, dg, db) from what ``layer_norm_fwd`` took and returned: dx like x, dg / db fp32 shaped like g / b (bsmm_layer_norm_grad)."""
    ax, K, N, S, code = _problem(x, g, b, axis, segments)
    if not isinstance(dy, torch.Tensor) or dy.shape != x.shape or dy.dtype != x.dtype or dy.device != x.device:
        raise ValueError("layer_norm_bwd: dy must have the shape, dtype and device of x")
    for t, what in ((mean, "mean"), (rstd, "rstd")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != S * N or t.device != x.device:
            raise ValueError("layer_norm_bwd: %s must be a float32 tensor with segments * N = %d elements on the device of x" % (what, S * N))
    dy, x, g, b, mean, rstd = (t.contiguous() for t in (dy, x, g, b, mean, rstd))
    dx = torch.empty_like(x)
    dg = torch.empty(g.shape, dtype=torch.float32, device=x.device)
    db = torch.empty(b.shape, dtype=torch.float32, device=x.device)
    a, ws = _args(x.device, ax, K, N, S, code, epsilon, relu, 1)
    _lib.check(_lib.load().bsmm_layer_norm_grad(dy.data_ptr(), x.data_ptr(), g.data_ptr(), b.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                                dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ctypes.byref(a)), "bsmm_layer_norm_grad")
    _lib.wrote(dx, dg, db)
    return dx, dg, db


if torch is not None:
    class _LayerNorm(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, g, b, axis, segments, epsilon, relu):
            y, mean, rstd = layer_norm_fwd(x, g, b, axis, segments, epsilon, relu)
            ctx.save_for_backward(x, g, b, mean, rstd)
            ctx.cfg = (axis, segments, epsilon, relu)
            return y

        @staticmethod
        def backward(ctx, dy):
            x, g, b, mean, rstd = ctx.saved_tensors
            axis, segments, epsilon, relu = ctx.cfg
            dx, dg, db = layer_norm_bwd(dy.to(x.dtype), x, g, b, mean, rstd, axis, segments, epsilon, relu)
            return dx, dg, db, None, None, None, None


def layer_norm(x, g, b, axis=1, segments=1, epsilon=1e-6, relu=False):
    """y = (x - mean) * rstd * g + b per segment of ``axis`` and per sample, then ReLU if asked; differentiable in x, g and b."""
    _problem(x, g, b, axis, segments)
    return _LayerNorm.apply(x, g, b, int(axis), int(segments), float(epsilon), bool(relu))


# ---- the NumPy definitions ------------------------------------------------------------------------------------------------------------
def _as_segments(a, K, axis, segments):
    """(S, K / S, N) for axis 0, (N, S, K / S) otherwise; the reduced axis of the view is 1 resp. 2."""
    return a.reshape(segments, K // segments, -1) if axis == 0 else a.reshape(-1, segments, K // segments)


def layer_norm_test(x, g, b, axis=1, segments=1, epsilon=1e-6, relu=False):
    x = np.asarray(x)
    K = x.shape[axis]
    ax = 0 if axis == 0 else 1
    red = 1 if ax == 0 else 2
    xs = _as_segments(x, K, ax, segments)
    gs = np.asarray(g).reshape((segments, K // segments, 1) if ax == 0 else (1, segments, K // segments))
    bs = np.asarray(b).reshape(gs.shape)
    mean = np.mean(xs, axis=red, keepdims=True)
    var = np.var(xs, axis=red, keepdims=True)
    rstd = np.reciprocal(np.sqrt(var + epsilon))
    y = (xs - mean) * rstd * gs + bs
    if relu:
        y = np.maximum(y, 0.0)
    return y.astype(x.dtype, copy=False).reshape(x.shape)


def layer_norm_grad_test(dy, x, g, b, axis=1, segments=1, epsilon=1e-6, relu=False):
    x, dy, g, b = np.asarray(x), np.asarray(dy), np.asarray(g), np.asarray(b)
    K = x.shape[axis]
    ax = 0 if axis == 0 else 1
    red, other = (1, 2) if ax == 0 else (2, 0)
    Ks = K // segments
    xs, dys = _as_segments(x, K, ax, segments), _as_segments(dy, K, ax, segments)
    gshape = (segments, Ks, 1) if ax == 0 else (1, segments, Ks)
    gs, bs = g.reshape(gshape), b.reshape(gshape)
    mean = np.mean(xs, axis=red, keepdims=True)
    rstd = np.reciprocal(np.sqrt(np.var(xs, axis=red, keepdims=True) + epsilon))
    xhat = (xs - mean) * rstd
    if relu:
        dys = dys * ((xhat * gs + bs) > 0.0)
    dg = np.sum(dys * xhat, axis=other, keepdims=True)
    db = np.sum(dys, axis=other, keepdims=True)
    dyg = dys * gs
    sum1 = np.sum(xhat * dyg, axis=red, keepdims=True)
    sum2 = np.sum(dyg, axis=red, keepdims=True)
    dx = (dyg - (xhat * sum1 + sum2) / float(Ks)) * rstd
    gout = (K, 1) if ax == 0 else (1, K)                  # (the reference returns dg / db in the 2-D shape it reshaped g / b to)
    return dx.astype(dy.dtype, copy=False).reshape(x.shape), dg.astype(g.dtype, copy=False).reshape(gout), db.astype(b.dtype, copy=False).reshape(gout)
