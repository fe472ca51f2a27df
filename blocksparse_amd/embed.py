"""Embedding lookup for the first layer of a model, with a gradient that is summed in a fixed order: the same arguments give the same bits.

The reference's name and arguments (blocksparse/embed.py) over the C ABI of include/bsmm_ends.h:

    y = embedding_lookup(emb, idx)                                  # emb (C, K) fp32 / fp16 / bf16, idx integer of any shape: y idx.shape + (K,)
    y, order = embedding_lookup_fwd(emb, idx)                       # the low-level pair; order: the inverted index the backward reads through
    dw = embedding_lookup_bwd(dy, idx, C, order=order)              # dw fp32 (C, K), every element stored

``idx`` may be uint8, int16, int32 or int64.  An index outside [0, C) reads as a row of zeros and contributes nothing to the gradient.  The
gradient is fp32 whatever the table's dtype, as in the reference; ``emb.grad`` receives it cast to the table's dtype, as autograd requires.
It uses no atomics: the contribution rows of one table row are added in ascending position, in chunks of a fixed length, whatever the
distribution of the indices.  ``sort_grad`` is accepted and ignored (the reference's ``sort_grad=False`` is its atomic variant, which is not
built), as ``atomics=`` is in ``bias_relu``.  The inverted index is ``torch.sort(idx, stable=True)``, built once per forward and kept for the
backward; it works under stream capture.  PyTorch is plumbing (memory, streams, autograd, the sort); there is no CPU fallback.

``embedding_lookup_test`` / ``embedding_lookup_grad_test`` are the NumPy definitions.
"""
import ctypes

import numpy as np

from . import _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def _idx32(idx, device):
    if torch is None:
        raise RuntimeError("blocksparse_amd needs PyTorch-ROCm for device memory")
    if not isinstance(idx, torch.Tensor) or idx.device.type != "cuda" or idx.device != device:
        raise RuntimeError("blocksparse_amd: idx must be a tensor on the ROCm device of the table (no CPU fallback)")
    if idx.dtype not in (torch.uint8, torch.int16, torch.int32, torch.int64):
        raise ValueError("embedding_lookup: idx must be uint8, int16, int32 or int64, got %s" % idx.dtype)
    if idx.numel() == 0:
        raise ValueError("embedding_lookup: idx must have at least one element")
    if idx.dtype == torch.int64:             # (an index beyond int32 names no row: it stays out of range)
        idx = idx.clamp(-1, 2 ** 31 - 1)
    return idx.reshape(-1).to(torch.int32).contiguous()


def _table(t, what):
    if torch is None:
        raise RuntimeError("blocksparse_amd needs PyTorch-ROCm for device memory")
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError("blocksparse_amd: %s must be a tensor on a ROCm device (no CPU fallback)" % what)
    code = _lib.dtype_code(t.dtype)
    if code is None:
        raise ValueError("embedding_lookup: %s must be float32, float16 or bfloat16, got %s" % (what, t.dtype))
    return code


def sort_order(idx):
    """The inverted index of bsmm_embed_grad: int32 positions that sort the flattened idx ascending, ties in ascending position."""
    flat = idx.reshape(-1)
    if flat.dtype == torch.uint8:            # (sorted as wider integers: the order is the same)
        flat = flat.to(torch.int16)
    return torch.sort(flat, stable=True)[1].to(torch.int32)


def embedding_lookup_fwd(emb, idx, want_order=True):
    """(y, order): y = emb[idx] with zeros for indices outside the table (bsmm_embed_fwd); order = sort_order(idx) or None."""
    code = _table(emb, "emb")
    if emb.dim() != 2 or emb.numel() == 0:
        raise ValueError("embedding_lookup: emb must be a (C, K) matrix, got shape %s" % (tuple(emb.shape),))
    i32 = _idx32(idx, emb.device)
    emb = emb.contiguous()
    C, K = int(emb.shape[0]), int(emb.shape[1])
    y = torch.empty(tuple(idx.shape) + (K,), dtype=emb.dtype, device=emb.device)
    a = _lib.BsmmEmbedArgs(C=C, K=K, nIdx=i32.numel(), dtype=code, workspace=None, workspace_bytes=0, stream=_lib.raw_stream(emb.device))
    _lib.check(_lib.load().bsmm_embed_fwd(emb.data_ptr(), i32.data_ptr(), y.data_ptr(), ctypes.byref(a)), "bsmm_embed_fwd")
    _lib.wrote(y)
    return y, (sort_order(i32) if want_order else None)


def embedding_lookup_bwd(dy, idx, C, order=None):
    """dw fp32 (C, K) = the rows of dy added per index (bsmm_embed_grad).  ``order``: what the forward returned, or None to sort here."""
    code = _table(dy, "dy")
    i32 = _idx32(idx, dy.device)
    n = i32.numel()
    if dy.dim() < 1 or dy.numel() == 0 or dy.numel() % n != 0 or tuple(dy.shape[:-1]) != tuple(idx.shape):
        raise ValueError("embedding_lookup_bwd: dy must be shaped idx.shape + (K,), got %s for idx %s" % (tuple(dy.shape), tuple(idx.shape)))
    K, C = int(dy.shape[-1]), int(C)
    if order is None:
        order = sort_order(i32)
    if not isinstance(order, torch.Tensor) or order.dtype != torch.int32 or order.numel() != n or order.device != dy.device:
        raise ValueError("embedding_lookup_bwd: order must be an int32 tensor with one entry per index on the device of dy")
    dy, order = dy.contiguous(), order.contiguous()
    a = _lib.BsmmEmbedArgs(C=C, K=K, nIdx=n, dtype=code, workspace=None, workspace_bytes=0, stream=_lib.raw_stream(dy.device))
    need = int(_lib.load().bsmm_ends_workspace_bytes(ctypes.byref(a), _lib.ENDS_EMBED_GRAD))
    if need == 0:
        raise ValueError("embedding_lookup_bwd: bad sizes C=%d K=%d nIdx=%d" % (C, K, n))
    ws = torch.empty(need // 4, dtype=torch.float32, device=dy.device)
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    dw = torch.empty((C, K), dtype=torch.float32, device=dy.device)
    _lib.check(_lib.load().bsmm_embed_grad(dy.data_ptr(), i32.data_ptr(), order.data_ptr(), dw.data_ptr(), ctypes.byref(a)), "bsmm_embed_grad")
    _lib.wrote(dw, ws)
    return dw


if torch is not None:
    class _EmbeddingLookup(torch.autograd.Function):
        @staticmethod
        def forward(ctx, emb, idx):
            y, order = embedding_lookup_fwd(emb, idx)
            ctx.save_for_backward(idx, order)
            ctx.table = (int(emb.shape[0]), emb.dtype)
            return y

        @staticmethod
        def backward(ctx, dy):
            idx, order = ctx.saved_tensors
            C, dtype = ctx.table
            return embedding_lookup_bwd(dy, idx, C, order=order).to(dtype), None


def embedding_lookup(emb, idx, sort_grad=True):
    """y = emb[idx]; differentiable in emb."""
    _table(emb, "emb")
    return _EmbeddingLookup.apply(emb, idx)


# ---- the NumPy definitions ------------------------------------------------------------------------------------------------------------
def embedding_lookup_test(emb, idx):
    emb, idx = np.asarray(emb), np.asarray(idx).astype(np.int64)
    live = (idx >= 0) & (idx < emb.shape[0])
    y = emb[np.where(live, idx, 0)]
    return np.where(live[..., None], y, np.zeros((), dtype=emb.dtype))


def embedding_lookup_grad_test(dy, idx, C):
    """dw (C, K) in float64."""
    dy, idx = np.asarray(dy, dtype=np.float64), np.asarray(idx).astype(np.int64).reshape(-1)
    dy = dy.reshape(idx.size, -1)
    live = (idx >= 0) & (idx < C)
    dw = np.zeros((int(C), dy.shape[1]), dtype=np.float64)
    np.add.at(dw, idx[live], dy[live])
    return dw
