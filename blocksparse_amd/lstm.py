"""The fused LSTM gates: what a recurrent model runs between two block-sparse matmuls, as one launch each way, in both activation layouts of
the matmul.

The reference's name and arguments (blocksparse/lstm.py:22-74) plus ``axis``, over the C ABI of include/bsmm_lstm.h:

    c_next, h_next = fused_lstm_gates(c, h, bias=b, forget_bias=1.0)            # c (N, K), h (N, 4K): column slices i | u | f | o
    c_next, h_next = fused_lstm_gates(c, h, axis=0)                             # c (K, N), h (4K, N): four contiguous (K, N) chunks,
                                                                                #   what layer_norm(h, g, b, axis=0, segments=4) produces
    c_next, h_next = fused_lstm_gates(c, i, u, f, o)                            # four tensors like c; no bias in this form

    si = sigmoid(i + b_i)    tu = tanh(u + b_u)    sf = sigmoid(f + b_f + forget_bias)    so = sigmoid(o + b_o)
    c_next = sf * c + si * tu            h_next = so * tanh(c_next)

``c`` is fp32, fp16 or bf16 of any rank: ``axis=0`` takes the leading dimension as the cells (the others are flattened into N), ``axis=-1``
or ``rank - 1`` the last one; the gates have the dtype of ``c``.  ``bias`` is fp32 with 4K elements.  All arithmetic is fp32, every stored
value is rounded once; sigmoid and tanh saturate to finite values.  The backward recomputes the activations from the saved inputs and
writes the four gate gradients of the fused form into ONE tensor shaped like ``h``; the bias gradient is ``ewops.bias_relu_bwd`` on that
tensor (fp32, summed in a fixed order).  PyTorch is plumbing (memory, streams, autograd); there is no CPU fallback.

``fused_lstm_gates_test`` / ``fused_lstm_gates_grad_test`` are the NumPy definitions.

Not here: ``split4`` / ``concat4`` (torch views and ``torch.cat``), ``FusedBasicLSTMCell``, ``grouped_lstm``,
``group_lstm_grads``, gradients in another dtype than the forward's, a second addend fused into the gates, and a bias gradient fused into
the backward launch.  ``sparse_relu`` lives in blocksparse_amd/select.py.
"""
import ctypes

import numpy as np

from . import _lib
from . import ewops

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def _problem(c, gates, bias, axis):
    """Validate and return (axis as 0 / 1, K, N, dtype code).  Raises before any launch."""
    if len(gates) not in (1, 4):
        raise ValueError("fused_lstm_gates: pass the fused gate tensor or the four tensors i, u, f, o, got %d tensors" % len(gates))
    if len(gates) == 4 and bias is not None:
        raise ValueError("fused_lstm_gates: a bias is not enabled with four gate tensors")
    code = ewops._dtype_code(c, "c")
    if c.dim() < 1:
        raise ValueError("fused_lstm_gates: c must have at least one dimension")
    axis = int(axis)
    if axis < 0:
        axis += c.dim()
    if axis != 0 and axis != c.dim() - 1:
        raise ValueError("fused_lstm_gates: axis must be 0 or the last dimension of c (rank %d), got %d" % (c.dim(), axis))
    K = int(c.shape[axis])
    if 4 * K >= 2 ** 31:
        raise ValueError("fused_lstm_gates: 4 * K must stay below 2^31, got K = %d" % K)
    want = list(c.shape)
    if len(gates) == 1:
        want[axis] = 4 * K
    for g in gates:
        if not isinstance(g, torch.Tensor) or g.device != c.device or g.dtype != c.dtype or list(g.shape) != want:
            raise ValueError("fused_lstm_gates: a gate tensor must have shape %s and the dtype and device of c" % (tuple(want),))
    for t in (c,) + tuple(gates):
        if not t.is_contiguous():
            raise ValueError("fused_lstm_gates: c and the gate tensors must be contiguous")
    if bias is not None:
        if not isinstance(bias, torch.Tensor) or bias.device.type != "cuda":
            raise RuntimeError("blocksparse_amd: bias must be a tensor on a ROCm device (no CPU fallback)")
        if bias.dtype != torch.float32 or bias.numel() != 4 * K or bias.device != c.device:
            raise ValueError("fused_lstm_gates: bias must be a float32 tensor with 4 K = %d elements on the device of c" % (4 * K))
    return (0 if axis == 0 else 1), K, c.numel() // K, code


def _gate_ptrs(gates, ax, K, N):
    """(four addresses, leading dimension) of the gates: the four tensors, or the slices of the fused one."""
    if len(gates) == 4:
        return [g.data_ptr() for g in gates], K
    h = gates[0]
    step = (K if ax == 1 else K * N) * h.element_size()
    return [h.data_ptr() + q * step for q in range(4)], 4 * K


def _like(t, c, what):
    if not isinstance(t, torch.Tensor) or t.shape != c.shape or t.dtype != c.dtype or t.device != c.device:
        raise ValueError("fused_lstm_gates: %s must have the shape, dtype and device of c" % what)
    return t.contiguous()


# ---- the low-level forms (no autograd) ------------------------------------------------------------------------------------------------
def fused_lstm_gates_fwd(c, *gates, bias=None, forget_bias=1.0, axis=-1):
    """(c_next, h_next), like c (bsmm_lstm_gates)."""
    ax, K, N, code = _problem(c, gates, bias, axis)
    bias = None if bias is None else bias.contiguous()
    ptrs, ld = _gate_ptrs(gates, ax, K, N)
    c_next = torch.empty(c.shape, dtype=c.dtype, device=c.device)
    h_next = torch.empty(c.shape, dtype=c.dtype, device=c.device)
    a = _lib.BsmmLstmArgs(K=K, N=N, axis=ax, dtype=code, gate_ld=ld, dgate_ld=ld, forget_bias=float(forget_bias), stream=_lib.raw_stream(c.device))
    _lib.check(_lib.load().bsmm_lstm_gates(c.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ptrs[3], None if bias is None else bias.data_ptr(),
                                           c_next.data_ptr(), h_next.data_ptr(), ctypes.byref(a)), "bsmm_lstm_gates")
    _lib.wrote(c_next, h_next)
    return c_next, h_next


def fused_lstm_gates_bwd(c, *gates, eh=None, ec=None, bias=None, forget_bias=1.0, axis=-1):
    """(dc, dgates) of ``fused_lstm_gates_fwd`` from the gradients ``eh`` of h_next and ``ec`` of c_next (either may be None: zero).
    ``dgates`` is ONE tensor shaped like the fused gate tensor, or the tuple (di, du, df, do) in the four-tensor form
    (bsmm_lstm_gates_grad).  The bias gradient is ``ewops.bias_relu_bwd(dgates, None, bias, axis)[1]``."""
    ax, K, N, code = _problem(c, gates, bias, axis)
    if eh is None and ec is None:
        raise ValueError("fused_lstm_gates_bwd: eh and ec cannot both be None")
    eh = None if eh is None else _like(eh, c, "eh")
    ec = None if ec is None else _like(ec, c, "ec")
    bias = None if bias is None else bias.contiguous()
    ptrs, ld = _gate_ptrs(gates, ax, K, N)
    dc = torch.empty(c.shape, dtype=c.dtype, device=c.device)
    dgates = tuple(torch.empty(g.shape, dtype=g.dtype, device=g.device) for g in gates)
    dptrs, dld = _gate_ptrs(dgates, ax, K, N)
    a = _lib.BsmmLstmArgs(K=K, N=N, axis=ax, dtype=code, gate_ld=ld, dgate_ld=dld, forget_bias=float(forget_bias), stream=_lib.raw_stream(c.device))
    ptr = lambda t: None if t is None else t.data_ptr()
    _lib.check(_lib.load().bsmm_lstm_gates_grad(c.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ptrs[3], ptr(bias), ptr(eh), ptr(ec), dc.data_ptr(),
                                                dptrs[0], dptrs[1], dptrs[2], dptrs[3], ctypes.byref(a)), "bsmm_lstm_gates_grad")
    _lib.wrote(dc, *dgates)
    return dc, (dgates[0] if len(gates) == 1 else dgates)


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------
if torch is not None:
    class _LstmGates(torch.autograd.Function):
        @staticmethod
        def forward(ctx, c, bias, forget_bias, axis, *gates):
            c_next, h_next = fused_lstm_gates_fwd(c, *gates, bias=bias, forget_bias=forget_bias, axis=axis)
            ctx.cfg = (forget_bias, axis, bias is not None)
            ctx.set_materialize_grads(False)             # an absent gradient stays None: the kernel reads one stream less
            ctx.save_for_backward(c, *(gates + ((bias,) if bias is not None else ())))
            return c_next, h_next

        @staticmethod
        def backward(ctx, ec, eh):
            forget_bias, axis, has_bias = ctx.cfg
            saved = ctx.saved_tensors
            c, bias = saved[0], (saved[-1] if has_bias else None)
            gates = saved[1:-1] if has_bias else saved[1:]
            if ec is None and eh is None:
                return (None,) * (4 + len(gates))
            ec = None if ec is None else ec.to(c.dtype)
            eh = None if eh is None else eh.to(c.dtype)
            dc, dg = fused_lstm_gates_bwd(c, *gates, eh=eh, ec=ec, bias=bias, forget_bias=forget_bias, axis=axis)
            db = None
            if has_bias:                                 # one more launch: the sum of the stored gate gradients, as the reference does
                db = ewops.bias_relu_bwd(dg, None, bias, axis=axis)[1]
            return (dc, db, None, None) + (dg if isinstance(dg, tuple) else (dg,))


def fused_lstm_gates(c, *args, bias=None, forget_bias=1.0, axis=-1, name=None):
    """(c_next, h_next) of the LSTM cell; differentiable in c, the gates and the bias.  ``args`` is the fused gate tensor -- (..., 4K) with
    ``axis=-1``, (4K, ...) with ``axis=0`` -- or the four tensors i, u, f, o shaped like c, and then ``bias`` must be None.  ``name`` is
    accepted for the reference's signature and ignored."""
    _problem(c, args, bias, axis)
    return _LstmGates.apply(c, bias, float(forget_bias), int(axis), *args)


# ---- the NumPy definitions ------------------------------------------------------------------------------------------------------------
def _np_sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e)).astype(x.dtype, copy=False)


def _np_gates(c, args, bias, axis):
    """(i, u, f, o) with the bias added, each shaped like c."""
    c = np.asarray(c)
    if len(args) not in (1, 4):
        raise ValueError("fused_lstm_gates: pass the fused gate tensor or the four tensors i, u, f, o, got %d tensors" % len(args))
    if len(args) == 4:
        if bias is not None:
            raise ValueError("fused_lstm_gates: a bias is not enabled with four gate tensors")
        return tuple(np.asarray(g) for g in args)
    h = np.asarray(args[0])
    ax = axis + c.ndim if axis < 0 else axis
    if ax != 0 and ax != c.ndim - 1:
        raise ValueError("fused_lstm_gates: axis must be 0 or the last dimension of c")
    K = c.shape[ax]
    if bias is not None:
        h = h + np.asarray(bias).reshape(tuple(4 * K if d == ax else 1 for d in range(c.ndim))).astype(h.dtype, copy=False)
    return tuple(np.take(h, np.arange(q * K, (q + 1) * K), axis=ax) for q in range(4))


def fused_lstm_gates_test(c, *args, bias=None, forget_bias=1.0, axis=-1):
    """(c_next, h_next) in the dtype of c."""
    c = np.asarray(c)
    i, u, f, o = _np_gates(c, args, bias, axis)
    c_next = _np_sigmoid(f + c.dtype.type(forget_bias)) * c + _np_sigmoid(i) * np.tanh(u)
    h_next = _np_sigmoid(o) * np.tanh(c_next)
    return c_next.astype(c.dtype, copy=False), h_next.astype(c.dtype, copy=False)


def fused_lstm_gates_grad_test(c, *args, eh=None, ec=None, bias=None, forget_bias=1.0, axis=-1):
    """(dc, dh) for the fused gate tensor -- (dc, dh, db) with a bias -- and (dc, di, du, df, do) for four tensors."""
    c = np.asarray(c)
    if eh is None and ec is None:
        raise ValueError("fused_lstm_gates_grad_test: eh and ec cannot both be None")
    eh = np.zeros_like(c) if eh is None else np.asarray(eh)
    ec = np.zeros_like(c) if ec is None else np.asarray(ec)
    i, u, f, o = _np_gates(c, args, bias, axis)
    si, tu, sf, so = _np_sigmoid(i), np.tanh(u), _np_sigmoid(f + c.dtype.type(forget_bias)), _np_sigmoid(o)
    ca = np.tanh(sf * c + si * tu)
    dC = eh * so * (1 - ca * ca) + ec
    d = [dC * tu * si * (1 - si), dC * si * (1 - tu * tu), dC * c * sf * (1 - sf), eh * ca * so * (1 - so)]
    d = [g.astype(c.dtype, copy=False) for g in d]
    dc = (dC * sf).astype(c.dtype, copy=False)
    if len(args) == 4:
        return (dc,) + tuple(d)
    ax = axis + c.ndim if axis < 0 else axis
    dh = np.concatenate(d, axis=ax)
    if bias is None:
        return dc, dh
    db = dh.sum(axis=tuple(q for q in range(c.ndim) if q != ax))
    return dc, dh, db.astype(np.asarray(bias).dtype, copy=False).reshape(np.asarray(bias).shape)
