"""Dynamic sparsity: which blocks of a block-sparse layer to drop, and which absent blocks to add.

The reference's names and arguments (blocksparse/optimize.py:292-341, blocksparse/matmul.py:556-609) over the C ABI of
include/bsmm_sparsity.h:

    norms = blocksparse_norm(w, norm="max")                       # fp32 [blocks]
    blocksparse_l2_decay(w, gate=gate, rate=0.05)                 # group lasso, in place
    blocksparse_prune(w, gate, step, sparsity=0.5)                # gate <- 0 / 1, in place
    score = bsmm.block_reduced_full_dw(xs, dys)                   # fp32 [CB, KB]: a growth score for EVERY block of the dense grid
    score = bsmm.block_reduced_full_dw(xs, dys, exact=True)       # the true per-block norm of the dense gradient
    new_bsmm, new_w = bsmm.relayout(w, new_layout)                # carry the weights over to another layout

The reduced score is an UPPER BOUND of the true block norm, not an estimate of it (|sum_n x_in y_jn| <= sum_n max_i |x_in| max_j |y_jn| and
||sum_n x_n y_n^T||_F <= sum_n ||x_n|| ||y_n||): on i.i.d. data it is tens of times the true norm.  ``exact=True`` costs a dense weight
gradient and gives the norm itself.  PyTorch is plumbing here as everywhere in the package (memory, streams, the sort of `blocks`
norms); there is no CPU fallback.
"""
import ctypes

import numpy as np

from . import _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

_BSIZES = (8, 16, 32, 64)
_dtype_code = _lib.require_dtype_code


def _norm_code(norm):
    n = str(norm).lower()
    if n not in ("max", "l2"):
        raise ValueError("norm must be 'max' or 'l2'")
    return _lib.NORM_L2 if n == "l2" else _lib.NORM_MAX


def _check_param_shape(param, gate=None):
    """blocksparse/optimize.py:296-299: [blocks, bsize, bsize] with bsize 8 / 16 / 32 / 64, one gate per block -- on a ROCm device."""
    if torch is None:
        raise RuntimeError("blocksparse_amd needs PyTorch-ROCm for device memory")
    for t, what in ((param, "param"), (gate, "gate")):
        if t is not None and (not isinstance(t, torch.Tensor) or t.device.type != "cuda"):
            raise RuntimeError("blocksparse_amd: %s must be a tensor on a ROCm device (no CPU fallback)" % what)
    if param.dim() != 3 or param.shape[1] != param.shape[2] or param.shape[1] not in _BSIZES or param.shape[0] < 1:
        raise ValueError("param must be [blocks, bsize, bsize] with bsize in %s, got %s" % (_BSIZES, tuple(param.shape)))
    if not param.is_contiguous():
        raise ValueError("param must be contiguous")
    if gate is not None:
        if gate.dtype != torch.float32 or gate.numel() != param.shape[0] or not gate.is_contiguous() or gate.device != param.device:
            raise ValueError("gate: expected a contiguous float32 tensor with one entry per block (%d) on the param's device" % param.shape[0])


def blocksparse_norm(param, norm="max"):
    """fp32 [blocks]: max |w| (``norm="max"``) or sqrt(sum w^2) (``"l2"``) of every block (op BlocksparseNorm)."""
    _check_param_shape(param)
    out = torch.empty(param.shape[0], dtype=torch.float32, device=param.device)
    _lib.check(_lib.load().bsmm_block_norm(param.data_ptr(), out.data_ptr(), param.shape[0], param.shape[1], _dtype_code(param.dtype),
                                           _norm_code(norm), _lib.raw_stream(param.device)), "bsmm_block_norm")
    return out


def blocksparse_l2_decay(param, gate=None, rate=0.05, epsilon=1e-12):
    """In place: w_b -= w_b * min(rate / sqrt(sum w_b^2 + epsilon), 1); blocks whose gate is 0 are left alone.  Returns ``param``
    (op BlocksparseL2Decay)."""
    _check_param_shape(param, gate)
    _lib.check(_lib.load().bsmm_block_l2_decay(param.data_ptr(), gate.data_ptr() if gate is not None else None, float(rate), float(epsilon),
                                               param.shape[0], param.shape[1], _dtype_code(param.dtype), _lib.raw_stream(param.device)),
               "bsmm_block_l2_decay")
    _lib.wrote(param)
    return param


def prune_keep(blocks, sparsity):
    """How many blocks the sparsity path keeps: the reference's float32 arithmetic (src/optimize_op.cc:651-670)."""
    return int(np.float32(blocks) * (np.float32(1) - np.float32(sparsity)) + np.float32(0.5))


def blocksparse_prune(param, gate, step, sparsity=None, threshold=None, norm="max", frequency=1):
    """Update ``gate`` (fp32 [blocks], in place) from the block norms of ``param`` and return it.

    ``sparsity``: the ``prune_keep(blocks, sparsity)`` blocks of largest norm get gate 1, the others 0 (equal norms: the lower block id
    first).  ``threshold``: gate = 0 where norm < threshold, else 1 -- a block that was 0 can come back.  Exactly one of the two.  Acts only
    when ``frequency > 0 and (frequency == 1 or step % frequency == 0)`` (ops BlocksparsePrune / BlocksparseThresholdPrune)."""
    _check_param_shape(param, gate)
    if gate is None:
        raise ValueError("blocksparse_prune needs a gate")
    if (sparsity is None) == (threshold is None):
        raise ValueError("exactly one of sparsity / threshold must be set")
    code = _norm_code(norm)
    if not (frequency > 0 and (frequency == 1 or int(step) % int(frequency) == 0)):
        return gate
    lib = _lib.load()
    blocks = param.shape[0]
    st = _lib.raw_stream(param.device)
    if sparsity is not None:
        idx = torch.sort(blocksparse_norm(param, norm=norm), descending=True, stable=True).indices.to(torch.int32)
        keep = min(max(prune_keep(blocks, sparsity), 0), blocks)
        _lib.check(lib.bsmm_block_prune(gate.data_ptr(), idx.data_ptr(), blocks, keep, st), "bsmm_block_prune")
    else:
        _lib.check(lib.bsmm_block_threshold_prune(param.data_ptr(), gate.data_ptr(), float(threshold), code, blocks, param.shape[1],
                                                  _dtype_code(param.dtype), st), "bsmm_block_threshold_prune")
    _lib.wrote(gate)
    return gate


# ---- block-reduced full weight gradient ------------------------------------------------------------------------------------------
def reduced_dtype(dtype):
    """Type of the reduced activations: fp16 stays fp16, bf16 stays bf16, fp32 is reduced to bf16 (include/bsmm_sparsity.h)."""
    return torch.float16 if dtype == torch.float16 else torch.bfloat16


def feature_reduce(ts, bsize, axis, norm="max"):
    """Stage 1 (bsmm_feature_reduce) on 1..8 activation tensors of one shape and dtype: [feature blocks, len(ts), N], 16-bit."""
    ts = [t.contiguous() for t in ts]
    F, N = (ts[0].shape[0], ts[0].numel() // ts[0].shape[0]) if axis == 0 else (ts[0].shape[-1], ts[0].numel() // ts[0].shape[-1])
    out = torch.empty((F // bsize, len(ts), N), dtype=reduced_dtype(ts[0].dtype), device=ts[0].device)
    ptrs = (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    _lib.check(_lib.load().bsmm_feature_reduce(ptrs, len(ts), out.data_ptr(), F, N, bsize, axis, _dtype_code(ts[0].dtype), _norm_code(norm),
                                               _lib.raw_stream(ts[0].device)), "bsmm_feature_reduce")
    return out


def reduced_dw(bsmm, x_red, y_red, dw, scale, accumulate):
    """Stage 2 (bsmm_reduced_dw) into ``dw`` (fp32 [CB, KB])."""
    lib = _lib.load()
    CB, KB, Kc = x_red.shape[0], y_red.shape[0], x_red.shape[1] * x_red.shape[2]
    stream = _lib.raw_stream(dw.device)
    ws = bsmm._scratch(dw.device, stream, "reduced_dw", 0, int(lib.bsmm_reduced_dw_workspace_bytes(CB, KB, Kc)))
    _lib.check(lib.bsmm_reduced_dw(x_red.data_ptr(), y_red.data_ptr(), dw.data_ptr(), CB, KB, Kc, float(scale), 1 if accumulate else 0,
                                   _dtype_code(x_red.dtype), ws.data_ptr(), ws.numel(), stream), "bsmm_reduced_dw")
    return dw


def _check_pairs(bsmm, xs, dys):
    if isinstance(xs, torch.Tensor):
        xs, dys = [xs], [dys]
    xs, dys = list(xs), list(dys)
    if len(xs) != len(dys) or not xs:
        raise ValueError("need equally many (at least one) x and dy tensors")
    for t in xs + dys:
        bsmm._check_tensor(t, "x/dy")
        if t.dtype != xs[0].dtype or t.device != xs[0].device:
            raise TypeError("all x/dy tensors must share one dtype and device")
    N = bsmm._n_of(xs[0], bsmm.C)
    for x, dy in zip(xs, dys):
        if bsmm._n_of(x, bsmm.C) != N or bsmm._n_of(dy, bsmm.K) != N:
            raise ValueError("all pairs must share the minibatch size")
    return xs, dys, N


def _exact_twin(bsmm):
    """The same operator over the all-ones layout (every block of the dense grid present), made once."""
    twin = getattr(bsmm, "_dense_twin", None)
    if twin is None:
        from .matmul import BlocksparseMatMul
        twin = BlocksparseMatMul(np.ones((bsmm.CB, bsmm.KB), dtype=np.int32), block_size=bsmm.bsize, feature_axis=bsmm.axis, z_order=bsmm.z_order,
                                 name=bsmm.name + "/dense")
        twin._scatter_idx = {}
        bsmm._dense_twin = twin
    return twin


def _exact_norms(bsmm, xs, dys, norm):
    twin = _exact_twin(bsmm)
    total = None
    try:                                 # fp32 sums where the streaming weight-gradient kernel serves the configuration ...
        for i in range(0, len(xs), 8):
            sums = twin.updat(xs[i:i + 8], dys[i:i + 8], sums_only=True)
            total = sums.clone() if total is None else total.add_(sums)
    except _lib.BsmmError as e:          # ... else (BSMM_ERR_UNSUPPORTED, refused before any launch) the fp32 weight gradient of fp32 copies of the
        if e.code != _lib.ERR_UNSUPPORTED:   # activations: the norm of a gradient rounded to bf16 would be off by up to 2^-9 per block
            raise
        total = twin.updat_grouped([t.float() for t in xs], [t.float() for t in dys], group_size=8)
    norms = blocksparse_norm(total, norm=norm)
    key = (norms.device.type, norms.device.index)
    idx = twin._scatter_idx.get(key)
    if idx is None:
        idx = twin._scatter_idx[key] = torch.from_numpy(np.array([c * bsmm.KB + k for c, k in twin.updat_list], dtype=np.int64)).to(norms.device)
    return norms, idx


def block_reduced_full_dw(bsmm, xs, dys, scale=1.0, norm="max", dw_full=None, return_reduced=False, exact=False):
    """See ``BlocksparseMatMul.block_reduced_full_dw``."""
    xs, dys, N = _check_pairs(bsmm, xs, dys)
    _norm_code(norm)
    dev = xs[0].device
    if bsmm.axis == 0 and N % 8:
        raise ValueError("feature axis 0 needs a minibatch that is a multiple of 8")
    if dw_full is not None:
        bsmm._check_tensor(dw_full, "dw_full")
        if tuple(dw_full.shape) != (bsmm.CB, bsmm.KB) or dw_full.dtype != torch.float32 or not dw_full.is_contiguous() or dw_full.device != dev:
            raise ValueError("dw_full must be a contiguous float32 [%d, %d] tensor on the activations' device" % (bsmm.CB, bsmm.KB))
    if return_reduced and (len(xs) > 8 or exact):
        raise ValueError("return_reduced=True takes at most 8 pairs (and not exact=True)")
    if exact:
        if dw_full is None:
            dw_full = torch.zeros((bsmm.CB, bsmm.KB), dtype=torch.float32, device=dev)
        if float(scale) != 0.0:
            norms, idx = _exact_norms(bsmm, xs, dys, norm)
            dw_full.view(-1).index_add_(0, idx, norms, alpha=float(scale))
        return dw_full
    accumulate = dw_full is not None
    if dw_full is None:            # (scale == 0 launches nothing: the result is then the zeros it starts from)
        dw_full = (torch.zeros if float(scale) == 0.0 else torch.empty)((bsmm.CB, bsmm.KB), dtype=torch.float32, device=dev)
    x_red = y_red = None
    for i in range(0, len(xs), 8):
        x_red = feature_reduce(xs[i:i + 8], bsmm.bsize, bsmm.axis, norm)
        y_red = feature_reduce(dys[i:i + 8], bsmm.bsize, bsmm.axis, norm)
        reduced_dw(bsmm, x_red, y_red, dw_full, scale, accumulate)
        accumulate = True
    if return_reduced:
        if bsmm.axis == 1:         # the reference's axis-1 shape [pairs, N, feature blocks], as views of the [feature blocks, pairs, N] arrays
            x_red, y_red = x_red.permute(1, 2, 0), y_red.permute(1, 2, 0)
        return dw_full, x_red, y_red
    return dw_full


# ---- carrying weights over to another layout ------------------------------------------------------------------------------------------
def relayout_map(old_list, new_list):
    """(src, dst): block ``src[i]`` of the old layout is block ``dst[i]`` of the new one, for every (c, k) present in both
    (``old_list`` / ``new_list``: the two operators' ``updat_list``)."""
    where = {tuple(ck): w for w, ck in enumerate(old_list)}
    pairs = [(where[tuple(ck)], w) for w, ck in enumerate(new_list) if tuple(ck) in where]
    src = np.array([p[0] for p in pairs], dtype=np.int64)
    dst = np.array([p[1] for p in pairs], dtype=np.int64)
    return src, dst


def relayout(bsmm, param, new_layout, init=0.0):
    """See ``BlocksparseMatMul.relayout``."""
    from .matmul import BlocksparseMatMul
    new_layout = np.asarray(new_layout)
    if new_layout.shape != bsmm.layout.shape:
        raise ValueError("new_layout must have the shape of the old one %s" % (bsmm.layout.shape,))
    if tuple(param.shape) != bsmm.w_shape:
        raise ValueError("param must have shape %s" % (bsmm.w_shape,))
    new = BlocksparseMatMul(new_layout, block_size=bsmm.bsize, feature_axis=bsmm.axis, z_order=bsmm.z_order, name=bsmm.name,
                            segmented=bsmm.segmented, plan_options=bsmm.plan_options, updat_split=bsmm.updat_split)
    src, dst = relayout_map(bsmm.updat_list, new.updat_list)
    if torch is not None and isinstance(param, torch.Tensor):
        out = torch.full(new.w_shape, float(init), dtype=param.dtype, device=param.device)
        if len(src):
            out.index_copy_(0, torch.from_numpy(dst).to(param.device), param.index_select(0, torch.from_numpy(src).to(param.device)))
    else:
        param = np.asarray(param)
        out = np.full(new.w_shape, init, dtype=param.dtype)
        out[dst] = param[src]
    return new, out
