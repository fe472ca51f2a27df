"""Float64 NumPy reference of the dynamic-sparsity operators (include/bsmm_sparsity.h, blocksparse_amd/sparsity.py): block norms, group
lasso decay, the two prune rules, the feature reduce and the block-reduced weight gradient.  Everything is computed in float64 and left
UNROUNDED unless a function says otherwise; storage rounding goes through oracle.bsmm_oracle.round_to."""
import numpy as np

from oracle import bsmm_oracle as orc

RED_DTYPE = {"f16": "f16", "bf16": "bf16", "f32": "bf16"}       # type of the reduced activations per activation type


def block_norm(w, norm):
    """[blocks]: max |w| or sqrt(sum w^2) per block."""
    w = np.asarray(w, dtype=np.float64).reshape(len(w), -1)
    return np.abs(w).max(axis=1) if norm == "max" else np.sqrt(np.square(w).sum(axis=1))


def l2_decay(w, gate=None, rate=0.05, epsilon=1e-12):
    """w_b - w_b * min(rate / sqrt(sum w_b^2 + epsilon), 1); blocks whose gate is 0 unchanged."""
    w = np.asarray(w, dtype=np.float64)
    ss = np.square(w.reshape(len(w), -1)).sum(axis=1)
    with np.errstate(divide="ignore"):
        decay = np.minimum(rate / np.sqrt(ss + epsilon), 1.0)
    out = w - w * decay[:, None, None]
    if gate is not None:
        off = np.asarray(gate) == 0
        out[off] = w[off]
    return out


def threshold_gate(norms, threshold):
    return np.where(np.asarray(norms) < threshold, 0.0, 1.0).astype(np.float32)


def keep_count(blocks, sparsity):
    return int(np.float32(blocks) * (np.float32(1) - np.float32(sparsity)) + np.float32(0.5))


def sparsity_gate(norms, sparsity):
    """1 for the keep_count blocks of largest norm (equal norms: the lower block id first), 0 for the others."""
    norms = np.asarray(norms)
    order = np.argsort(-norms, kind="stable")
    gate = np.zeros(len(norms), dtype=np.float32)
    gate[order[:keep_count(len(norms), sparsity)]] = 1.0
    return gate


def feature_reduce(ts, bsize, axis, norm):
    """[feature blocks, pairs, N] (the C ABI's layout for both axes), float64, unrounded."""
    outs = []
    for t in ts:
        t = np.asarray(t, dtype=np.float64)
        if axis == 0:
            b = t.reshape(t.shape[0] // bsize, bsize, -1)                     # [fb, i, n]
        else:
            b = t.reshape(-1, t.shape[-1] // bsize, bsize).transpose(1, 2, 0)   # [fb, i, n]
        outs.append(np.abs(b).max(axis=1) if norm == "max" else np.sqrt(np.square(b).sum(axis=1)))
    return np.stack(outs, axis=1)


def reduced_dw(x_red, y_red, scale=1.0, dw_full=None):
    """scale * x_red . y_red^T over (pair, n) [+ dw_full], from reduced arrays in the C ABI's layout."""
    x = np.asarray(x_red, dtype=np.float64).reshape(len(x_red), -1)
    y = np.asarray(y_red, dtype=np.float64).reshape(len(y_red), -1)
    dw = scale * (x @ y.T)
    return dw if dw_full is None else dw + np.asarray(dw_full, dtype=np.float64)


def block_reduced_full_dw(xs, dys, bsize, axis, norm, dtype, scale=1.0, dw_full=None):
    """The whole operator on host arrays of storage-type values: the reduced arrays are rounded once to their 16-bit type, as on the device."""
    rd = RED_DTYPE[dtype]
    xr = orc.round_to(feature_reduce(xs, bsize, axis, norm), rd)
    yr = orc.round_to(feature_reduce(dys, bsize, axis, norm), rd)
    return reduced_dw(xr, yr, scale, dw_full)


def dense_dw(xs, dys, axis):
    """sum over the pairs of the dense weight gradient [C, K], float64."""
    tot = 0.0
    for x, dy in zip(xs, dys):
        x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
        tot = tot + (x @ dy.T if axis == 0 else x.reshape(-1, x.shape[-1]).T @ dy.reshape(-1, dy.shape[-1]))
    return tot


def dense_block_norms(dw, bsize, norm):
    """[CB, KB] norms of the bsize x bsize blocks of a dense [C, K] matrix."""
    C, K = dw.shape
    b = dw.reshape(C // bsize, bsize, K // bsize, bsize).transpose(0, 2, 1, 3).reshape(C // bsize, K // bsize, -1)
    return np.abs(b).max(axis=2) if norm == "max" else np.sqrt(np.square(b).sum(axis=2))


def relayout(param, old_list, new_list, init=0.0):
    param = np.asarray(param)
    where = {tuple(ck): w for w, ck in enumerate(old_list)}
    out = np.full((len(new_list),) + param.shape[1:], init, dtype=param.dtype)
    for w, ck in enumerate(new_list):
        if tuple(ck) in where:
            out[w] = param[where[tuple(ck)]]
    return out
