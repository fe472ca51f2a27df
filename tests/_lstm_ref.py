"""Float64 reference of the LSTM-gate tests (include/bsmm_lstm.h), independent of the package's NumPy functions.  c is (K, N) for axis 0 and
(N, K) for axis 1 (higher ranks as the operator flattens them); the fused gate tensor has 4K where c has K, in gate order i, u, f, o; the
bias has 4K elements in the same order."""
import numpy as np


def sigmoid(x):
    """1 / (1 + exp(-x)) without overflow: through exp(-|x|)."""
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _ax(c, axis):
    c = np.asarray(c)
    axis = axis + c.ndim if axis < 0 else axis
    assert axis in (0, c.ndim - 1)
    return axis


def split(h, axis):
    """The four gates of a fused tensor."""
    h = np.asarray(h)
    return tuple(np.split(h, 4, axis=_ax(h, axis)))


def fuse(parts, axis):
    return np.concatenate([np.asarray(p) for p in parts], axis=_ax(parts[0], axis))


def _pre(c, gates, bias, fb, axis):
    """float64 c and the four pre-activations (bias and forget bias added)."""
    c = np.asarray(c, dtype=np.float64)
    z = [np.asarray(g, dtype=np.float64) for g in gates]
    assert len(z) == 4 and all(g.shape == c.shape for g in z)
    if bias is not None:
        ax = _ax(c, axis)
        K = c.shape[ax]
        b = np.asarray(bias, dtype=np.float64).reshape(4, K)
        shape = tuple(K if d == ax else 1 for d in range(c.ndim))
        z = [g + b[q].reshape(shape) for q, g in enumerate(z)]
    z[2] = z[2] + float(fb)
    return c, z


def forward(c, gates, bias=None, fb=1.0, axis=-1):
    """(c_next, h_next) in float64; gates = (i, u, f, o), each like c."""
    c, (zi, zu, zf, zo) = _pre(c, gates, bias, fb, axis)
    cn = sigmoid(zf) * c + sigmoid(zi) * np.tanh(zu)
    return cn, sigmoid(zo) * np.tanh(cn)


def backward(c, gates, eh=None, ec=None, bias=None, fb=1.0, axis=-1):
    """(dc, (di, du, df, do), db) in float64; db [4K] is the sum of the unrounded gate gradients, None without a bias."""
    c, (zi, zu, zf, zo) = _pre(c, gates, bias, fb, axis)
    assert eh is not None or ec is not None
    eh = np.zeros_like(c) if eh is None else np.asarray(eh, dtype=np.float64)
    ec = np.zeros_like(c) if ec is None else np.asarray(ec, dtype=np.float64)
    si, tu, sf, so = sigmoid(zi), np.tanh(zu), sigmoid(zf), sigmoid(zo)
    ca = np.tanh(sf * c + si * tu)
    dC = eh * so * (1.0 - ca * ca) + ec
    d = (dC * tu * si * (1.0 - si), dC * si * (1.0 - tu * tu), dC * c * sf * (1.0 - sf), eh * ca * so * (1.0 - so))
    db = None
    if bias is not None:
        ax = _ax(c, axis)
        other = tuple(q for q in range(c.ndim) if q != ax)
        db = np.concatenate([g.sum(axis=other) for g in d])
    return dC * sf, d, db


# ---- inputs of the GPU tests ----------------------------------------------------------------------------------------------------------
def make_inputs(K, N, axis, dtype, seed, shape=None, std=1.0):
    """C, H (the fused gate tensor), EH, EC in the storage type's values and B fp32 [4K]: N(0, std) through fp16, then rounded to the storage
    type (as _ewops_ref.make_inputs draws them).  Read-only."""
    from oracle import bsmm_oracle as orc
    shape = tuple(shape or ((K, N) if axis == 0 else (N, K)))
    ax = 0 if axis == 0 else len(shape) - 1
    assert shape[ax] == K
    hshape = tuple(4 * K if d == ax else s for d, s in enumerate(shape))
    rng = np.random.RandomState(seed)
    f16 = lambda a: a.astype(np.float16).astype(np.float32)
    C = orc.round_to(f16(rng.normal(0.0, std, shape)), dtype)
    H = orc.round_to(f16(rng.normal(0.0, std, hshape)), dtype)
    EH = orc.round_to(f16(rng.normal(0.0, std, shape)), dtype)
    EC = orc.round_to(f16(rng.normal(0.0, std, shape)), dtype)
    B = f16(rng.normal(0.0, 1.0, 4 * K))
    for a in (C, H, EH, EC, B):
        a.setflags(write=False)
    return C, H, EH, EC, B
