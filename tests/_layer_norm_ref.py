"""Float64 reference of the layer norm tests (include/bsmm_norm.h): forward, statistics and the three gradients, vectorised over segments
and independent of the package's NumPy functions.  x is (K, N) for axis 0 and (N, K) for axis 1 (higher ranks are flattened the way the
operator flattens them); g, b have K elements; mean / rstd come back as [S, N]."""
import numpy as np


def _view(a, K, axis, S):
    """axis 0: (S, Ks, N), features on dim 1;  axis 1: (S, Ks, N) too, by moving (N, S, Ks) around -- one layout for all the formulas."""
    a = np.asarray(a, dtype=np.float64)
    if axis == 0:
        return a.reshape(S, K // S, -1)
    return a.reshape(-1, S, K // S).transpose(1, 2, 0)


def _unview(a, shape, axis):
    return (a.reshape(shape) if axis == 0 else a.transpose(2, 0, 1).reshape(shape))


def _axis01(x, axis):
    x = np.asarray(x)
    axis = axis + x.ndim if axis < 0 else axis
    assert axis in (0, x.ndim - 1)
    return (0 if axis == 0 else 1), x.shape[axis]


def stats(x, axis=1, segments=1, epsilon=1e-6):
    """(mean, rstd), each [S, N], biased variance as the mean of squared deviations."""
    ax, K = _axis01(x, axis)
    xs = _view(x, K, ax, segments)
    mean = xs.mean(axis=1)
    var = ((xs - mean[:, None, :]) ** 2).mean(axis=1)
    return mean, 1.0 / np.sqrt(var + epsilon)


def pre_activation(x, g, b, axis=1, segments=1, epsilon=1e-6):
    """xhat * g + b in the shape of x (what ReLU is applied to and what masks dy)."""
    ax, K = _axis01(x, axis)
    xs = _view(x, K, ax, segments)
    mean, rstd = stats(x, axis, segments, epsilon)
    gs = np.asarray(g, dtype=np.float64).reshape(segments, K // segments, 1)
    bs = np.asarray(b, dtype=np.float64).reshape(segments, K // segments, 1)
    return _unview((xs - mean[:, None, :]) * rstd[:, None, :] * gs + bs, np.asarray(x).shape, ax)


def forward(x, g, b, axis=1, segments=1, epsilon=1e-6, relu=False):
    y = pre_activation(x, g, b, axis, segments, epsilon)
    return np.maximum(y, 0.0) if relu else y


def backward(dy, x, g, b, axis=1, segments=1, epsilon=1e-6, relu=False):
    """(dx like x, dg [K], db [K])."""
    ax, K = _axis01(x, axis)
    Ks = K // segments
    xs, dys = _view(x, K, ax, segments), _view(dy, K, ax, segments)
    mean, rstd = stats(x, axis, segments, epsilon)
    gs = np.asarray(g, dtype=np.float64).reshape(segments, Ks, 1)
    bs = np.asarray(b, dtype=np.float64).reshape(segments, Ks, 1)
    xhat = (xs - mean[:, None, :]) * rstd[:, None, :]
    if relu:
        dys = np.where(xhat * gs + bs > 0.0, dys, 0.0)
    dg = (dys * xhat).sum(axis=2).reshape(K)
    db = dys.sum(axis=2).reshape(K)
    dyg = dys * gs
    sum1 = (xhat * dyg).sum(axis=1, keepdims=True)
    sum2 = dyg.sum(axis=1, keepdims=True)
    dx = (dyg - (xhat * sum1 + sum2) / Ks) * rstd[:, None, :]
    return _unview(dx, np.asarray(x).shape, ax), dg, db
