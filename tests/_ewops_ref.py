"""Float64 reference of the ewops tests (include/bsmm_ew.h) and a NumPy Philox4x32-10 of its own, independent of the package's NumPy
functions.  x is (K, N) for axis 0 and (N, K) for axis 1 (higher ranks as the operator flattens them); b has K elements; a mask is the packed
int32 / uint32 words, bit i % 32 of word i / 32 = element i of the flattened tensor."""
import numpy as np

ALPHA = 1.702
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = 0xFFFFFFFF


def philox(counter, key):
    """One Philox4x32-10 call on Python integers: counter = 4 words, key = 2 words -> 4 words."""
    c0, c1, c2, c3 = (int(v) & U32 for v in counter)
    k0, k1 = (int(v) & U32 for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & U32, (p0 >> 32) ^ c3 ^ k1, p0 & U32
        k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
    return c0, c1, c2, c3


def philox_np(c_lo, c_hi, o_lo, o_hi, k0, k1):
    """The same on uint64 arrays of calls (the products of two 32-bit values fit 64 bits)."""
    c = [np.asarray(c_lo, dtype=np.uint64), np.asarray(c_hi, dtype=np.uint64), np.full_like(np.asarray(c_lo, dtype=np.uint64), o_lo),
         np.full_like(np.asarray(c_lo, dtype=np.uint64), o_hi)]
    lo, sh = np.uint64(U32), np.uint64(32)
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> sh) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
    return c


def threshold_of(keep_prob):
    return int(round(float(keep_prob) * 65536.0))


def scale_of(keep_prob):
    return float(np.float32(1.0 / float(keep_prob)))


def keep_bits(n, seed, offset, threshold):
    """bool [n]: element i belongs to call i // 8 and takes the 16 bits (w[(i % 8) // 2] >> 16 (i % 2)) & 0xffff; kept iff below threshold."""
    seed, offset = int(seed) % 2 ** 64, int(offset) % 2 ** 64
    calls = np.arange((n + 7) // 8, dtype=np.uint64)
    w = philox_np(calls & np.uint64(U32), calls >> np.uint64(32), offset & U32, offset >> 32, seed & U32, seed >> 32)
    halves = np.stack([w[0] & np.uint64(0xFFFF), w[0] >> np.uint64(16), w[1] & np.uint64(0xFFFF), w[1] >> np.uint64(16),
                       w[2] & np.uint64(0xFFFF), w[2] >> np.uint64(16), w[3] & np.uint64(0xFFFF), w[3] >> np.uint64(16)], axis=1)
    return halves.reshape(-1)[:n] < np.uint64(threshold)


def keep_bit_loop(i, seed, offset, threshold):
    """The definition for ONE element, on Python integers."""
    seed, offset = int(seed) % 2 ** 64, int(offset) % 2 ** 64
    c = i // 8
    w = philox((c & U32, c >> 32, offset & U32, offset >> 32), (seed & U32, seed >> 32))
    return ((w[(i % 8) // 2] >> (16 * (i % 2))) & 0xFFFF) < threshold


def pack(bits):
    """uint32 [ceil(n / 32)], pad bits zero."""
    bits = np.asarray(bits, dtype=bool).reshape(-1)
    words = np.zeros((bits.size + 31) // 32, dtype=np.uint32)
    for i in np.nonzero(bits)[0]:
        words[i // 32] |= np.uint32(1 << (i % 32))
    return words


def pack_fast(bits):
    bits = np.asarray(bits, dtype=bool).reshape(-1)
    padded = np.zeros((bits.size + 31) // 32 * 32, dtype=np.uint64)
    padded[:bits.size] = bits
    return (padded.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def mask_words(n, seed, offset, keep_prob):
    return pack_fast(keep_bits(n, seed, offset, threshold_of(keep_prob)))


def as_u32(mask):
    """A device mask (int32 tensor or array) as uint32 words."""
    a = mask.detach().cpu().numpy() if hasattr(mask, "detach") else np.asarray(mask)
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1)


def unpack(words, n):
    words = np.asarray(words, dtype=np.uint32).astype(np.uint64)
    return (((words[:, None] >> np.arange(32, dtype=np.uint64)) & np.uint64(1)).reshape(-1)[:n]).astype(bool)


def _axis01(x, axis):
    x = np.asarray(x)
    axis = axis + x.ndim if axis < 0 else axis
    assert axis in (0, x.ndim - 1)
    return 0 if axis == 0 else 1


def _bias(x, b, axis):
    x = np.asarray(x)
    b = np.asarray(b, dtype=np.float64).reshape(-1)
    return b.reshape((-1,) + (1,) * (x.ndim - 1)) if _axis01(x, axis) == 0 else b


def pre_activation(x, b, axis):
    return np.asarray(x, dtype=np.float64) + _bias(x, b, axis)


def sigmoid(z):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-ALPHA * z))


def act(z, a):
    return z if a == 0 else (np.maximum(z, 0.0) if a == 1 else z * sigmoid(z))


def act_grad(z, a):
    if a == 0:
        return np.ones_like(z)
    if a == 1:
        return (z > 0.0).astype(np.float64)
    s = sigmoid(z)
    return s + ALPHA * z * s * (1.0 - s)


def _db(dx, axis):
    ax = _axis01(dx, axis)
    return dx.reshape(dx.shape[0], -1).sum(axis=1) if ax == 0 else dx.reshape(-1, dx.shape[-1]).sum(axis=0)


def forward(x, b, axis, a=0, kept=None, scale=1.0, residual=None):
    """act(x + b), then kept ? * scale : 0, then + residual; kept: bool like x (flattened order) or None."""
    v = act(pre_activation(x, b, axis), a)
    if kept is not None:
        v = np.where(np.asarray(kept).reshape(v.shape), v * float(scale), 0.0)
    if residual is not None:
        v = v + np.asarray(residual, dtype=np.float64)
    return v


def backward(dy, x, b, axis, a=0, kept=None, scale=1.0):
    """(dx like x, db [K])."""
    g = np.asarray(dy, dtype=np.float64)
    if kept is not None:
        g = np.where(np.asarray(kept).reshape(g.shape), g * float(scale), 0.0)
    dx = g * act_grad(pre_activation(x, b, axis), a)
    return dx, _db(dx, axis)


# ---- inputs of the GPU tests ----------------------------------------------------------------------------------------------------------
def make_inputs(K, N, axis, dtype, grid, seed, shape=None):
    """X, E (gradient of y), R (residual) in the storage type's values, B fp32.  grid: x on multiples of 1/16 in [-4, 4) (exact in bf16) and b
    on multiples of 1/16 plus 1/32, so that every z = x + b is an odd multiple of 1/32: a ReLU mask is decided far from any rounding, with
    no element excluded.  Otherwise N(0, 1) through fp16."""
    from oracle import bsmm_oracle as orc
    shape = shape or ((K, N) if axis == 0 else (N, K))
    rng = np.random.RandomState(seed)
    f16 = lambda a: a.astype(np.float16).astype(np.float32)
    if grid:
        X = (rng.randint(-64, 64, size=shape) / 16.0).astype(np.float32)
        B = (rng.randint(-16, 16, size=K) / 16.0 + 1.0 / 32.0).astype(np.float32)
        assert np.array_equal(orc.round_to(X, dtype), X)
    else:
        X = orc.round_to(f16(rng.normal(0.0, 1.0, shape)), dtype)
        B = f16(rng.normal(0.0, 1.0, K))
    E = orc.round_to(f16(rng.normal(0.0, 1.0, shape)), dtype)
    R = orc.round_to(f16(rng.normal(0.0, 1.0, shape)), dtype)
    for a in (X, E, R, B):
        a.setflags(write=False)
    return X, E, R, B
