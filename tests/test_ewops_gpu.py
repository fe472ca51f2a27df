"""GPU tier of the layer epilogue (include/bsmm_ew.h through blocksparse_amd/ewops.py) against the float64 helper tests/_ewops_ref.py on
inputs pre-rounded to the storage type: y and dx at the bars of their dtype (tests/_parity.py), db -- fp32 in every dtype -- at the fp32
bars, masks bit for bit against the NumPy Philox, the fp32 fused launches bit for bit against the composed sequence.  Each shape is the
smallest that reaches a distinct code path (see PATHS).  ReLU cases use inputs whose every pre-activation is an odd multiple of 1/32
(asserted, no element excluded)."""
import numpy as np
import pytest

import _ewops_ref as ER
import _parity as P
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f16", "bf16")
ACTS = (0, 1, 2)
ACT_KW = {0: {}, 1: dict(relu=True), 2: dict(fast_gelu=True)}
SEED = (1 << 40) + 12345
KEEP = 0.8
# (K, N, axis): what the case is there for.  A group is 8 consecutive elements; a forward workgroup takes 256 groups; an axis-0 backward
# workgroup sweeps 8192 columns of one row; an axis-1 backward lane owns 8 columns (16-byte path) or one.
PATHS = [
    (1, 1, 0), (1, 1, 1), (32, 32, 0), (32, 32, 1),    # the reference test's shapes
    (31, 5, 0), (5, 31, 1),                              # element path: groups cross rows, a ragged last group, pad bytes of the last mask word
    (96, 40, 0), (40, 96, 1),                            # 16-byte path
    (40, 1043, 0),                                       # ragged strips: several workgroups forward, rows that start at any bit of a mask word
    (1043, 36, 1),                                       # rows not 16-byte aligned (16-bit), four column tiles backward (element path)
    (8, 3001, 1),                                        # many rows, few features: 256 lanes share one column unit, row-group partials of db
    (2056, 3, 1),                                        # wide rows: two column tiles on the 16-byte path
    (3, 8193, 0),                                        # N one past what a workgroup sweeps: the row cut over workgroups, element path
    (3, 8200, 0),                                        # the same on the 16-byte path
    (2049, 8, 0),                                        # more rows than the backward grid has workgroups: the grid stride
]
IDS = ["K%d-N%d-a%d" % c for c in PATHS]
SMALL = [(31, 5, 0), (5, 31, 1), (96, 40, 0), (40, 96, 1), (40, 1043, 0), (1043, 36, 1), (8, 3001, 1), (3, 8200, 0)]
SMALL_IDS = ["K%d-N%d-a%d" % c for c in SMALL]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from blocksparse_amd import ewops
    return torch, ewops


_cache = {}


def make_case(K, N, axis, dtype, grid=True, shape=None):
    """Seeded inputs and, lazily, float64 results: computed once per case and shared, never modified."""
    key = (K, N, axis, dtype, grid, shape)
    if key not in _cache:
        X, E, R, B = ER.make_inputs(K, N, axis, dtype, grid, 1000 * K + 10 * N + axis, shape)
        _cache[key] = dict(X=X, E=E, R=R, B=B, ref={})
    return _cache[key]


def reference(c, axis, a, kept_key=None, kept=None, scale=1.0, residual=False):
    key = (a, kept_key, residual)
    if key not in c["ref"]:
        ax = 0 if axis == 0 else -1
        y = ER.forward(c["X"], c["B"], ax, a, kept, scale, c["R"] if residual else None)
        dx, db = ER.backward(c["E"], c["X"], c["B"], ax, a, kept, scale)
        c["ref"][key] = (y, dx, db)
    return c["ref"][key]


def at_offset(torch, a, dtype, off_bytes=0):
    """The array on the device in its storage type, its first element ``off_bytes`` past an allocation boundary (still contiguous)."""
    t = P.to_dev(a, dtype, torch)
    if not off_bytes:
        return t
    e = off_bytes // t.element_size()
    buf = torch.empty(t.numel() + e, dtype=t.dtype, device=t.device)
    v = buf[e:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == off_bytes
    return v


def f32dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")


def check(name, got, want64, dtype, ctx):
    want = orc.round_to(np.asarray(want64), dtype) if dtype != "f32" else np.asarray(want64)
    got = P.to_host(got)
    assert got.shape == want.shape, (ctx, name, got.shape, want.shape)
    assert np.isfinite(got).all(), (ctx, name)
    l2, mx = P.errors(got, want)
    print(ctx, name, "l2 %.3g max %.3g" % (l2, mx))
    assert l2 <= P.L2_BAR[dtype] and mx <= P.MAX_BAR[dtype], (ctx, name, l2, mx)


def bits_equal(torch, a, b):
    """Bit for bit (a -0 is not a +0)."""
    iv = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


@pytest.mark.parametrize("a", ACTS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", PATHS, ids=IDS)
def test_bias_act_against_float64(env, case, dtype, a):
    torch, ewops = env
    K, N, axis = case
    c = make_case(K, N, axis, dtype)
    z = ER.pre_activation(c["X"], c["B"], axis)
    assert np.abs(z).min() >= 1.0 / 32.0                 # every ReLU mask is decided far from rounding: no element is excluded
    if a == 1 and K * N > 1:
        assert (z > 0).any() and (z < 0).any()
    wy, wdx, wdb = reference(c, axis, a)
    x, dy, b = P.to_dev(c["X"], dtype, torch), P.to_dev(c["E"], dtype, torch), f32dev(torch, c["B"])
    y = ewops.bias_relu_fwd(x, b, axis=axis, **ACT_KW[a])
    dx, db = ewops.bias_relu_bwd(dy, {0: None, 1: y, 2: x}[a], b, axis=axis, **ACT_KW[a])
    assert y.dtype == x.dtype and y.shape == x.shape and dx.dtype == x.dtype and dx.shape == x.shape
    assert db.dtype == torch.float32 and db.shape == b.shape
    if a == 0:
        assert dx is dy
    check("y", y, wy, dtype, (case, dtype, a))
    check("dx", dx, wdx, dtype, (case, dtype, a))
    check("db", db, wdb, "f32", (case, dtype, a))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(96, 40, 0), (40, 1043, 0), (1043, 36, 1), (2056, 3, 1)], ids=["K96-N40-a0", "K40-N1043-a0", "K1043-N36-a1", "K2056-N3-a1"])
def test_fast_gelu_on_random_inputs(env, case, dtype):
    """N(0, 1) inputs (the grid of the other tests has 128 values of x): the exponential and the division at the fp32 bars."""
    torch, ewops = env
    K, N, axis = case
    c = make_case(K, N, axis, dtype, grid=False)
    wy, wdx, wdb = reference(c, axis, 2)
    x, dy, b = P.to_dev(c["X"], dtype, torch), P.to_dev(c["E"], dtype, torch), f32dev(torch, c["B"])
    y = ewops.bias_relu_fwd(x, b, axis=axis, fast_gelu=True)
    dx, db = ewops.bias_relu_bwd(dy, x, b, axis=axis, fast_gelu=True)
    check("y", y, wy, dtype, (case, dtype))
    check("dx", dx, wdx, dtype, (case, dtype))
    check("db", db, wdb, "f32", (case, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fast_gelu_saturates_to_finite_values(env, dtype):
    torch, ewops = env
    Z = np.array([[-100.0, 100.0, -30.0, 30.0, -100.0, 100.0, -30.0, 30.0, 0.0]], dtype=np.float32)      # (1, 9): axis 0, element path
    E = np.full_like(Z, 1.5)
    for X, B in ((Z, np.zeros(1, dtype=np.float32)), (Z - 2.0, np.full(1, 2.0, dtype=np.float32))):      # z reached without and with a bias
        x, dy, b = P.to_dev(X, dtype, torch), P.to_dev(E, dtype, torch), f32dev(torch, B)
        y = ewops.bias_relu_fwd(x, b, axis=0, fast_gelu=True)
        dx, db = ewops.bias_relu_bwd(dy, x, b, axis=0, fast_gelu=True)
        assert torch.isfinite(y.float()).all() and torch.isfinite(dx.float()).all() and torch.isfinite(db).all()
        check("y", y, ER.forward(X, B, 0, 2), dtype, dtype)
        wdx, wdb = ER.backward(E, X, B, 0, 2)
        check("dx", dx, wdx, dtype, dtype)
        check("db", db, wdb, "f32", dtype)
        yh, dxh = P.to_host(y)[0], P.to_host(dx)[0]
        assert (yh[[0, 4]] == 0).all() and (yh[[1, 5]] == 100.0).all() and (dxh[[0, 4]] == 0).all() and (dxh[[1, 5]] == 1.5).all()
    y = ewops.fast_gelu(P.to_dev(Z.reshape(3, 3), dtype, torch))
    check("fast_gelu", y, ER.forward(Z.reshape(3, 3), np.zeros(3), -1, 2), dtype, dtype)


@pytest.mark.parametrize("n", [1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 511, 512, 513, 8192, 8193])
def test_mask_kernel_bit_for_bit(env, n):
    """8193: one element past what a workgroup of the mask kernel makes (256 words)."""
    torch, ewops = env
    for offset, kp in ((0, KEEP), ((1 << 33) + 5, 0.5), (2, 1.0)):
        st = ewops.set_entropy(SEED, offset=offset)
        mask = ewops.dropout_mask(n, kp)
        assert mask.dtype == torch.int32 and mask.shape == ((n + 31) // 32,)
        assert np.array_equal(ER.as_u32(mask), ER.mask_words(n, SEED, offset, kp)), (n, offset, kp)       # every word, pad bits included
        assert np.array_equal(ER.as_u32(mask), ewops.dropout_mask_test(n, SEED, offset, kp).view(np.uint32))
        assert st.tolist() == [SEED, offset + 1] and ewops.entropy_state() is st


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", PATHS, ids=IDS)
def test_fused_against_float64_and_its_mask_bit_for_bit(env, case, dtype):
    """The fused forward with generate = 1 and the fused backward, activations aligned and 2 / 4 bytes off: the mask is the NumPy one whatever
    the dtype, the axis and the kernel, y / dx / db follow the float64 helper under that mask."""
    torch, ewops = env
    K, N, axis = case
    c = make_case(K, N, axis, dtype)
    total = K * N
    a = (K + N + axis) % 3
    offset = 7 + axis
    want_mask = ER.mask_words(total, SEED, offset, KEEP)
    kept = ER.unpack(want_mask, total)
    wy, wdx, wdb = reference(c, axis, a, ("fused", offset), kept, ER.scale_of(KEEP), residual=True)
    b = f32dev(torch, c["B"])
    for off in ((0, 4) if dtype == "f32" else (0, 2, 4)):
        x, dy, r = (at_offset(torch, c[n], dtype, off) for n in ("X", "E", "R"))
        ewops.set_entropy(SEED, offset=offset)
        y, mask = ewops.bias_dropout_fwd(x, b, KEEP, axis=axis, residual=r, **ACT_KW[a])
        assert np.array_equal(ER.as_u32(mask), want_mask), (case, dtype, off)
        assert ewops.entropy_state().tolist() == [SEED, offset + 1]
        dx, db = ewops.bias_dropout_bwd(dy, x, b, mask, KEEP, axis=axis, **ACT_KW[a])
        check("y", y, wy, dtype, (case, dtype, off, a))
        check("dx", dx, wdx, dtype, (case, dtype, off, a))
        check("db", db, wdb, "f32", (case, dtype, off, a))
    # without a residual, and the dropout alone (no bias): the same mask again
    ewops.set_entropy(SEED, offset=offset)
    y, mask = ewops.bias_dropout_fwd(x, b, KEEP, axis=axis, **ACT_KW[a])
    assert np.array_equal(ER.as_u32(mask), want_mask)
    check("y-no-residual", y, ER.forward(c["X"], c["B"], axis, a, kept, ER.scale_of(KEEP)), dtype, (case, dtype, a))
    ewops.set_entropy(SEED, offset=offset)
    y, mask = ewops.dropout(x, KEEP)
    assert np.array_equal(ER.as_u32(mask), want_mask)
    check("dropout", y, np.where(kept.reshape(c["X"].shape), c["X"].astype(np.float64) * ER.scale_of(KEEP), 0.0), dtype, (case, dtype))
    check("apply", ewops.apply_dropout_mask(dy, mask, KEEP), np.where(kept.reshape(c["E"].shape), c["E"].astype(np.float64) * ER.scale_of(KEEP), 0.0),
          dtype, (case, dtype))


@pytest.mark.parametrize("a", ACTS)
@pytest.mark.parametrize("case", PATHS, ids=IDS)
def test_fp32_fused_equals_the_composed_sequence_bit_for_bit(env, case, a):
    torch, ewops = env
    K, N, axis = case
    c = make_case(K, N, axis, "f32", grid=(a == 1))
    x, dy, r, b = (f32dev(torch, c[n]) for n in ("X", "E", "R", "B"))
    ewops.set_entropy(SEED, offset=11)
    mask = ewops.dropout_mask(K * N, KEEP)
    # forward: bias_relu -> dropout -> torch add
    y1 = ewops.bias_relu_fwd(x, b, axis=axis, **ACT_KW[a])
    y2 = ewops.apply_dropout_mask(y1, mask, KEEP)
    composed = y2 + r
    fused, same = ewops.bias_dropout_fwd(x, b, KEEP, axis=axis, residual=r, mask=mask, **ACT_KW[a])
    assert same is mask
    assert bits_equal(torch, fused, composed), (case, a)
    # backward, its mirror: the residual's gradient is dy; dropout on dy; then the bias / activation gradient
    g = ewops.apply_dropout_mask(dy, mask, KEEP)
    cdx, cdb = ewops.bias_relu_bwd(g, {0: None, 1: y1, 2: x}[a], b, axis=axis, **ACT_KW[a])
    fdx, fdb = ewops.bias_dropout_bwd(dy, x, b, mask, KEEP, axis=axis, **ACT_KW[a])
    assert bits_equal(torch, fdx, cdx), (case, a)
    assert bits_equal(torch, fdb, cdb), (case, a)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_recompute_with_the_returned_mask_gives_the_same_bits(env, case, dtype):
    torch, ewops = env
    K, N, axis = case
    c = make_case(K, N, axis, dtype)
    x, r, b = P.to_dev(c["X"], dtype, torch), P.to_dev(c["R"], dtype, torch), f32dev(torch, c["B"])
    ewops.set_entropy(SEED, offset=3)
    y, mask = ewops.bias_dropout_fwd(x, b, KEEP, axis=axis, fast_gelu=True, residual=r)
    kept_words = mask.clone()
    y2, mask2 = ewops.bias_dropout_fwd(x, b, KEEP, axis=axis, fast_gelu=True, residual=r, mask=mask)
    assert mask2 is mask and torch.equal(mask, kept_words)                    # read, not written
    assert bits_equal(torch, y, y2), (case, dtype)
    assert ewops.entropy_state().tolist() == [SEED, 4]                          # the recompute draws nothing


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", SMALL + [(3, 8193, 0)], ids=SMALL_IDS + ["K3-N8193-a0"])
def test_backward_twice_gives_the_same_bits(env, case, dtype):
    torch, ewops = env
    K, N, axis = case
    c = make_case(K, N, axis, dtype)
    x, dy, b = P.to_dev(c["X"], dtype, torch), P.to_dev(c["E"], dtype, torch), f32dev(torch, c["B"])
    ewops.set_entropy(SEED, offset=5)
    mask = ewops.dropout_mask(K * N, KEEP)
    first = ewops.bias_dropout_bwd(dy, x, b, mask, KEEP, axis=axis, fast_gelu=True) + ewops.bias_relu_bwd(dy, x, b, axis=axis, fast_gelu=True)
    torch.empty(1 << 20, device="cuda").fill_(float("nan"))       # (another workspace block for the second call, with other contents)
    second = ewops.bias_dropout_bwd(dy, x, b, mask, KEEP, axis=axis, fast_gelu=True) + ewops.bias_relu_bwd(dy, x, b, axis=axis, fast_gelu=True)
    for f, s, name in zip(first, second, ("dx", "db", "dx-plain", "db-plain")):
        assert bits_equal(torch, f, s), (case, dtype, name)


@pytest.mark.parametrize("axis", (0, -1))
def test_autograd_gives_the_low_level_gradients(env, axis):
    """All three functions, on a rank-3 input: (24, 3, 8) features first, (3, 5, 40) features last."""
    torch, ewops = env
    from blocksparse_amd import bias_dropout, bias_relu, dropout
    shape = (24, 3, 8) if axis == 0 else (3, 5, 40)
    K = shape[axis]
    c = make_case(K, int(np.prod(shape)) // K, axis, "bf16", shape=shape)
    x, dy, r = (P.to_dev(c[n], "bf16", torch) for n in ("X", "E", "R"))
    b = f32dev(torch, c["B"]).view(2, K // 2)            # (the gradient comes back in the shape of b)
    for a in ACTS:
        xr, br = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y = bias_relu(xr, br, axis=axis, **ACT_KW[a])
        got = torch.autograd.grad(y, (xr, br), dy)
        y2 = ewops.bias_relu_fwd(x, b, axis=axis, **ACT_KW[a])
        want = ewops.bias_relu_bwd(dy, {0: None, 1: y2, 2: x}[a], b, axis=axis, **ACT_KW[a])
        assert bits_equal(torch, y.detach(), y2)
        for g, w, name in zip(got, want, ("dx", "db")):
            assert bits_equal(torch, g, w), (axis, a, name)
        assert got[0].dtype == torch.bfloat16 and got[1].dtype == torch.float32 and got[1].shape == b.shape
        check("y", y2, ER.forward(c["X"], c["B"], axis, a), "bf16", (axis, a))
        # the fused pair, with a residual
        xr, br, rr = x.clone().requires_grad_(True), b.clone().requires_grad_(True), r.clone().requires_grad_(True)
        ewops.set_entropy(SEED, offset=21)
        y, mask = bias_dropout(xr, br, KEEP, axis=axis, residual=rr, **ACT_KW[a])
        assert not mask.requires_grad and np.array_equal(ER.as_u32(mask), ER.mask_words(x.numel(), SEED, 21, KEEP))
        got = torch.autograd.grad(y, (xr, br, rr), dy)
        y2, _ = ewops.bias_dropout_fwd(x, b, KEEP, axis=axis, residual=r, mask=mask, **ACT_KW[a])
        want = ewops.bias_dropout_bwd(dy, x, b, mask, KEEP, axis=axis, **ACT_KW[a]) + (dy,)
        assert bits_equal(torch, y.detach(), y2)
        for g, w, name in zip(got, want, ("dx", "db", "dresidual")):
            assert bits_equal(torch, g, w), (axis, a, name)
    xr = x.clone().requires_grad_(True)
    ewops.set_entropy(SEED, offset=22)
    y, mask = dropout(xr, KEEP)
    (got,) = torch.autograd.grad(y, (xr,), dy)
    assert bits_equal(torch, got, ewops.apply_dropout_mask(dy, mask, KEEP)) and bits_equal(torch, y.detach(), ewops.apply_dropout_mask(x, mask, KEEP))
    y3, mask3 = dropout(xr, KEEP, mask=mask)                                  # a given mask is applied as it is
    assert bits_equal(torch, y3.detach(), y.detach()) and torch.equal(mask3, mask)


@pytest.mark.parametrize("axis", (0, 1))
def test_captured_step_draws_a_fresh_mask_on_every_replay(env, axis):
    torch, ewops = env
    K, N, o = 96, 40, 100
    c = make_case(K, N, axis, "bf16")
    x, dy, r = (P.to_dev(c[n], "bf16", torch) for n in ("X", "E", "R"))
    b = f32dev(torch, c["B"])

    def step():
        y, mask = ewops.bias_dropout_fwd(x, b, KEEP, axis=axis, fast_gelu=True, residual=r)
        return (y, mask) + tuple(ewops.bias_dropout_bwd(dy, x, b, mask, KEEP, axis=axis, fast_gelu=True))

    st = ewops.set_entropy(SEED, offset=o)
    step()
    torch.cuda.synchronize()
    ewops.set_entropy(SEED, offset=o)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    torch.cuda.synchronize()
    assert st.tolist() == [SEED, o]                                           # capturing ran nothing
    seen = []
    for i in range(2):
        graph.replay()
        torch.cuda.synchronize()
        seen.append([t.clone() for t in outs])
    assert st.tolist() == [SEED, o + 2] and ewops.entropy_state() is st
    assert not torch.equal(seen[0][1], seen[1][1])
    for i in range(2):
        want_mask = ER.mask_words(K * N, SEED, o + i, KEEP)
        assert np.array_equal(ER.as_u32(seen[i][1]), want_mask), (axis, i)
        kept = ER.unpack(want_mask, K * N)
        wy, wdx, wdb = reference(c, axis, 2, ("capture", o + i), kept, ER.scale_of(KEEP), residual=True)
        check("y", seen[i][0], wy, "bf16", (axis, i))
        check("dx", seen[i][2], wdx, "bf16", (axis, i))
        check("db", seen[i][3], wdb, "f32", (axis, i))


def test_sizes_beyond_the_grid(env):
    """More work than 2048 workgroups take in one pass.  Forward: 2049 workgroups' worth of groups, 16-byte path.  Axis-1 backward: three
    column tiles times 1024 row partitions, element path."""
    torch, ewops = env
    K, N, axis = 2, 2097160, 0
    c = make_case(K, N, axis, "bf16")
    x, b = P.to_dev(c["X"], "bf16", torch), f32dev(torch, c["B"])
    ewops.set_entropy(SEED, offset=1)
    y, mask = ewops.bias_dropout_fwd(x, b, KEEP, axis=axis, relu=True)
    want_mask = ER.mask_words(K * N, SEED, 1, KEEP)
    assert np.array_equal(ER.as_u32(mask), want_mask)
    check("y", y, ER.forward(c["X"], c["B"], axis, 1, ER.unpack(want_mask, K * N), ER.scale_of(KEEP)), "bf16", "forward")
    K, N, axis = 513, 16384, 1
    c = make_case(K, N, axis, "bf16")
    x, dy, b = P.to_dev(c["X"], "bf16", torch), P.to_dev(c["E"], "bf16", torch), f32dev(torch, c["B"])
    dx, db = ewops.bias_relu_bwd(dy, ewops.bias_relu_fwd(x, b, axis=axis, relu=True), b, axis=axis, relu=True)
    wy, wdx, wdb = reference(c, axis, 1)
    check("dx", dx, wdx, "bf16", "backward")
    check("db", db, wdb, "f32", "backward")


def test_bad_arguments_raise_before_any_launch(env):
    torch, ewops = env
    from blocksparse_amd import bias_dropout, bias_relu, dropout
    x = torch.zeros(6, 4, 8, device="cuda")
    b8, b6 = torch.zeros(8, device="cuda"), torch.zeros(6, device="cuda")
    with pytest.raises(ValueError):
        bias_relu(x, b8, axis=1)                                  # a middle axis
    with pytest.raises(ValueError):
        bias_relu(x, b6, axis=-1)                                 # b has the wrong length
    with pytest.raises(ValueError):
        bias_relu(x, b8.half(), axis=-1)
    with pytest.raises(ValueError):
        bias_relu(x.double(), b8, axis=-1)
    with pytest.raises(ValueError):
        bias_relu(x, b8, relu=True, fast_gelu=True)
    with pytest.raises(ValueError):
        dropout(x, 0.0)
    with pytest.raises(ValueError):
        dropout(x, 0.5, mask=torch.zeros(5, dtype=torch.int32, device="cuda"))          # 192 elements want 6 words
    with pytest.raises(ValueError):
        dropout(x, 0.5, mask=torch.zeros(6, dtype=torch.int64, device="cuda"))
    with pytest.raises(NotImplementedError):
        dropout(x, 0.5, mask_shape=(6, 1, 1))
    with pytest.raises(ValueError):
        bias_dropout(x, b8, 1.5)
    with pytest.raises(ValueError):
        bias_dropout(x, b8, 0.5, residual=x[:3])
    with pytest.raises(ValueError):
        ewops.bias_dropout_bwd(x[:3], x, b8, torch.zeros(6, dtype=torch.int32, device="cuda"), 0.5)
    with pytest.raises(ValueError):
        ewops.bias_relu_bwd(x, x[:3], b8, relu=True)
    y = bias_relu(x, b6.view(2, 3), axis=0, atomics=False)        # b in any shape; atomics accepted
    assert y.shape == x.shape
    y, mask = dropout(x + 1.0, 1.0)                               # keep everything
    assert torch.equal(y, x + 1.0) and int(ER.unpack(ER.as_u32(mask), x.numel()).sum()) == x.numel()
