"""GPU tier of the layer norm (include/bsmm_norm.h through blocksparse_amd/norms.py) against the float64 helper tests/_layer_norm_ref.py on
inputs pre-rounded to the storage type.  y and dx are held to the bars of their dtype (tests/_parity.py), mean / rstd / dg / db are fp32 in
every dtype and held to the fp32 bars.  Each shape is the smallest that reaches a distinct code path (see PATHS); ReLU only where the
smallest pre-activation of the inputs is provably far from fp32 rounding of the mask (asserted, no element excluded)."""
import numpy as np
import pytest

import _layer_norm_ref as LR
import _parity as P
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f16", "bf16")
# (K, N, axis, S): what the case is there for
PATHS = [
    (32, 4, 0, 1), (31, 4, 0, 1), (33, 4, 0, 1),       # the reference test's shapes and a power of two, both axes
    (32, 4, 1, 1), (31, 4, 1, 1), (33, 4, 1, 1),
    (96, 40, 0, 1),                                      # 16-byte path
    (96, 37, 0, 2),                                      # element path, segments on axis 0
    (1031, 24, 0, 1),                                    # prime K, few columns: K cut over many workgroups, ragged last slice
    (40, 1043, 0, 1),                                    # several strips and a ragged last one, element path
    (40, 1048, 0, 1),                                    # several strips, the last partly filled, 16-byte path
    (128, 5, 1, 4),                                      # segments on axis 1
    (36, 1043, 1, 1),                                    # rows not 16-byte aligned (16-bit), many rows per group
    (2052, 3, 1, 1),                                     # just past what a wave holds (2048): a workgroup per row; element path for 16-bit
    (2056, 3, 1, 1),                                     # the same on the 16-byte path
    (8193, 3, 1, 1),                                     # one past what is read once (8192): the streamed row, element path
    (8200, 3, 1, 1),                                     # the streamed row on the 16-byte path
]
RELU_PATHS = [p for p in PATHS if p[0] <= 96 and p[1] <= 40]
IDS = lambda cases: ["K%d-N%d-a%d-S%d" % c for c in cases]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from blocksparse_amd import norms
    return torch, norms


_cache = {}


def make_case(K, N, axis, S, dtype, relu=False, shape=None, seed=None):
    """Seeded inputs (N(0, 1) through fp16, then the storage type; g, b through fp16) and the float64 results, computed once per case."""
    key = (K, N, axis, S, dtype, relu, shape, seed)
    if key in _cache:
        return _cache[key]
    shape = shape or ((K, N) if axis == 0 else (N, K))
    base = 1000 * K + 10 * N + axis if seed is None else seed
    for attempt in range(64):                            # (ReLU: the first seed whose smallest pre-activation is clear of the mask's rounding)
        rng = np.random.RandomState(base + 7919 * attempt)
        f16 = lambda a: a.astype(np.float16).astype(np.float32)
        X = orc.round_to(f16(rng.normal(0.0, 1.0, shape)), dtype)
        E = orc.round_to(f16(rng.normal(0.0, 1.0, shape)), dtype)
        G, B = f16(rng.normal(0.0, 1.0, K)), f16(rng.normal(0.0, 1.0, K))
        if not relu or np.abs(LR.pre_activation(X, G, B, axis, S)).min() >= 1e-4:
            break
    ax = 0 if axis == 0 else -1
    c = dict(X=X, E=E, G=G, B=B, Y=LR.forward(X, G, B, ax, S, 1e-6, relu))
    c["MEAN"], c["RSTD"] = LR.stats(X, ax, S, 1e-6)
    c["DX"], c["DG"], c["DB"] = LR.backward(E, X, G, B, ax, S, 1e-6, relu)
    for a in c.values():
        a.setflags(write=False)
    _cache[key] = c
    return c


def dev(torch, c, dtype):
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")
    return P.to_dev(c["X"], dtype, torch), P.to_dev(c["E"], dtype, torch), f32(c["G"]), f32(c["B"])


def check(name, got, want64, dtype, ctx):
    want = orc.round_to(np.asarray(want64), dtype) if dtype != "f32" else np.asarray(want64)
    got = P.to_host(got)
    assert got.shape == want.shape, (ctx, name, got.shape, want.shape)
    assert np.isfinite(got).all(), (ctx, name)
    l2, mx = P.errors(got, want)
    print(ctx, name, "l2 %.3g max %.3g" % (l2, mx))
    assert l2 <= P.L2_BAR[dtype] and mx <= P.MAX_BAR[dtype], (ctx, name, l2, mx)


def run_and_check(env, c, axis, S, dtype, relu, ctx):
    torch, norms = env
    x, dy, g, b = dev(torch, c, dtype)
    y, mean, rstd = norms.layer_norm_fwd(x, g, b, axis=axis, segments=S, relu=relu)
    dx, dg, db = norms.layer_norm_bwd(dy, x, g, b, mean, rstd, axis=axis, segments=S, relu=relu)
    assert y.dtype == x.dtype and dx.dtype == x.dtype and y.shape == x.shape and dx.shape == x.shape
    assert mean.dtype == rstd.dtype == dg.dtype == db.dtype == torch.float32 and dg.shape == g.shape and db.shape == b.shape
    assert tuple(mean.shape) == c["MEAN"].shape == tuple(rstd.shape)
    check("y", y, c["Y"], dtype, ctx)
    check("mean", mean, c["MEAN"], "f32", ctx)
    check("rstd", rstd, c["RSTD"], "f32", ctx)
    check("dx", dx, c["DX"], dtype, ctx)
    check("dg", dg, c["DG"], "f32", ctx)
    check("db", db, c["DB"], "f32", ctx)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", PATHS, ids=IDS(PATHS))
def test_against_float64(env, case, dtype):
    K, N, axis, S = case
    run_and_check(env, make_case(K, N, axis, S, dtype), axis, S, dtype, False, (case, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", RELU_PATHS, ids=IDS(RELU_PATHS))
def test_relu_against_float64(env, case, dtype):
    K, N, axis, S = case
    c = make_case(K, N, axis, S, dtype, relu=True)
    smallest = np.abs(LR.pre_activation(c["X"], c["G"], c["B"], axis, S)).min()
    print(case, dtype, "smallest |pre-activation| %.3g" % smallest)
    assert smallest >= 1e-4, (case, dtype, smallest)     # the mask of every element is decided far above fp32 rounding: none is excluded
    assert (c["Y"] == 0).any() and (c["Y"] > 0).any()
    run_and_check(env, c, axis, S, dtype, True, (case, dtype, "relu"))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis", (0, -1))
def test_rank_three_inputs(env, axis, dtype):
    shape = (24, 3, 8) if axis == 0 else (3, 5, 40)      # axis 0: N = 24 columns (16-byte path);  last axis: 15 rows of 40
    K = shape[axis]
    c = make_case(K, int(np.prod(shape)) // K, axis, 2, dtype, shape=shape)
    run_and_check(env, c, axis, 2, dtype, False, (shape, axis, dtype))


def test_bad_arguments_raise_before_any_launch(env):
    torch, norms = env
    x = torch.zeros(6, 4, 8, device="cuda")
    g8, g6 = torch.ones(8, device="cuda"), torch.ones(6, device="cuda")
    with pytest.raises(ValueError):
        norms.layer_norm(x, g8, g8, axis=1)                       # a middle axis
    with pytest.raises(ValueError):
        norms.layer_norm(x, g6, g6, axis=-1)                      # g has the wrong length
    with pytest.raises(ValueError):
        norms.layer_norm(x, g8, g8, axis=-1, segments=3)
    with pytest.raises(ValueError):
        norms.layer_norm(x, g8.half(), g8, axis=-1)
    with pytest.raises(ValueError):
        norms.layer_norm(x.double(), g8, g8, axis=-1)
    with pytest.raises(ValueError):
        norms.layer_norm_bwd(x[:3], x, g8, g8, torch.zeros(1, 24, device="cuda"), torch.zeros(1, 24, device="cuda"), axis=-1)
    y = norms.layer_norm(x, g8.view(2, 4), g8.view(1, 8), axis=-1)     # g and b in any shape
    assert y.shape == x.shape


@pytest.mark.parametrize("axis", (0, 1))
def test_large_offset_keeps_the_variance(env, axis):
    """x = 300 + 0.5 N(0, 1): an fp32 mean carries a few eps of relative error and the subtraction magnifies it by |mean| / std = 600, which
    sets the bar 32 * 2^-24 * 600 = 1.1e-3 (two-pass fp32 in NumPy: 2.3e-4); E[x^2] - mean^2 loses the variance and lands at 0.14."""
    torch, norms = env
    K, N = 512, 8
    rng = np.random.RandomState(77 + axis)
    X = (300.0 + 0.5 * rng.normal(0.0, 1.0, (K, N) if axis == 0 else (N, K))).astype(np.float32)
    G, B = np.ones(K, dtype=np.float32), np.zeros(K, dtype=np.float32)
    want = LR.forward(X, G, B, axis)
    y, mean, rstd = norms.layer_norm_fwd(*(torch.from_numpy(a).to("cuda") for a in (X, G, B)), axis=axis)
    l2, _ = P.errors(P.to_host(y), want)
    print("offset axis", axis, "l2 %.3g" % l2)
    assert l2 <= 32 * 2.0 ** -24 * 300.0 / 0.5, (axis, l2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(96, 40, 0, 2), (96, 37, 0, 2), (1031, 24, 0, 1), (128, 5, 1, 4), (36, 1043, 1, 1), (2052, 3, 1, 1)],
                         ids=IDS([(96, 40, 0, 2), (96, 37, 0, 2), (1031, 24, 0, 1), (128, 5, 1, 4), (36, 1043, 1, 1), (2052, 3, 1, 1)]))
def test_backward_twice_gives_the_same_bits(env, case, dtype):
    torch, norms = env
    K, N, axis, S = case
    x, dy, g, b = dev(torch, make_case(K, N, axis, S, dtype), dtype)
    y, mean, rstd = norms.layer_norm_fwd(x, g, b, axis=axis, segments=S)
    first = norms.layer_norm_bwd(dy, x, g, b, mean, rstd, axis=axis, segments=S)
    torch.empty(1 << 20, device="cuda").fill_(float("nan"))       # (another workspace block for the second call, with other contents)
    second = norms.layer_norm_bwd(dy, x, g, b, mean, rstd, axis=axis, segments=S)
    for a, c, name in zip(first, second, ("dx", "dg", "db")):
        assert torch.equal(a, c), (case, dtype, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(96, 40, 0, 2), (33, 4, 0, 1), (128, 5, 1, 4), (2052, 3, 1, 1)], ids=IDS([(96, 40, 0, 2), (33, 4, 0, 1), (128, 5, 1, 4), (2052, 3, 1, 1)]))
def test_relu_is_the_identity_on_positive_pre_activations(env, case, dtype):
    """With b shifted so that every pre-activation is positive, relu=True stores the bits relu=False stores, forward and backward."""
    torch, norms = env
    K, N, axis, S = case
    c = make_case(K, N, axis, S, dtype)
    x, dy, g, b = dev(torch, c, dtype)
    shift = float(np.ceil(-LR.pre_activation(c["X"], c["G"], c["B"], axis, S).min())) + 1.0
    b = b + shift
    assert LR.pre_activation(c["X"], c["G"], c["B"] + shift, axis, S).min() >= 0.5
    plain = norms.layer_norm_fwd(x, g, b, axis=axis, segments=S, relu=False)
    relu = norms.layer_norm_fwd(x, g, b, axis=axis, segments=S, relu=True)
    for a, r, name in zip(plain, relu, ("y", "mean", "rstd")):
        assert torch.equal(a, r), (case, dtype, name)
    gp = norms.layer_norm_bwd(dy, x, g, b, plain[1], plain[2], axis=axis, segments=S, relu=False)
    gr = norms.layer_norm_bwd(dy, x, g, b, plain[1], plain[2], axis=axis, segments=S, relu=True)
    for a, r, name in zip(gp, gr, ("dx", "dg", "db")):
        assert torch.equal(a, r), (case, dtype, name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(96, 40, 0, 2), (96, 37, 0, 2), (128, 5, 1, 4), (4104, 20, 1, 2)], ids=IDS([(96, 40, 0, 2), (96, 37, 0, 2), (128, 5, 1, 4), (4104, 20, 1, 2)]))
def test_segments_equal_separate_calls_on_the_slices(env, case, dtype):
    torch, norms = env
    K, N, axis, S = case
    Ks = K // S
    x, dy, g, b = dev(torch, make_case(K, N, axis, S, dtype), dtype)
    y, mean, rstd = norms.layer_norm_fwd(x, g, b, axis=axis, segments=S, relu=True)
    dx, dg, db = norms.layer_norm_bwd(dy, x, g, b, mean, rstd, axis=axis, segments=S, relu=True)
    for s in range(S):
        k = slice(s * Ks, (s + 1) * Ks)
        cut = (lambda t: t[k].contiguous()) if axis == 0 else (lambda t: t[:, k].contiguous())
        ys, ms, rs = norms.layer_norm_fwd(cut(x), g[k].contiguous(), b[k].contiguous(), axis=axis, relu=True)
        dxs, dgs, dbs = norms.layer_norm_bwd(cut(dy), cut(x), g[k].contiguous(), b[k].contiguous(), ms, rs, axis=axis, relu=True)
        for whole, part, name in ((cut(y), ys, "y"), (mean[s:s + 1], ms, "mean"), (rstd[s:s + 1], rs, "rstd"), (cut(dx), dxs, "dx"), (dg[k], dgs, "dg"),
                                  (db[k], dbs, "db")):
            assert torch.equal(whole, part), (case, dtype, s, name)


@pytest.mark.parametrize("axis", (0, 1))
def test_autograd_gives_the_low_level_gradients(env, axis):
    torch, norms = env
    from blocksparse_amd import layer_norm
    K, N, S = 96, 40, 2
    x, dy, g, b = dev(torch, make_case(K, N, axis, S, "bf16"), "bf16")
    g, b = g.view(2, 48), b.view(1, K)                   # (gradients come back in the shapes of g and b)
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, g, b))
    y = layer_norm(xr, gr, br, axis=axis, segments=S, relu=True)
    got = torch.autograd.grad(y, (xr, gr, br), dy)
    y2, mean, rstd = norms.layer_norm_fwd(x, g, b, axis=axis, segments=S, relu=True)
    want = norms.layer_norm_bwd(dy, x, g, b, mean, rstd, axis=axis, segments=S, relu=True)
    assert torch.equal(y.detach(), y2)
    for a, w, name in zip(got, want, ("dx", "dg", "db")):
        assert a.dtype == w.dtype and a.shape == w.shape and torch.equal(a, w), (axis, name)
    assert got[0].dtype == torch.bfloat16 and got[1].dtype == got[2].dtype == torch.float32 and got[1].shape == g.shape and got[2].shape == b.shape


@pytest.mark.parametrize("axis", (0, 1))
def test_captured_forward_and_backward_replay_onto_refreshed_inputs(env, axis):
    """One single-stream capture of forward plus backward: a replay computes from the CURRENT contents of x, dy, g and b."""
    torch, norms = env
    K, N, S = 96, 40, 2
    x, dy, g, b = dev(torch, make_case(K, N, axis, S, "bf16"), "bf16")
    x2, dy2, g2, b2 = dev(torch, make_case(K, N, axis, S, "bf16", seed=4242), "bf16")
    assert not torch.equal(x, x2)

    def step():
        y, mean, rstd = norms.layer_norm_fwd(x, g, b, axis=axis, segments=S, relu=True)
        return (y, mean, rstd) + tuple(norms.layer_norm_bwd(dy, x, g, b, mean, rstd, axis=axis, segments=S, relu=True))

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for t, t2 in ((x, x2), (dy, dy2), (g, g2), (b, b2)):
        t.copy_(t2)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in outs]
    want = step()
    torch.cuda.synchronize()
    for a, w, name in zip(got, want, ("y", "mean", "rstd", "dx", "dg", "db")):
        assert torch.equal(a, w), (axis, name)
    c2 = make_case(K, N, axis, S, "bf16", relu=False, seed=4242)
    l2, _ = P.errors(P.to_host(got[1]), c2["MEAN"])
    assert l2 <= P.L2_BAR["f32"]


OUTLIER_PARAMS = [(case, dtype) for case in LR.OUTLIER_CASES for dtype in LR.outlier_dtypes(case)]


def check_outlier(name, got, c, dtype, ctx):
    """An fp32 result: max(the fp32 bar, 8 x the error of the float32 NumPy model on the same input), for the L2 and the max figure alike
    (the margin is over the model, whose pairwise sums a lane-serial kernel does not reproduce -- not over the code under test).  A 16-bit
    result: the bars of its dtype against float64 rounded once, as everywhere in this file."""
    got = P.to_host(got)
    assert got.shape == c[name].shape and np.isfinite(got).all(), (ctx, name)
    if dtype != "f32":
        l2, mx = P.errors(got, orc.round_to(c[name], dtype))
        print(ctx, name, "device l2 %.3g max %.3g" % (l2, mx))
        assert l2 <= P.L2_BAR[dtype] and mx <= P.MAX_BAR[dtype], (ctx, name, l2, mx)
        return
    l2_bar, mx_bar, ml2, mmx = LR.outlier_bars(c, name, P.L2_BAR["f32"], P.MAX_BAR["f32"])
    l2, mx = P.errors(got, c[name])
    print(ctx, name, "model l2 %.3g max %.3g | device l2 %.3g max %.3g | bars %.3g %.3g" % (ml2, mmx, l2, mx, l2_bar, mx_bar))
    assert l2 <= l2_bar and mx <= mx_bar, (ctx, name, l2, mx, l2_bar, mx_bar)


OUTLIER_MARKS = [pytest.mark.parametrize("at", (0, 1), ids=("first-feature", "second-feature")),
                 pytest.mark.parametrize("A", LR.OUTLIER_SIZES, ids=lambda a: "A%d" % a),
                 pytest.mark.parametrize("case,dtype", OUTLIER_PARAMS, ids=["K%d-N%d-a%d-S%d-%s" % (c + (d,)) for c, d in OUTLIER_PARAMS])]


def outlier_marks(fn):
    for m in reversed(OUTLIER_MARKS):
        fn = m(fn)
    return fn


@outlier_marks
def test_outlier_first_feature_keeps_the_variance(env, case, dtype, A, at):
    """N(0, 1) inputs whose first feature of every segment is +A / -A (a massive-activation dimension), and as the control the same
    outlier in the second feature: the statistics may not depend on which element a kernel reads first.  mean, rstd (fp32 in every dtype)
    and an fp32 y against float64 by check_outlier, a 16-bit y at the bars of its dtype.
    With var = sum (x - c)^2 / Ks - (mean - c)^2, c = the first feature, the kernels of the axis-0 statistics and of the streamed axis-1
    row missed the rstd bar on every first-feature case and met it on every control.  Measured rstd L2 error of that form on an MI355X,
    next to the float32 model of tests/_layer_norm_ref.py (stats_f32_shifted): Ks = 512: 1.1e-5 (model 1.4e-5) at A = 30, 1.7e-5 (2.1e-5)
    at A = 1000; Ks = 8200 on axis 0: 6.9e-5 (1.4e-4) and 8.1e-4 (1.2e-3), bf16 8.6e-4; Ks = 8193 on axis 1: 1.5e-5 (4.9e-5) and 8.7e-5
    (9.0e-4).  The segments of 48 features failed on the max figure of y only (3.4e-5 against 2.6e-5); their rstd stayed under 2e-6.
    The two-pass kernels measure at most 2.0e-7 over all cases (the float32 two-pass model, whose NumPy sum down a column is serial: up
    to 3.4e-6 at Ks = 8200 on axis 0, which is where the model's half of the bar comes into play)."""
    torch, norms = env
    K, N, axis, S = case
    c = LR.outlier_case(K, N, axis, S, dtype, A, at)
    ctx = (case, dtype, A, at)
    x, dy, g, b = dev(torch, c, dtype)
    y, mean, rstd = norms.layer_norm_fwd(x, g, b, axis=axis, segments=S)
    assert tuple(mean.shape) == c["MEAN"].shape == tuple(rstd.shape) and mean.dtype == rstd.dtype == torch.float32
    check_outlier("MEAN", mean, c, "f32", ctx)
    check_outlier("RSTD", rstd, c, "f32", ctx)
    check_outlier("Y", y, c, dtype, ctx)


@outlier_marks
def test_outlier_feature_backward_from_float64_statistics(env, case, dtype, A, at):
    """The backward on the same inputs, from the float64 statistics rounded to fp32, so that it stands apart from the forward: dx, dg and
    db by check_outlier against the float32 NumPy evaluation of the formulas of include/bsmm_norm.h.
    The max figure is max |diff| / mean |dg|, and the outlier's own dg is 470 times the mean |dg| (57.7 against 0.122 at K8193 bf16):
    there 2e-5 of the mean is 0.64 of ONE fp32 step of the value, so the bar asks for a dg that is all but correctly rounded.  With the
    term dy (x - mean) rstd and its sum over the samples in fp32 the kernels missed the max figure of dg on two cases, 0.9 steps from float64:
      K8193-N3-a1-S1-bf16-A1000-first-feature:   device 2.84e-5, bar max(2e-5, 8 x 2.81e-6) = 2.25e-5
      K8200-N8-a0-S1-f16-A1000-second-feature:   device 6.20e-5, bar max(2e-5, 8 x 6.93e-6) = 5.54e-5
    The axis-0 kernel and the column walk of the streamed axis-1 row now form that term and sum it in fp64 within a partial: 2.81e-6 and
    6.93e-6 on an MI355X, the model's own figures (both are the correctly rounded fp32 value); over all 52 cases dg is at most 0.13 of its bar."""
    torch, norms = env
    K, N, axis, S = case
    c = LR.outlier_case(K, N, axis, S, dtype, A, at)
    ctx = (case, dtype, A, at)
    x, dy, g, b = dev(torch, c, dtype)
    m32, r32 = (torch.from_numpy(np.ascontiguousarray(c[n])).to("cuda") for n in ("MEAN32", "RSTD32"))
    dx, dg, db = norms.layer_norm_bwd(dy, x, g, b, m32, r32, axis=axis, segments=S)
    check_outlier("DX", dx, c, dtype, ctx)
    check_outlier("DG", dg, c, "f32", ctx)
    check_outlier("DB", db, c, "f32", ctx)
