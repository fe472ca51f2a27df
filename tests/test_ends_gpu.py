"""GPU tier of the two operators at the ends of a model (include/bsmm_ends.h): softmax cross-entropy and the embedding lookup against
float64 evaluated on the same rounded inputs (tests/_ends_ref.py), in three dtypes, on every kernel path.  Each cross-entropy case asserts
the path it is there for (bsmm_xent_path), so a moved threshold cannot leave a path untested.

Criteria.  loss and dw: the fp32 bars of tests/_parity.py (dw: over the rows an index names; the others are exactly zero).  A 16-bit g or dx: every element equal or adjacent to the once-rounded float64
value (the fp16 scale applied before the rounding), at most 1 % adjacent, tensor L2 within the dtype's bar.  An fp32 dx: the correctly
rounded fp32 product, element by element.  An fp32 g, per element:
|got - want| <= (4 + 2 |x - max|) 2^-22 p + 2^-23 |want| + 2^-149 -- the rounding of the exponent's argument grows with |x - max|; the
rest is a few ulp for exp2, the reciprocal and the sum, and one step of the fp32 subnormals, below which no fp32 value can follow p.  Bit-exact: the forward in place, the backward in place, a repeated call, the embedding's forward,
its gradient of exactly summable values, and the rows no index names."""
import numpy as np
import pytest

import _ends_ref as ER
import _parity as P

pytestmark = pytest.mark.gpu
DTYPES = ("f32", "f16", "bf16")
S, R, W, G, V, T = 1, 2, 3, 4, 256, 512           # BSMM_XENT_* (tests/test_ends_host.py holds the binding's copies against the header)
# (N, K, elements the tensors lie off a 16-byte boundary, the path): every path on both sides of its limits, both access widths, the
# register depths of the short path (K <= 256 / 512 / 1024), rows beyond the reference's 65536, and more rows than the grid has workgroups
XENT_CASES = [
    (1, 1, 0, S), (3, 10, 0, S), (64, 256, 0, S | V), (5, 255, 0, S), (5, 257, 0, S), (4, 520, 0, S | V), (4, 1024, 0, S | V), (4, 1024, 1, S),
    (16, 1031, 0, R), (3, 1032, 0, R | V), (3, 4096, 1, R), (3, 4097, 0, W), (3, 8192, 0, R | V), (3, 8193, 0, W), (3, 8200, 0, W | V),
    (2, 16384, 1, W), (2, 16385, 0, G), (2, 32768, 0, W | V), (2, 32776, 0, G | V), (2, 65536, 0, G | V), (2, 70001, 0, G),
    (8197, 8, 0, S | V | T), (2049, 1032, 0, R | V | T),
]
XENT_IDS = ["N%d-K%d-off%d" % c[:3] for c in XENT_CASES]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import embed, xent
    return torch, xent, embed


def _place(torch, a, dtype, off):
    """a device tensor of the storage type holding `a`, `off` elements past a 16-byte boundary"""
    t = P.to_dev(a, dtype, torch)
    if not off:
        return t
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=t.device)
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _empty(torch, like, off):
    buf = torch.empty(like.numel() + 8, dtype=like.dtype, device=like.device)
    return buf[off:off + like.numel()].view(like.shape)


@pytest.mark.parametrize("dist", ("normal", "uniform"))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", XENT_CASES, ids=XENT_IDS)
def test_xent_against_float64(env, case, dtype, dist):
    torch, xent, _ = env
    N, K, off, path = case
    X, labels, dy = ER.xent_inputs(N, K, dtype, dist)
    wloss, wg, wp, wdist = ER.xent_ref(X, labels)
    scale = ER.stash_scale(dtype)
    ctx = (case, dtype, dist)
    x = _place(torch, X, dtype, off)
    lab = torch.from_numpy(labels).to("cuda")
    out = _empty(torch, x, off)
    assert xent.xent_path(x, out) == path and xent.xent_path(x) == path, (ctx, xent.xent_path(x, out))
    loss, g = xent.softmax_cross_entropy_fwd(x, lab, out=out)
    assert g is out and loss.dtype == torch.float32 and loss.shape == (N,)
    assert np.array_equal(P.to_host(x), X)                                       # the logits are as they were
    l2, mx = P.errors(P.to_host(loss), wloss)
    print("%s: loss L2 %.2e max %.2e" % (ctx, l2, mx))
    assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (ctx, "loss", l2, mx)
    got = P.to_host(g)
    if dtype == "f32":
        ratio, at = ER.f32_g_ratio(got, wg, wp, wdist)
        print("%s: fp32 g worst ratio to the bound %.3f at flat index %d" % (ctx, ratio, at))
        assert ratio <= 1.0, (ctx, "fp32 g beyond its bound", ratio, at, got.reshape(-1)[at], wg.reshape(-1)[at])
    else:
        ER.check_16bit(got, wg * scale, dtype, (ctx, "g"))
    ignored = (labels < 0) | (labels >= K)
    if ignored.any():
        assert not P.to_host(loss)[ignored].any() and not got[ignored].any(), (ctx, "ignored rows")
    # the same bits again, and in place over the logits
    loss2, g2 = xent.softmax_cross_entropy_fwd(x, lab, out=_empty(torch, x, off))
    assert torch.equal(loss2, loss) and torch.equal(g2, g), (ctx, "forward twice")
    xin = _empty(torch, x, off)
    xin.copy_(x)
    assert xent.xent_path(xin, xin) == path
    loss3, g3 = xent.softmax_cross_entropy_fwd(xin, lab, out=xin)
    assert g3 is xin and torch.equal(loss3, loss) and torch.equal(g3, g), (ctx, "forward in place")
    # the backward from the float64 stash rounded once, out of place and over the stash
    stash = ER.rounded(wg * scale, dtype)
    gs = _place(torch, stash, dtype, off)
    d = torch.from_numpy(dy).to("cuda")
    dx = xent.softmax_cross_entropy_bwd(gs, d, out=_empty(torch, gs, off))
    wdx = stash.astype(np.float64) / scale * dy.astype(np.float64)[:, None]
    gotdx = P.to_host(dx)
    if dtype == "f32":
        ER.check_f32_dx(gotdx, stash, dy, (ctx, "dx"))
    else:
        ER.check_16bit(gotdx, wdx, dtype, (ctx, "dx"))
    if ignored.any():
        assert not gotdx[ignored].any(), (ctx, "dx of ignored rows")
    assert np.array_equal(P.to_host(gs), stash)
    dx2 = xent.softmax_cross_entropy_bwd(gs, d, out=gs)
    assert dx2 is gs and torch.equal(dx2, dx), (ctx, "backward in place")


# (K, elements off a 16-byte boundary, the path): every path, both access widths
MASKED_CASES = [(10, 0, S), (520, 0, S | V), (1024, 1, S), (1032, 0, R | V), (4097, 0, W), (8200, 0, W | V), (16385, 0, G), (32776, 0, G | V),
                (32776, 1, G)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", MASKED_CASES, ids=["K%d-off%d" % c[:2] for c in MASKED_CASES])
def test_xent_masked_classes_against_float64(env, case, dtype):
    """Classes masked with -inf (tests/_ends_ref.py xent_masked_inputs: six rows, one pattern each) have probability 0.  The loss at the
    fp32 bars over the rows whose float64 loss is finite; the row whose label names a masked class has loss +inf and g[label] = -scale
    exactly; g of every masked class is exactly 0 (it is exp2(-inf) / s); every other element by the criteria of
    test_xent_against_float64, unchanged; the same bits from a second call and from the call in place.
    The streamed kernel once started every lane's running maximum at -inf and added exp2((-inf) - (-inf)) = NaN for a unit of masked
    classes read before any finite one: rows head, unit0 and single (and whatever else puts a masked unit first in a lane) came back NaN."""
    torch, xent, _ = env
    K, off, path = case
    X, labels = ER.xent_masked_inputs(K, dtype)
    wloss, wg, wp, wdist = ER.xent_ref(X, labels)
    scale = ER.stash_scale(dtype)
    ctx = (case, dtype)
    hot = ER.MASKED_LABEL_ROW
    fin_rows = np.isfinite(wloss)
    assert fin_rows.sum() == len(ER.MASKS) - 1 and wloss[hot] == np.inf
    x = _place(torch, X, dtype, off)
    lab = torch.from_numpy(labels).to("cuda")
    out = _empty(torch, x, off)
    assert xent.xent_path(x, out) == path and xent.xent_path(x) == path, (ctx, xent.xent_path(x, out))
    loss, g = xent.softmax_cross_entropy_fwd(x, lab, out=out)
    assert np.array_equal(P.to_host(x), X)
    hloss, got = P.to_host(loss), P.to_host(g)
    print("%s: loss %s" % (ctx, hloss))
    assert np.isfinite(hloss[fin_rows]).all(), (ctx, "loss of rows", [ER.MASKS[i] for i in np.nonzero(~np.isfinite(hloss) & fin_rows)[0]])
    l2, mx = P.errors(hloss[fin_rows], wloss[fin_rows])
    print("%s: loss L2 %.2e max %.2e" % (ctx, l2, mx))
    assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (ctx, "loss", l2, mx)
    assert hloss[hot] == np.inf, (ctx, "loss of a masked label", hloss[hot])
    finite = np.isfinite(X)
    assert not np.isnan(got).any(), (ctx, "NaN in g of rows", [ER.MASKS[i] for i in np.nonzero(np.isnan(got).any(axis=1))[0]])
    assert not got[~finite & (wg == 0)].any(), (ctx, "g of a masked class")
    assert got[hot, labels[hot]] == -scale and wg[hot, labels[hot]] == -1.0, (ctx, "g of the masked label", got[hot, labels[hot]])
    if dtype == "f32":
        ratio, at = ER.f32_g_ratio(got, wg, wp, wdist, finite)
        print("%s: fp32 g worst ratio to the bound %.3f at finite element %d" % (ctx, ratio, at))
        assert ratio <= 1.0, (ctx, "fp32 g beyond its bound", ratio, at)
    else:
        ER.check_16bit(got, wg * scale, dtype, (ctx, "g"), finite)
    loss2, g2 = xent.softmax_cross_entropy_fwd(x, lab, out=_empty(torch, x, off))
    assert torch.equal(loss2, loss) and torch.equal(g2, g), (ctx, "forward twice")
    xin = _empty(torch, x, off)
    xin.copy_(x)
    assert xent.xent_path(xin, xin) == path
    loss3, g3 = xent.softmax_cross_entropy_fwd(xin, lab, out=xin)
    assert g3 is xin and torch.equal(loss3, loss) and torch.equal(g3, g), (ctx, "forward in place")


@pytest.mark.parametrize("dtype", ("bf16", "f32"))
@pytest.mark.parametrize("K", (256, 16385))
def test_xent_nonfinite_row_stays_in_its_row(env, K, dtype):
    """+inf in row 2, NaN in row 5, row 6 all -inf: those rows' losses are NaN, as the float64 definition gives, and every other row's loss
    and g keep the bits of a call on the clean tensor (the short path shares a workgroup between four rows)."""
    torch, xent, _ = env
    N = 8
    X, _, _ = ER.xent_inputs(N, K, dtype, "uniform")
    labels = (np.arange(N) * 37 + 11) % K
    bad = X.copy()
    bad[2, K // 3] = np.inf
    bad[5, K - 2] = np.nan
    bad[6, :] = -np.inf
    with np.errstate(invalid="ignore"):
        wloss = ER.xent_ref(bad, labels)[0]
    dirty = np.array([2, 5, 6])
    clean = np.setdiff1d(np.arange(N), dirty)
    assert np.isnan(wloss[dirty]).all() and np.isfinite(wloss[clean]).all()
    lab = torch.from_numpy(labels).to("cuda")
    want_loss, want_g = xent.softmax_cross_entropy_fwd(P.to_dev(X, dtype, torch), lab)
    loss, g = xent.softmax_cross_entropy_fwd(P.to_dev(bad, dtype, torch), lab)
    assert xent.xent_path(g) & 255 == (S if K == 256 else G)
    assert torch.isnan(loss[torch.from_numpy(dirty).to("cuda")]).all(), (K, dtype, P.to_host(loss))
    rows = torch.from_numpy(clean).to("cuda")
    assert torch.equal(loss[rows], want_loss[rows]) and torch.equal(g[rows], want_g[rows]), (K, dtype, "a clean row changed")
    l2, mx = P.errors(P.to_host(loss)[clean], wloss[clean])
    assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (K, dtype, l2, mx)


@pytest.mark.parametrize("K,path", ((4097, W), (16385, G)))
def test_xent_strided_long_rows(env, K, path):
    """More rows than the grid has workgroups on the two paths for long rows: 7 base rows, checked against float64 in a call of their own,
    tiled on the device to N = 2049.  Row r keeps the bits of base row r % 7; only the base rows ever reach the host."""
    torch, xent, _ = env
    base, N = 7, 2049
    X, labels, _ = ER.xent_inputs(base, K, "bf16", "uniform")
    wloss, wg, _, _ = ER.xent_ref(X, labels)
    x7 = P.to_dev(X, "bf16", torch)
    lab7 = torch.from_numpy(labels).to("cuda")
    assert xent.xent_path(x7) == path
    loss7, g7 = xent.softmax_cross_entropy_fwd(x7, lab7)
    l2, mx = P.errors(P.to_host(loss7), wloss)
    assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (K, l2, mx)
    ER.check_16bit(P.to_host(g7), wg, "bf16", (K, "g of the base rows"))
    reps = (N + base - 1) // base
    x = x7.repeat(reps, 1)[:N].contiguous()
    lab = lab7.repeat(reps)[:N].contiguous()
    assert xent.xent_path(x) == path | T, xent.xent_path(x)
    loss, g = xent.softmax_cross_entropy_fwd(x, lab)
    assert torch.equal(loss, loss7.repeat(reps)[:N]), (K, "loss")
    assert torch.equal(g, g7.repeat(reps, 1)[:N]), (K, "g")


@pytest.mark.parametrize("ltype", ("uint8", "int16", "int32", "int64"))
def test_xent_label_dtypes(env, ltype):
    torch, xent, _ = env
    X, labels, _ = ER.xent_inputs(64, 256, "bf16", "normal")
    labels = np.where(labels < 0, 255 if ltype == "uint8" else -1, labels)      # (uint8 has no -1; 256 = K does not fit either: 255 is a class)
    labels = np.where(labels >= 256, 255 if ltype == "uint8" else 256, labels)
    x = P.to_dev(X, "bf16", torch)
    want = xent.softmax_cross_entropy_fwd(x, torch.from_numpy(labels.astype(np.int64)).to("cuda"))
    got = xent.softmax_cross_entropy_fwd(x, torch.from_numpy(labels.astype(np.int64)).to("cuda").to(getattr(torch, ltype)).reshape(8, 8))
    assert torch.equal(got[0].reshape(-1), want[0]) and torch.equal(got[1], want[1])
    wloss, _, _, _ = ER.xent_ref(X, labels)
    l2, mx = P.errors(P.to_host(want[0]), wloss)
    assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"]
    if ltype == "int64":                      # a label beyond int32 names no class
        big = torch.full((64,), 1 << 40, dtype=torch.int64, device="cuda")
        loss, g = xent.softmax_cross_entropy_fwd(x, big)
        assert not loss.any() and not g.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_xent_autograd_equals_the_low_level_pair(env, dtype):
    torch, xent, _ = env
    import blocksparse_amd
    N, K = 24, 520
    X, labels, dy = ER.xent_inputs(N, K, dtype, "normal")
    x = P.to_dev(X, dtype, torch).reshape(4, 6, K).requires_grad_(True)
    lab = torch.from_numpy(labels).to("cuda").reshape(4, 6)
    d = torch.from_numpy(dy).to("cuda").reshape(4, 6)
    loss = blocksparse_amd.softmax_cross_entropy(logits=x, labels=lab)
    assert loss.shape == (4, 6) and loss.dtype == torch.float32
    before = x.detach().clone()
    loss.backward(d)
    wloss, wg = xent.softmax_cross_entropy_fwd(x.detach(), lab)
    wdx = xent.softmax_cross_entropy_bwd(wg, d)
    assert torch.equal(loss.detach(), wloss) and torch.equal(x.grad, wdx) and x.grad.dtype == x.dtype
    assert torch.equal(x.detach(), before)                                       # autograd never works in place
    # a mean over the rows, the way a model takes it
    x.grad = None
    blocksparse_amd.softmax_cross_entropy(x, lab).mean().backward()
    assert torch.equal(x.grad, xent.softmax_cross_entropy_bwd(wg, torch.full((N,), 1.0 / N, device="cuda")).reshape(4, 6, K))


def test_xent_captured_step_replays_on_refreshed_logits(env):
    torch, xent, _ = env
    N, K = 64, 256
    X, labels, dy = ER.xent_inputs(N, K, "bf16", "normal")
    X2, _, _ = ER.xent_inputs(N, K, "bf16", "uniform")
    x = P.to_dev(X, "bf16", torch)
    lab = torch.from_numpy(labels).to("cuda")
    d = torch.from_numpy(dy).to("cuda")

    def step():
        loss, g = xent.softmax_cross_entropy_fwd(x, lab)
        return loss, g, xent.softmax_cross_entropy_bwd(g, d)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    torch.cuda.synchronize()
    for data in (X, X2):
        x.copy_(P.to_dev(data, "bf16", torch))
        graph.replay()
        torch.cuda.synchronize()
        want = step()
        for a, b in zip(outs, want):
            assert torch.equal(a, b)
        l2, mx = P.errors(P.to_host(outs[0]), ER.xent_ref(data, labels)[0])
        assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"]


# ---- embedding ------------------------------------------------------------------------------------------------------------------------
# (C, K, nIdx): one element; the element path; 16-byte rows on one team of 64 lanes; rows that are no multiple of 16 bytes on four column
# tiles of the element path; two column tiles of the 16-byte path
EMBED_SHAPES = [(1, 1, 1), (7, 5, 40), (50, 96, 300), (300, 1043, 64), (16, 2056, 33)]
EMBED_CASES = [(s, p) for s in EMBED_SHAPES for p in ER.PATTERNS]
EMBED_IDS = ["C%d-K%d-n%d-%s" % (s + (p,)) for s, p in EMBED_CASES]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", EMBED_CASES, ids=EMBED_IDS)
def test_embedding_against_numpy(env, case, dtype):
    torch, _, embed = env
    (C, K, n0), pattern = case
    idx = ER.embed_indices(C, n0, pattern)
    n = idx.size
    Wt, DY, DYX = ER.embed_values(C, K, n, dtype)
    ctx = (case, dtype)
    w = P.to_dev(Wt, dtype, torch)
    i64 = torch.from_numpy(idx).to("cuda")
    y, order = embed.embedding_lookup_fwd(w, i64)
    assert y.shape == (n, K) and y.dtype == w.dtype and order.dtype == torch.int32
    assert np.array_equal(P.to_host(y), ER.embed_fwd_ref(Wt, idx)), (ctx, "forward")
    assert np.array_equal(order.cpu().numpy(), ER.stable_order(np.clip(idx, -1, 2 ** 31 - 1))), (ctx, "order")
    want, named = ER.embed_grad_ref(DY, idx, C)
    dw = embed.embedding_lookup_bwd(P.to_dev(DY, dtype, torch), i64, C, order=order)
    assert dw.dtype == torch.float32 and dw.shape == (C, K)
    ER.check_dw(P.to_host(dw), want, named, ctx)
    dw2 = embed.embedding_lookup_bwd(P.to_dev(DY, dtype, torch), i64, C)             # (sorting again: the same order, the same bits)
    assert torch.equal(dw, dw2), (ctx, "backward twice")
    # exactly summable values: bit for bit against float64
    wantx, _ = ER.embed_grad_ref(DYX, idx, C)
    dwx = embed.embedding_lookup_bwd(P.to_dev(DYX, dtype, torch), i64, C, order=order)
    assert np.array_equal(P.to_host(dwx).astype(np.float64), wantx), (ctx, "exact sums")


@pytest.mark.parametrize("itype", ("uint8", "int16", "int32", "int64"))
def test_embedding_index_dtypes_and_shapes(env, itype):
    torch, _, embed = env
    C, K = 50, 96
    idx = ER.embed_indices(C, 300, "skew")
    Wt, DY, _ = ER.embed_values(C, K, idx.size, "bf16")
    w = P.to_dev(Wt, "bf16", torch)
    it = torch.from_numpy(idx).to("cuda").to(getattr(torch, itype)).reshape(3, 4, 25)
    y, order = embed.embedding_lookup_fwd(w, it)
    assert y.shape == (3, 4, 25, K) and np.array_equal(P.to_host(y).reshape(300, K), ER.embed_fwd_ref(Wt, idx))
    dw = embed.embedding_lookup_bwd(P.to_dev(DY, "bf16", torch).reshape(3, 4, 25, K), it, C, order=order)
    ER.check_dw(P.to_host(dw), *ER.embed_grad_ref(DY, idx, C), ctx=itype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_embedding_autograd(env, dtype):
    torch, _, embed = env
    import blocksparse_amd
    C, K = 50, 96
    idx = ER.embed_indices(C, 300, "outside")
    Wt, _, DYX = ER.embed_values(C, K, idx.size, dtype)
    w = P.to_dev(Wt, dtype, torch).requires_grad_(True)
    it = torch.from_numpy(idx).to("cuda").reshape(10, 30)
    y = blocksparse_amd.embedding_lookup(w, it, sort_grad=False)                  # (accepted and ignored)
    assert y.shape == (10, 30, K) and np.array_equal(P.to_host(y).reshape(300, K), ER.embed_fwd_ref(Wt, idx))
    y.backward(P.to_dev(DYX, dtype, torch).reshape(10, 30, K))
    assert w.grad.dtype == w.dtype and w.grad.shape == (C, K)
    # w.grad is the fp32 gradient rounded once to the table's dtype
    want = ER.rounded(ER.embed_grad_ref(DYX, idx, C)[0], dtype)
    assert np.array_equal(P.to_host(w.grad), want)


def test_embedding_captured_step_replays_on_refreshed_indices(env):
    torch, _, embed = env
    C, K, n = 50, 96, 300
    idx_a, idx_b = ER.embed_indices(C, n, "skew"), ER.embed_indices(C, n, "tiled")
    Wt, DY, _ = ER.embed_values(C, K, n, "bf16")
    w, dy = P.to_dev(Wt, "bf16", torch), P.to_dev(DY, "bf16", torch)
    it = torch.from_numpy(idx_a).to("cuda")

    def step():
        y, order = embed.embedding_lookup_fwd(w, it)
        return y, embed.embedding_lookup_bwd(dy, it, C, order=order)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    torch.cuda.synchronize()
    for idx in (idx_a, idx_b):
        it.copy_(torch.from_numpy(idx).to("cuda"))
        graph.replay()
        torch.cuda.synchronize()
        want = step()
        assert torch.equal(outs[0], want[0]) and torch.equal(outs[1], want[1])
        assert np.array_equal(P.to_host(outs[0]), ER.embed_fwd_ref(Wt, idx))
        ER.check_dw(P.to_host(outs[1]), *ER.embed_grad_ref(DY, idx, C), ctx="captured")
