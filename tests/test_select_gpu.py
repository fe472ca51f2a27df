"""GPU tier of the fused row selection (include/bsmm_select.h through blocksparse_amd/select.py) against tests/_select_ref.py: the selected
set bit for bit under the pinned order -- distinct values, ties across the k-th position, +-0 ties, more masked elements than K - k --,
``rectified_top_k`` bit for bit against the NumPy float32 definition, the softmaxes, their gradient and ``sparse_relu`` against float64 at the
bars of tests/_parity.py, repeatability, the 16-byte against the element form, autograd and one captured forward + backward.  Row lengths:
1, 5, around the wave (63 .. 65), T - 1, T, T + 1 at every path threshold T, 1000, 1024 and the longest row served; every test asserts the
path it ran."""
import numpy as np
import pytest

import _parity as P
import _select_ref as SR
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f16", "bf16")
KS = (1, 5, 63, 64, 65) + tuple(T + d for T in SR.THRESHOLDS for d in (-1, 0, 1)) + (1000, 1024, SR.MAX_K)
SCALE = 0.25                              # a power of two: distinct inputs stay distinct scores; the scores span less than 0.7
CASES = [(K, d) for K in sorted(set(KS)) for d in DTYPES]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from blocksparse_amd import select
    return torch, select


def ks_of(K):
    return sorted({k for k in (1, 2, 17, K - 1, K) if 1 <= k <= K})


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rounded(a64, dtype):
    return orc.round_to(np.asarray(a64), dtype) if dtype != "f32" else np.asarray(a64)


def close(got, want64, dtype, what):
    l2, mx = P.errors(P.to_host(got).reshape(np.shape(want64)), rounded(want64, dtype))
    assert l2 <= P.L2_BAR[dtype] and mx <= P.MAX_BAR[dtype], (what, l2, mx)


def close_l2(got, want64, dtype, what):
    """The L2 bar alone, where most of the expected values are zeros: the max bar is measured against mean |ref|, which k of K non-zero
    values pull down by K / k -- it then asks of the few non-zero values K / k times the accuracy it stands for."""
    l2, mx = P.errors(P.to_host(got).reshape(np.shape(want64)), rounded(want64, dtype))
    assert l2 <= P.L2_BAR[dtype], (what, l2, mx)


def path_of(select, torch, K, dtype, *tensors):
    aligned = all(t is None or t.data_ptr() % 16 == 0 for t in tensors)
    got = select.select_path(K, getattr(torch, P.TORCH_DT[dtype]), aligned)
    assert got == SR.path_name(K, dtype, aligned)
    return got


@pytest.mark.parametrize("case", CASES, ids=["K%d-%s" % c for c in CASES])
def test_selection_bit_for_bit(env, case):
    """Nine rows -- one more than a multiple of the four rows of a workgroup -- of four data sets in ONE call per k: distinct values,
    five values with a tie across the k-th position, +-0 across it, and rows with fewer than k unmasked elements (every row has a mask row
    of its own).  The nonzero pattern of the top-k softmax is S less its masked members, and rectified top-k stores the bits of the NumPy
    float32 definition rounded once, with and without the rebase."""
    torch, select = env
    K, dtype = case
    rng = np.random.default_rng(100 * K + DTYPES.index(dtype))
    geom = {"wave8": K <= 512, "wave16": 512 < K <= 1024, "group2": 1024 < K <= 2048, "group4": K > 2048}
    for k in ks_of(K):
        X = np.concatenate((SR.distinct_rows(2, K, dtype, rng), SR.tied_rows(2, K, k, rng), SR.zero_rows(2, K, k, rng),
                            SR.distinct_rows(3, K, dtype, rng)))
        M = np.concatenate((np.ones((6, K), dtype=np.float32), SR.sparse_mask(3, K, k, rng)))
        assert np.array_equal(SR.round_in(X, dtype), X)
        if k < K:                                          # the ties do cross the k-th position
            o = SR.order(X[2:6])
            assert (np.take_along_axis(X[2:6], o[:, k - 1:k], 1) == np.take_along_axis(X[2:6], o[:, k:k + 1], 1)).all()
        assert ((M[6:] != 0).sum(axis=1) < k).all()        # more than K - k masked
        y64, S = SR.topk_softmax(X, k, M, SCALE)
        want_nz = S & (M != 0)
        assert y64[want_nz].min(initial=1.0) > 2 * SR.TINY[dtype] and not y64[~want_nz].any()     # every selected probability is a normal number
        x, m = P.to_dev(X, dtype, torch), torch.from_numpy(M).cuda()
        y = select.masked_top_k_softmax_fwd(x, k, m, SCALE)
        path = path_of(select, torch, K, dtype, x, m, y)
        assert geom[path.split("-")[0]], (K, path)
        got = P.to_host(y)
        assert np.array_equal(got != 0, want_nz), (case, k, "selected set", np.argwhere((got != 0) != want_nz)[:4])
        close_l2(y, y64, dtype, (case, k, "top-k softmax"))
        for rebase in (True, False):
            want = rounded(select.rectified_top_k_test(X, k, rebase), dtype)
            got = P.to_host(select.rectified_top_k_fwd(x, k, rebase))
            assert np.array_equal(bits(got), bits(want)), (case, k, rebase, np.argwhere(bits(got) != bits(want))[:4])
            # the float64 helper agrees once its difference is rounded to fp32 as the definition's is (53 bits: no double rounding)
            np.testing.assert_array_equal(want, rounded(SR.rect(X, k, rebase).astype(np.float32), dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", (65, 1025))
def test_softmax_values_gradients_and_mask_shapes(env, K, dtype):
    """(2, 3, 5, K) with masks of 1, T and H * T rows and without one; k = 17 of 65 resp. half of 1025 (at least a quarter of the expected
    values are non-zero, so the max bar, which is relative to mean |ref|, keeps its meaning) and k = K; masked_softmax and softmax are the
    k = K calls.  One (h, t) row of the largest mask is all zeros: those rows store zeros."""
    torch, select = env
    rng = np.random.default_rng(K + DTYPES.index(dtype))
    B, H, T = 2, 3, 5
    X = SR.round_in(rng.normal(0.0, 1.0, (B, H, T, K)), dtype)
    DY = SR.round_in(rng.normal(0.0, 1.0, (B, H, T, K)), dtype)
    x, dy = P.to_dev(X, dtype, torch), P.to_dev(DY, dtype, torch)
    for mshape in (None, (1, 1, 1, K), (1, 1, T, K), (1, H, T, K)):
        M = m = None
        if mshape is not None:
            M = np.where(rng.random(mshape) < 0.3, 0.0, rng.choice([1.0, 0.5, 2.0], mshape)).astype(np.float32)
            M[..., 3] = 1.0
            if mshape[1] == H:
                M[0, 1, 2, :] = 0.0
            m = torch.from_numpy(M).cuda()
        for k in (17 if K == 65 else K // 2, K):
            scale = 0.5
            y64, _ = SR.topk_softmax(X, k, M, scale)
            if k == K:
                y = select.masked_softmax_fwd(x, m, scale) if m is not None else select.softmax(x, scale)
            else:
                y = select.masked_top_k_softmax_fwd(x, k, m, scale)
            assert path_of(select, torch, K, dtype, x, m, y) == SR.path_name(K, dtype)
            close(y, y64, dtype, (K, dtype, mshape, k, "y"))
            yh = P.to_host(y).astype(np.float64)
            dead = np.zeros((B, H, T), dtype=bool)
            if mshape is not None and mshape[1] == H:
                dead[:, 1, 2] = True
                assert not yh[dead].any()
            sums = yh.sum(axis=-1)[~dead]
            print("row sums: max |sum - 1| = %.3g" % np.abs(sums - 1).max())
            assert np.abs(sums - 1).max() <= P.MAX_BAR[dtype], (K, dtype, mshape, k)
            dx = select.masked_softmax_bwd(dy, y, m, scale)
            close(dx, SR.softmax_grad(DY, P.to_host(y), M, scale), dtype, (K, dtype, mshape, k, "dx"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_nan_and_inf_stay_in_their_rows(env, dtype):
    torch, select = env
    rng = np.random.default_rng(5)
    for K in (65, 2049):
        X = SR.round_in(rng.normal(0.0, 1.0, (7, K)), dtype)
        bad = X.copy()
        bad[1, K // 2] = np.nan
        bad[4, 3] = np.inf
        clean, dirty = P.to_dev(X, dtype, torch), P.to_dev(bad, dtype, torch)
        keep = [0, 2, 3, 5, 6]
        for k in (2, K):
            a, b = select.masked_top_k_softmax_fwd(clean, k, None, 0.5), select.masked_top_k_softmax_fwd(dirty, k, None, 0.5)
            assert torch.equal(a[keep], b[keep]) and torch.isnan(b[1]).any() and torch.isnan(b[4]).any()
            a, b = select.rectified_top_k_fwd(clean, k), select.rectified_top_k_fwd(dirty, k)
            assert torch.equal(a[keep], b[keep])
            assert bool(torch.isnan(b[1, K // 2])) and int(torch.isnan(b[1]).sum()) == 1          # the NaN is selected and shows
            want = select.rectified_top_k_test(bad, k)
            assert np.array_equal(np.isnan(P.to_host(b)), np.isnan(want))


@pytest.mark.parametrize("dtype", DTYPES)
def test_sparse_relu_against_float64(env, dtype):
    torch, select = env
    rng = np.random.default_rng(9 + DTYPES.index(dtype))
    for K, R in ((1, 3), (65, 5), (1000, 5), (1025, 1), (2049, 7)):
        X = SR.round_in(rng.normal(0.5, 1.0, (R, K)), dtype)
        DZ = SR.round_in(rng.normal(0.0, 1.0, (R, K)), dtype)
        x, dz = P.to_dev(X, dtype, torch), P.to_dev(DZ, dtype, torch)
        for alpha in (1.0, 0.25):
            y64, cut, sigma = SR.sparse_relu(X, alpha)
            y = select.sparse_relu_fwd(x, alpha)
            assert path_of(select, torch, K, dtype, x, y) == SR.path_name(K, dtype)
            got = P.to_host(y)
            if K > 1:
                close(y, y64, dtype, (K, R, dtype, alpha))
                far = np.abs(X - cut) > 1e-3 * sigma
                assert np.array_equal((got > 0)[far], (X > cut)[far]) and (got >= 0).all()
            else:
                assert not got.any()                       # one element: it is the mean, sigma is 0
            dx = select.relu_rule_bwd(dz, y)
            assert np.array_equal(bits(P.to_host(dx)), bits(np.where(got > 0, DZ, np.float32(0))))


def test_sparse_relu_large_offset_separates_the_variance_forms(env):
    """fp32 rows of mean 1e4 and sigma 1.  E[x^2] - mean^2 in fp32 works on squares of 1e8 whose ulp is 8: its sigma is noise of the order of
    the squares' rounding, several units.  The variance around the mean works on differences of order 1: what is left is the error of the
    mean -- 1000 addends of 1e4, partial sums up to 1e7 (ulp 1), at most 16 + 6 roundings of half an ulp along any addend's path, so
    |mean error| <= 11 / 1000 -- plus one ulp of 1e4 (1e-3) in x - cut.  Bound: 0.02, far below what the other form gives."""
    torch, select = env
    rng = np.random.default_rng(77)
    K = 1000
    X = (1e4 + rng.normal(0.0, 1.0, (5, K))).astype(np.float32)
    y64, cut, sigma = SR.sparse_relu(X, 1.0)
    assert np.abs(sigma - 1).max() < 0.1
    got = P.to_host(select.sparse_relu_fwd(torch.from_numpy(X).cuda(), 1.0)).astype(np.float64)
    naive = np.sqrt(np.maximum(np.mean(X * X, axis=1, dtype=np.float32) - np.square(np.mean(X, axis=1, dtype=np.float32)), 0))
    print("large offset: max |y - y64| = %.4g, sigma of the E[x^2] form off by %.3g" % (np.abs(got - y64).max(), np.abs(naive - sigma[:, 0]).max()))
    assert np.abs(naive - sigma[:, 0]).max() > 0.1
    assert np.abs(got - y64).max() <= 0.02


@pytest.mark.parametrize("dtype", DTYPES)
def test_repeated_calls_and_both_access_forms_store_the_same_bits(env, dtype):
    """Every op twice on the same tensors, then on copies that start one element off a 16-byte boundary: the element form gives a lane the
    same elements as the 16-byte form, so all results are bit-identical."""
    torch, select = env
    td = getattr(torch, P.TORCH_DT[dtype])
    rng = np.random.default_rng(31)
    for K in (64, 1024, 2048, 4096):
        R = 5
        X, DY = SR.round_in(rng.normal(0.0, 1.0, (R, K)), dtype), SR.round_in(rng.normal(0.0, 1.0, (R, K)), dtype)
        X[:, ::3] = X[:, :1]                               # ties, so that the tie rule is part of what must repeat
        M = np.where(rng.random((R, K)) < 0.3, 0.0, 1.0).astype(np.float32)

        def off(a, t):                                     # a contiguous copy whose first element is one element past a 16-byte boundary
            buf = torch.empty(a.size + 8, dtype=t, device="cuda")
            v = buf[1:1 + a.size].view(a.shape)
            v.copy_(torch.from_numpy(a).cuda().to(t))
            assert v.data_ptr() % 16 != 0 and v.is_contiguous()
            return v

        def run(x, dy, m):
            y = select.masked_top_k_softmax_fwd(x, 17, m, 0.5)
            r = select.rectified_top_k_fwd(x, 17)
            s = select.sparse_relu_fwd(x, 0.5)
            return (y, select.masked_softmax_fwd(x, m, 0.5), select.masked_softmax_bwd(dy, y, m, 0.5), r, s, select.relu_rule_bwd(dy, s))

        x, dy, m = P.to_dev(X, dtype, torch), P.to_dev(DY, dtype, torch), torch.from_numpy(M).cuda()
        assert path_of(select, torch, K, dtype, x, dy, m).endswith("-wide")
        first, second = run(x, dy, m), run(x, dy, m)
        xo, dyo, mo = off(X, td), off(DY, td), off(M, torch.float32)
        assert not path_of(select, torch, K, dtype, xo, dyo, mo).endswith("-wide")
        third = run(xo, dyo, mo)
        iv = torch.int32 if dtype == "f32" else torch.int16
        for name, a, b, c in zip(("topk", "softmax", "grad", "rect", "sparse_relu", "relu_grad"), first, second, third):
            assert torch.equal(a.view(iv), b.view(iv)), (K, dtype, name, "repeat")
            assert torch.equal(a.view(iv), c.view(iv)), (K, dtype, name, "element form")


@pytest.mark.parametrize("dtype", DTYPES)
def test_autograd_equals_the_low_level_pairs(env, dtype):
    torch, select = env
    import blocksparse_amd as ba
    rng = np.random.default_rng(41)
    B, H, T, K = 2, 3, 5, 65
    X, G = SR.round_in(rng.normal(0.0, 1.0, (B, H, T, K)), dtype), SR.round_in(rng.normal(0.0, 1.0, (B, H, T, K)), dtype)
    m = torch.from_numpy(np.where(rng.random((1, 1, T, K)) < 0.3, 0.0, 1.0).astype(np.float32)).cuda()
    g = P.to_dev(G, dtype, torch)
    ops = (
        (lambda x: ba.rectified_top_k(x, 9), lambda x: select.rectified_top_k_fwd(x, 9), lambda y: select.rectified_top_k_bwd(g, y)),
        (lambda x: ba.rectified_top_k(x, 9, rebase=False), lambda x: select.rectified_top_k_fwd(x, 9, False), lambda y: select.relu_rule_bwd(g, y)),
        (lambda x: ba.masked_top_k_softmax(x, 9, m, 0.5), lambda x: select.masked_top_k_softmax_fwd(x, 9, m, 0.5),
         lambda y: select.masked_top_k_softmax_bwd(g, y, m, 0.5)),
        (lambda x: ba.masked_softmax(x, m, 0.5), lambda x: select.masked_softmax_fwd(x, m, 0.5), lambda y: select.masked_softmax_bwd(g, y, m, 0.5)),
        (lambda x: ba.softmax(x, 2.0), lambda x: select.masked_softmax_fwd(x, None, 2.0), lambda y: select.masked_softmax_bwd(g, y, None, 2.0)),
        (lambda x: ba.sparse_relu(x, 0.5), lambda x: select.sparse_relu_fwd(x, 0.5), lambda y: select.sparse_relu_bwd(g, y)),
    )
    for i, (op, fwd, bwd) in enumerate(ops):
        x = P.to_dev(X, dtype, torch).requires_grad_()
        y = op(x)
        y.backward(g)
        want_y = fwd(x.detach())
        assert torch.equal(y.detach(), want_y) and torch.equal(x.grad, bwd(want_y)), (dtype, i)
        assert float(x.grad.float().abs().sum()) > 0


def test_captured_forward_and_backward_replay_onto_refreshed_inputs(env):
    """One single-stream capture of every forward and backward: a replay computes from the CURRENT contents of x, dy and the mask."""
    torch, select = env
    rng = np.random.default_rng(51)
    R, K = 9, 1025
    make = lambda: (P.to_dev(SR.round_in(rng.normal(0.0, 1.0, (R, K)), "bf16"), "bf16", torch), P.to_dev(SR.round_in(rng.normal(0.0, 1.0, (R, K)), "bf16"), "bf16", torch),
                    torch.from_numpy(np.where(rng.random((1, K)) < 0.3, 0.0, 1.0).astype(np.float32)).cuda())
    (x, dy, m), (x2, dy2, m2) = make(), make()
    assert not torch.equal(x, x2) and not torch.equal(m, m2)

    def step():
        y = select.masked_top_k_softmax_fwd(x, 17, m, 0.5)
        r = select.rectified_top_k_fwd(x, 17)
        s = select.sparse_relu_fwd(x, 1.0)
        return y, select.masked_softmax_bwd(dy, y, m, 0.5), r, select.relu_rule_bwd(dy, r), s, select.relu_rule_bwd(dy, s)

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    for t, t2 in ((x, x2), (dy, dy2), (m, m2)):
        t.copy_(t2)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in outs]
    want = step()
    torch.cuda.synchronize()
    for a, w, name in zip(got, want, ("y", "dx", "rect", "drect", "srelu", "dsrelu")):
        assert torch.equal(a, w), name
    y64, _ = SR.topk_softmax(P.to_host(x2), 17, P.to_host(m2), 0.5)
    close_l2(got[0], y64, "bf16", "captured y")
