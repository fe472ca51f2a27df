"""GPU tier of the dynamic-sparsity operators (blocksparse_amd/sparsity.py, include/bsmm_sparsity.h) against the float64 helper
tests/_sparsity_ref.py: block norms, group-lasso decay, threshold and sparsity pruning, the feature reduce, the block-reduced weight
gradient (edge tiles, contraction tails, accumulate, scale 0, groups of 8, determinism), the planted case where the bound is tight, the
bound itself against ``exact=True``, and the relayout round trip.  Every input comes from a seeded generator."""
import functools

import numpy as np
import pytest

import _parity as P
import _sparsity_ref as SR
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f16", "bf16")
BLOCKS = 37


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import blocksparse_amd as B
    from blocksparse_amd import _lib
    _lib.load()
    return torch, B


# ---- weights ---------------------------------------------------------------------------------------------------------------------
ZERO_BLOCK, SPIKE_BLOCK = 3, 5


def _weights(bs, dtype):
    """37 blocks ~ N(0, 0.01) in the storage type; block 3 all zero, block 5 with one element 1000 x the rest."""
    rng = np.random.RandomState(1000 + bs)
    W = rng.normal(0.0, 0.01, (BLOCKS, bs, bs)).astype(np.float32)
    W[ZERO_BLOCK] = 0.0
    W[SPIKE_BLOCK, bs // 2, 1] = 10.0
    return orc.round_to(W, dtype)


def _mid_threshold(norms):
    """Midway between the two adjacent sorted norms with the widest gap in the middle third: no norm is within rounding of it (the gap is
    at least 100 fp32 roundings wide)."""
    s = np.sort(np.asarray(norms, dtype=np.float64))
    lo, hi = len(s) // 3, 2 * len(s) // 3
    j = lo + int(np.argmax(s[lo + 1:hi + 1] - s[lo:hi]))
    assert s[j + 1] - s[j] > 1e-5 * s[j + 1]
    return 0.5 * (s[j] + s[j + 1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bs", (8, 16, 32, 64))
def test_norm_decay_threshold_prune(env, bs, dtype):
    torch, B = env
    W = _weights(bs, dtype)
    w = P.to_dev(W, dtype, torch)
    # max norm: bit-equal; l2 norm: a sum of squares has no cancellation
    got_max = P.to_host(B.blocksparse_norm(w, norm="max"))
    assert np.array_equal(got_max, SR.block_norm(W, "max").astype(np.float32)), (bs, dtype)
    got_l2 = P.to_host(B.blocksparse_norm(w, norm="l2"))
    l2, _ = P.errors(got_l2, SR.block_norm(W, "l2"))
    print("l2 norm", bs, dtype, l2)
    assert l2 <= P.L2_BAR["f32"] and got_l2[ZERO_BLOCK] == 0.0
    assert torch.equal(w, P.to_dev(W, dtype, torch))                      # norms do not write the weights
    # decay, gated: gate-0 blocks bit-for-bit alone
    gate_np = (np.random.RandomState(7).rand(BLOCKS) < 0.7).astype(np.float32)
    gate_np[[0, 11]] = 0.0
    gate_np[[ZERO_BLOCK, SPIKE_BLOCK, 1]] = 1.0
    gate = torch.from_numpy(gate_np).cuda()
    for g_t, g_np in ((gate, gate_np), (None, None)):
        wd = w.clone()
        assert B.blocksparse_l2_decay(wd, gate=g_t, rate=0.05, epsilon=1e-12) is wd
        P.assert_blocks(P.to_host(wd), SR.l2_decay(W, g_np, 0.05, 1e-12), dtype, BLOCKS, ctx=("decay", bs, dtype, g_np is not None))
        if g_np is not None:
            off = torch.from_numpy(g_np == 0).cuda()
            assert torch.equal(wd[off], w[off]) and not torch.equal(wd[~off], w[~off])
    # threshold prune: every gate rewritten -- a block that was 0 comes back
    for norm in ("max", "l2"):
        norms = SR.block_norm(W, norm)
        thr = _mid_threshold(norms)
        want = SR.threshold_gate(norms, thr)
        start = 1.0 - want                                                # every gate has to flip
        assert start[SPIKE_BLOCK] == 0.0 and want[SPIKE_BLOCK] == 1.0 and want[ZERO_BLOCK] == 0.0
        g = torch.from_numpy(start.astype(np.float32)).cuda()
        assert B.blocksparse_prune(w, g, step=0, threshold=thr, norm=norm) is g
        assert np.array_equal(P.to_host(g), want), (bs, dtype, norm)


@pytest.mark.parametrize("norm", ("max", "l2"))
@pytest.mark.parametrize("bs,dtype", ((16, "bf16"), (32, "f32"), (8, "f16")))
def test_sparsity_prune(env, bs, dtype, norm):
    torch, B = env
    W = _weights(bs, dtype)
    # a tie across the cut of sparsity 0.5 (keep 19): the block of rank 19 becomes a copy of the block of rank 18
    order = np.argsort(-SR.block_norm(W, norm), kind="stable")
    a, b = int(order[18]), int(order[19])
    W[b] = W[a]
    norms = SR.block_norm(W, norm)
    assert norms[a] == norms[b]
    w = P.to_dev(W, dtype, torch)
    for sparsity, keep in ((0.5, 19), (0.9, 4), (0.0, 37)):
        want = SR.sparsity_gate(norms, sparsity)
        assert int(want.sum()) == keep
        if sparsity == 0.5:
            assert want[min(a, b)] == 1.0 and want[max(a, b)] == 0.0     # the lower index is kept first
        g = torch.full((BLOCKS,), 0.5, device="cuda")
        assert B.blocksparse_prune(w, g, step=5, sparsity=sparsity, norm=norm) is g
        assert np.array_equal(P.to_host(g), want), (bs, dtype, norm, sparsity)
    # frequency
    half = torch.full((BLOCKS,), 0.5, device="cuda")
    g = half.clone()
    B.blocksparse_prune(w, g, step=3, sparsity=0.5, norm=norm, frequency=4)
    assert torch.equal(g, half)
    B.blocksparse_prune(w, g, step=8, sparsity=0.5, norm=norm, frequency=0)
    assert torch.equal(g, half)
    B.blocksparse_prune(w, g, step=0, threshold=1.0, norm=norm, frequency=0)
    assert torch.equal(g, half)
    B.blocksparse_prune(w, g, step=8, sparsity=0.5, norm=norm, frequency=4)
    assert np.array_equal(P.to_host(g), SR.sparsity_gate(norms, 0.5))
    with pytest.raises(ValueError):
        B.blocksparse_prune(w, g, step=0)
    with pytest.raises(ValueError):
        B.blocksparse_prune(w, g, step=0, sparsity=0.5, threshold=1.0)


# ---- feature reduce and reduced dW -------------------------------------------------------------------------------------------------
GRID = [(0, bs, 264) for bs in (8, 16, 32)] + [(1, bs, 200) for bs in (8, 16, 32, 64)]
CASES = [(axis, bs, N, 3, 5, pc, dt) for axis, bs, N in GRID for pc in (1, 3, 8) for dt in ("f16", "bf16", "f32")]
CASES.append((1, 8, 200, 33, 65, 3, "bf16"))                 # more than one 32 x 32 tile each way
CASES.append((0, 8, 264, 33, 65, 3, "f16"))
CASE_IDS = ["a%d-bs%d-N%d-%dx%d-p%d-%s" % c for c in CASES]


def _acts(axis, bs, N, CB, KB, pc, dtype, seed):
    rng = np.random.RandomState(seed)
    shape = (lambda f: (f, N)) if axis == 0 else (lambda f: (N, f))
    xs = [orc.round_to(rng.normal(0.0, 0.1, shape(CB * bs)).astype(np.float32), dtype) for _ in range(pc)]
    ys = [orc.round_to(rng.normal(0.0, 0.1, shape(KB * bs)).astype(np.float32), dtype) for _ in range(pc)]
    return xs, ys


@functools.lru_cache(maxsize=None)
def _run_case(case):
    """One device run per (case, norm), shared by the reduce and the dW statements: host inputs and device outputs as NumPy arrays."""
    import torch
    import blocksparse_amd as B
    axis, bs, N, CB, KB, pc, dtype = case
    bsmm = B.BlocksparseMatMul(P.random_layout(CB, KB, 0.4, seed=3), block_size=bs, feature_axis=axis)
    xs, ys = _acts(axis, bs, N, CB, KB, pc, dtype, seed=11 * bs + pc)
    txs, tys = [P.to_dev(a, dtype, torch) for a in xs], [P.to_dev(a, dtype, torch) for a in ys]
    out = {"xs": xs, "ys": ys}
    for norm in ("max", "l2"):
        dw, xr, yr = bsmm.block_reduced_full_dw(txs, tys, norm=norm, return_reduced=True)
        assert dw.dtype == torch.float32 and tuple(dw.shape) == (CB, KB)
        rt = torch.float16 if dtype == "f16" else torch.bfloat16
        want_shape = (lambda fb: (fb, pc, N)) if axis == 0 else (lambda fb: (pc, N, fb))
        assert xr.dtype == rt and yr.dtype == rt and tuple(xr.shape) == want_shape(CB) and tuple(yr.shape) == want_shape(KB)
        if axis == 1:                                     # back to the C ABI's [feature blocks, pairs, N]
            xr, yr = xr.permute(2, 0, 1), yr.permute(2, 0, 1)
        out[norm] = (P.to_host(dw), P.to_host(xr), P.to_host(yr))
    return out


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_feature_reduce(env, case):
    axis, bs, N, CB, KB, pc, dtype = case
    res = _run_case(case)
    rd = SR.RED_DTYPE[dtype]
    for ts, fbs, which in ((res["xs"], CB, 1), (res["ys"], KB, 2)):
        got = res["max"][which]
        assert np.array_equal(got, orc.round_to(SR.feature_reduce(ts, bs, axis, "max"), rd)), (case, which)
        rep = P.block_report(res["l2"][which], SR.feature_reduce(ts, bs, axis, "l2"), rd, fbs)
        assert rep["finite"] and rep["elem_bad"] == 0 and rep["tensor_l2"] <= P.L2_BAR[rd], (case, which, rep)


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_reduced_dw(env, case):
    """Against x_red . y_red^T in float64 on the device's own reduced values.  At most 2112 non-negative terms: no cancellation; an fp32
    chain of that length sits at 1e-7."""
    for norm in ("max", "l2"):
        dw, xr, yr = _run_case(case)[norm]
        l2, _ = P.errors(dw, SR.reduced_dw(xr, yr))
        print("reduced dw", case, norm, l2)
        assert np.isfinite(dw).all() and l2 <= P.L2_BAR["f32"], (case, norm, l2)


@pytest.mark.parametrize("axis,bs,N,dtype", ((1, 32, 200, "bf16"), (0, 16, 264, "f16"), (1, 64, 200, "f32")))
def test_reduced_dw_accumulate_scale_groups_determinism(env, axis, bs, N, dtype):
    torch, B = env
    CB, KB = 3, 5
    bsmm = B.BlocksparseMatMul(np.ones((CB, KB), dtype=np.int32), block_size=bs, feature_axis=axis)
    xs, ys = _acts(axis, bs, N, CB, KB, 11, dtype, seed=77)
    txs, tys = [P.to_dev(a, dtype, torch) for a in xs], [P.to_dev(a, dtype, torch) for a in ys]
    old_np = np.random.RandomState(5).normal(0.0, 50.0, (CB, KB)).astype(np.float32)
    for norm in ("max", "l2"):
        # the device's own reduced values of the two groups (8 + 3)
        parts = []
        for sl in (slice(0, 8), slice(8, 11)):
            dw, xr, yr = bsmm.block_reduced_full_dw(txs[sl], tys[sl], norm=norm, return_reduced=True)
            if axis == 1:
                xr, yr = xr.permute(2, 0, 1), yr.permute(2, 0, 1)
            parts.append((P.to_host(dw), SR.reduced_dw(P.to_host(xr), P.to_host(yr))))
        # accumulate onto a random dw_full, in place, with a scale
        old = torch.from_numpy(old_np).cuda()
        got = bsmm.block_reduced_full_dw(txs[:8], tys[:8], scale=0.5, norm=norm, dw_full=old)
        assert got is old
        l2, _ = P.errors(P.to_host(got), 0.5 * parts[0][1] + old_np.astype(np.float64))
        assert l2 <= P.L2_BAR["f32"], ("accumulate", norm, l2)
        # scale 0 leaves dw_full bit-identical
        keep = old.clone()
        assert bsmm.block_reduced_full_dw(txs[:8], tys[:8], scale=0.0, norm=norm, dw_full=old) is old and torch.equal(old, keep)
        assert not bsmm.block_reduced_full_dw(txs[:3], tys[:3], scale=0.0, norm=norm).any()
        # 11 pairs: groups of 8 + 3, the second accumulating onto the first
        all11 = bsmm.block_reduced_full_dw(txs, tys, norm=norm)
        l2, _ = P.errors(P.to_host(all11), parts[0][1] + parts[1][1])
        assert l2 <= P.L2_BAR["f32"], ("groups", norm, l2)
        with pytest.raises(ValueError):
            bsmm.block_reduced_full_dw(txs, tys, norm=norm, return_reduced=True)
        # the same arguments give the same bits
        assert torch.equal(all11, bsmm.block_reduced_full_dw(txs, tys, norm=norm))
        assert torch.equal(torch.from_numpy(parts[0][0]).cuda(), bsmm.block_reduced_full_dw(txs[:8], tys[:8], norm=norm))


# ---- the bound and where it is tight -----------------------------------------------------------------------------------------------
# ``exact=True`` always takes the norms of an fp32 gradient (BlocksparseMatMul.block_reduced_full_dw): the fp32 bar for every activation type
EXACT_BAR = P.L2_BAR["f32"]


@pytest.mark.parametrize("axis,bs,dtype", ((1, 32, "f32"), (0, 16, "f32"), (1, 32, "bf16"), (0, 32, "f16"), (1, 64, "bf16")))
def test_planted_identity(env, axis, bs, dtype):
    """Where the bound is tight.  Every pair is non-zero in ONE minibatch column (a different one per pair), its entries are non-negative
    and the largest entry of every feature block sits at the same feature for every pair: every term of sum_p x_p y_p^T then peaks at the
    same element of a block, so max |block| = sum_p max |x_p| max |y_p| -- the reduced dW with norm="max" IS the exact max norm.  The
    values are bf16-representable, so the reduced arrays are exact for every activation type."""
    torch, B = env
    CB, KB, N, pc = 3, 5, 64, 3
    bsmm = B.BlocksparseMatMul(P.random_layout(CB, KB, 0.5, seed=1), block_size=bs, feature_axis=axis)
    rng = np.random.RandomState(21)

    def planted(fb):
        ts = []
        for p in range(pc):
            col = orc.round_to(rng.uniform(0.05, 0.5, (fb, bs)).astype(np.float32), "bf16")
            col[:, 3] = orc.round_to(rng.uniform(0.6, 1.0, fb).astype(np.float32), "bf16")     # the block's peak: feature 3 for every pair
            t = np.zeros((fb * bs, N), dtype=np.float32)
            t[:, 5 + 17 * p] = col.reshape(-1)
            ts.append(t if axis == 0 else np.ascontiguousarray(t.T))
        return ts
    xs, ys = planted(CB), planted(KB)
    txs, tys = [P.to_dev(a, dtype, torch) for a in xs], [P.to_dev(a, dtype, torch) for a in ys]
    want = SR.dense_block_norms(SR.dense_dw(xs, ys, axis), bs, "max")
    assert np.allclose(want, SR.reduced_dw(SR.feature_reduce(xs, bs, axis, "max"), SR.feature_reduce(ys, bs, axis, "max")), rtol=1e-12)
    red = P.to_host(bsmm.block_reduced_full_dw(txs, tys, norm="max"))
    exact = P.to_host(bsmm.block_reduced_full_dw(txs, tys, norm="max", exact=True))
    for name, got, ref in (("reduced vs float64", red, want), ("exact vs float64", exact, want), ("reduced vs exact", red, exact)):
        l2, _ = P.errors(got, ref)
        print("planted", axis, bs, dtype, name, l2)
        assert l2 <= P.L2_BAR["f32"], (name, l2)


# slack of reduced >= exact: max-norm of 16-bit inputs -- the reduced values are exact, only fp32 accumulation differs (1e-5); l2 -- each
# reduced factor is rounded once to its 16-bit type (relative 2^-11 fp16, 2^-8 bf16), two factors per product, doubled for headroom;
# fp32 inputs are reduced to bf16, so both of their norms carry the bf16 l2 slack
BOUND_SLACK = {("f16", "max"): 1e-5, ("bf16", "max"): 1e-5, ("f16", "l2"): 2.0 ** -10, ("bf16", "l2"): 2.0 ** -7,
               ("f32", "max"): 2.0 ** -7, ("f32", "l2"): 2.0 ** -7}


@pytest.mark.parametrize("norm", ("max", "l2"))
@pytest.mark.parametrize("axis,bs,dtype", ((1, 32, "bf16"), (0, 32, "f16"), (0, 16, "bf16"), (1, 8, "f16"), (1, 64, "bf16"), (1, 16, "f32"), (0, 8, "f32")))
def test_reduced_is_an_upper_bound_of_exact(env, axis, bs, dtype, norm):
    torch, B = env
    CB, KB, N, pc = 3, 5, 64, 3
    bsmm = B.BlocksparseMatMul(P.random_layout(CB, KB, 0.5, seed=2), block_size=bs, feature_axis=axis)
    xs, ys = _acts(axis, bs, N, CB, KB, pc, dtype, seed=300 + bs)
    txs, tys = [P.to_dev(a, dtype, torch) for a in xs], [P.to_dev(a, dtype, torch) for a in ys]
    exact = P.to_host(bsmm.block_reduced_full_dw(txs, tys, norm=norm, exact=True))
    want = SR.dense_block_norms(SR.dense_dw(xs, ys, axis), bs, norm)
    l2, _ = P.errors(exact, want)
    print("exact", axis, bs, dtype, norm, l2)
    assert exact.shape == (CB, KB) and l2 <= EXACT_BAR, l2
    red = P.to_host(bsmm.block_reduced_full_dw(txs, tys, norm=norm))
    m = BOUND_SLACK[(dtype, norm)]
    print("bound", axis, bs, dtype, norm, float((red / exact).min()), float((red / exact).max()))
    assert (red >= exact * (1.0 - m)).all(), (red, exact)
    # scale and dw_full apply to exact=True as they do to the reduced form
    old_np = np.random.RandomState(6).normal(0.0, 1.0, (CB, KB)).astype(np.float32)
    old = torch.from_numpy(old_np).cuda()
    got = bsmm.block_reduced_full_dw(txs, tys, scale=0.25, norm=norm, exact=True, dw_full=old)
    assert got is old
    l2, _ = P.errors(P.to_host(got), 0.25 * exact.astype(np.float64) + old_np)
    assert l2 <= P.L2_BAR["f32"], l2


# ---- relayout ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis,bs,dtype", ((1, 32, "bf16"), (0, 16, "f32"), (1, 16, "f16"), (0, 8, "bf16")))
def test_relayout_round_trip(env, axis, bs, dtype):
    """Drop 5 blocks, add 4: fprop through the new operator equals fprop of the old one with the dropped blocks gated off (the new
    blocks are zero).  Compared to the L2 bar: bit-equality is not guaranteed across plans."""
    torch, B = env
    N = 128
    lay = P.random_layout(8, 10, 0.4, seed=8)
    old = B.BlocksparseMatMul(lay, block_size=bs, feature_axis=axis)
    rng = np.random.RandomState(9)
    present = [tuple(ck) for ck in old.updat_list]
    absent = [(c, k) for c in range(8) for k in range(10) if not lay[c, k]]
    drop = [present[i] for i in rng.choice(len(present), 5, replace=False)]
    add = [absent[i] for i in rng.choice(len(absent), 4, replace=False)]
    new_lay = lay.copy()
    for c, k in drop:
        new_lay[c, k] = 0
    for c, k in add:
        new_lay[c, k] = 1
    W, X, _ = P.make_inputs(old.w_shape, old.i_shape(N), old.o_shape(N), dtype, seed=4)
    w, x = P.to_dev(W, dtype, torch), P.to_dev(X, dtype, torch)
    new, w2 = old.relayout(w, new_lay, init=0.0)
    assert new.blocks == old.blocks - 5 + 4 and w2.dtype == w.dtype and tuple(w2.shape) == new.w_shape and w2.is_cuda
    assert np.array_equal(P.to_host(w2), SR.relayout(W, old.updat_list, new.updat_list, 0.0))
    gate_np = np.array([0.0 if ck in drop else 1.0 for ck in present], dtype=np.float32)
    ref = P.to_host(old.fprop(x, w, gate=torch.from_numpy(gate_np).cuda()))
    got = P.to_host(new.fprop(x, w2))
    l2, _ = P.errors(got, ref)
    print("relayout", axis, bs, dtype, l2)
    assert l2 <= P.L2_BAR[dtype], l2
    _, w3 = old.relayout(w, new_lay, init=0.5)
    where = {ck: i for i, ck in enumerate(new.updat_list)}
    assert all(bool((w3[where[ck]] == 0.5).all()) for ck in add)
