"""GPU tier of the weight-update operators (include/bsmm_optim.h, blocksparse_amd/optimize.py) against tests/_optimize_ref.py.

Shapes: 37 blocks (odd, no multiple of any per-wave packing) of every block size, flat sizes 1 / 63 / 4097; the suite's gate (blocks 0 and
36 off, block 4 on, the rest on at 60 %).  Bars: three Adam steps must keep m, v and p inside the project's fp32 bars against float64
(L2 2e-6, max 2e-5) and the update p_new - p_old within 1e-5 (L2) -- simulating this arithmetic in NumPy fp32 with these inputs gives
4e-8 and 1.0e-6; the factor of ten allows for FMA contraction and a different division.  The learning rate is 1e-3 so that the three
steps move p by ~4e-4, a thousand times the fp32 rounding of p itself (p ~ 1e-2: 6e-10 per step) -- with a smaller rate the update bar
would measure the rounding of p, not the update.  No per-element ulp distances: m and p cancel.  Everything "unchanged" or "equal to
another run" is compared bit for bit."""
import functools

import numpy as np
import pytest

import _optimize_ref as OR
import _parity as P
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu

BLOCKS = 37
LR = 1e-3
SETTINGS = dict(grad_scale=0.5, saturate=2.0, clip_sigma=3.0)
NORM_SCALE = 0.7
STEPS = 3


@pytest.fixture(scope="module")
def env():
    import torch
    from blocksparse_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    _lib.load()
    return torch, _lib


def _inputs(n, gdt, seed):
    rng = np.random.RandomState(seed)
    g = rng.normal(0.0, 0.1, n).astype(np.float32)
    g[::97] *= 50.0
    g = orc.round_to(g, gdt).astype(np.float32)
    p = rng.normal(0.0, 0.01, n).astype(np.float32)
    m = rng.normal(0.0, 0.01, n).astype(np.float32)
    v = rng.uniform(0.0, 1e-2, n).astype(np.float32)
    m[::53] = 0.0
    v[::53] = 0.0
    return p, m, v, g


@functools.lru_cache(maxsize=None)
def _adam_case(bs, size, gdt):
    """Host side of one parity case, computed once and never written again: inputs, gate and the float64 state after STEPS steps."""
    n = BLOCKS * bs * bs if bs else size
    p, m, v, g = _inputs(n, gdt, 11 * bs + size)
    gate = OR.gate_pattern(BLOCKS, np.random.RandomState(bs + 1)) if bs else None
    rp, rm, rv = p, m, v
    for _ in range(STEPS):
        rp, rm, rv = OR.adam(rp, rm, rv, g, LR, gate=gate, bsize=bs, norm_scale=NORM_SCALE, **SETTINGS)
    for a in (p, m, v, g, rp, rm, rv) + ((gate,) if bs else ()):
        a.setflags(write=False)
    return p, m, v, g, gate, rp, rm, rv


def _dev(torch, a, dtype="f32", shape=None, misalign=0):
    """A device copy of ``a``; misalign = 1: a view that starts one element into a larger allocation (the element path)."""
    t = torch.from_numpy(np.array(a, dtype=np.float32)).cuda().to(getattr(torch, P.TORCH_DT[dtype]))
    if misalign:
        big = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
        big[misalign:misalign + t.numel()].copy_(t)
        t = big[misalign:misalign + t.numel()]
        assert t.data_ptr() % 16 != 0
    return t.view(shape) if shape is not None else t


def _check_parity(torch, bs, size, gdt, misalign, p16dt="bf16"):
    from blocksparse_amd import adam_step
    p0, m0, v0, g0, gate0, rp, rm, rv = _adam_case(bs, size, gdt)
    shape = (BLOCKS, bs, bs) if bs else None
    p, m, v = (_dev(torch, a, shape=shape, misalign=misalign) for a in (p0, m0, v0))
    g = _dev(torch, g0, gdt, shape, misalign)
    p16 = _dev(torch, np.full(p0.shape, 7.0), p16dt, shape, misalign)
    gate = torch.from_numpy(np.array(gate0)).cuda() if bs else None
    ns = torch.full((1,), NORM_SCALE, device="cuda")
    versions = [t._version for t in (p, m, v, p16)]
    for _ in range(STEPS):
        adam_step(p, g, m, v, LR, gate=gate, norm_scale=ns, param16=p16, **SETTINGS)
    assert all(t._version > old for t, old in zip((p, m, v, p16), versions))
    ctx = (bs, size, gdt, misalign)
    for name, got, ref in (("m", m, rm), ("v", v, rv), ("p", p, rp)):
        l2, mx = P.errors(P.to_host(got).reshape(-1), ref)
        print("adam %s %s: L2 %.3e max %.3e" % (ctx, name, l2, mx))
        assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (ctx, name, l2, mx)
    upd = P.to_host(p).reshape(-1).astype(np.float64) - p0
    l2, _ = P.errors(upd, rp - p0)
    print("adam %s update: L2 %.3e" % (ctx, l2))
    assert l2 <= 1e-5, (ctx, "update", l2)
    live = np.ones(p0.size, dtype=bool) if gate0 is None else np.repeat(gate0 != 0, bs * bs)
    assert live.sum() > 0 and (gate0 is None or (~live).sum() >= 2 * bs * bs)
    # gated-off blocks keep their bits in every tensor; the working copy of the others is param rounded once
    for got, old in ((p, p0), (m, m0), (v, v0), (p16, np.full(p0.shape, 7.0, dtype=np.float32))):
        assert np.array_equal(P.to_host(got).reshape(-1)[~live], old[~live]), ctx
    lv = torch.from_numpy(live).cuda()
    assert torch.equal(p16.reshape(-1)[lv], p.reshape(-1).to(p16.dtype)[lv]), ctx


@pytest.mark.parametrize("gdt", ("f32", "f16", "bf16"))
@pytest.mark.parametrize("bs", (8, 16, 32, 64))
def test_adam_parity_blocks(env, bs, gdt):
    _check_parity(env[0], bs, 0, gdt, 0, "f16" if gdt == "f16" else "bf16")


@pytest.mark.parametrize("misalign", (0, 1))
@pytest.mark.parametrize("size", (1, 63, 4097))
def test_adam_parity_flat(env, size, misalign):
    for gdt in ("f32", "bf16"):
        _check_parity(env[0], 0, size, gdt, misalign)


def test_adam_parity_blocks_element_path(env):
    _check_parity(env[0], 16, 0, "f16", 1)


# ---------------------------------------------------------------------------------------------------------------- exact properties
def _state(torch, bs, gdt="bf16", seed=5):
    p0, m0, v0, g0 = _inputs(BLOCKS * bs * bs, gdt, seed)
    shape = (BLOCKS, bs, bs)
    return [_dev(torch, a, shape=shape) for a in (p0, m0, v0)], _dev(torch, g0, gdt, shape)


def _run(torch, bs, g=None, gdt="bf16", p16dt=None, lr=LR, **kw):
    """One step from the standard state; returns (p, m, v[, p16])."""
    from blocksparse_amd import adam_step
    (p, m, v), g_std = _state(torch, bs, gdt)
    p16 = torch.full((BLOCKS, bs, bs), 7.0, device="cuda", dtype=getattr(torch, P.TORCH_DT[p16dt])) if p16dt else None
    adam_step(p, g_std if g is None else g, m, v, lr, param16=p16, **kw)
    return (p, m, v) + ((p16,) if p16dt else ())


@pytest.mark.parametrize("bs", (8, 32))
def test_lr_select_steps_selected_blocks_at_lr_new(env, bs):
    torch, _ = env
    sel_np = (np.random.RandomState(3).rand(BLOCKS) < 0.4).astype(np.float32)
    sel_np[1], sel_np[2] = 1.0, 0.0
    sel = torch.from_numpy(sel_np).cuda()
    gate = torch.from_numpy(OR.gate_pattern(BLOCKS, np.random.RandomState(bs + 1))).cuda()
    mixed = _run(torch, bs, gate=gate, lr_select=sel, lr_new=5e-3, **SETTINGS)
    at_lr = _run(torch, bs, gate=gate, **SETTINGS)
    at_new = _run(torch, bs, gate=gate, lr=5e-3, **SETTINGS)
    on = sel != 0
    for a, b, c in zip(mixed, at_lr, at_new):
        assert torch.equal(a[on], c[on]) and torch.equal(a[~on], b[~on])
    assert not torch.equal(mixed[0][on & (gate != 0)], at_lr[0][on & (gate != 0)])        # (the two rates do differ)


@pytest.mark.parametrize("bs", (8, 64))
def test_norm_scale_zero_stores_nothing(env, bs):
    torch, _ = env
    (p0, m0, v0), _g = _state(torch, bs)
    zero = torch.zeros(1, device="cuda")
    got = _run(torch, bs, p16dt="bf16", norm_scale=zero, **SETTINGS)
    for a, b in zip(got, (p0, m0, v0, torch.full_like(got[3], 7.0))):
        assert torch.equal(a, b)


@pytest.mark.parametrize("gdt", ("f32", "f16", "bf16"))
def test_zero_infs_and_nans_equal_planted_zeros(env, gdt):
    torch, _ = env
    bs = 16
    (_p, _m, _v), g = _state(torch, bs, gdt)
    bad, zeroed = g.clone().view(-1), g.clone().view(-1)
    idx = torch.tensor([0, 5, 255, 256, 1000, 5000, BLOCKS * bs * bs - 1], device="cuda")
    vals = torch.tensor([float("inf"), float("-inf"), float("nan"), float("inf"), float("nan"), float("-inf"), float("nan")], device="cuda")
    bad[idx] = vals.to(bad.dtype)
    zeroed[idx] = 0
    a = _run(torch, bs, g=bad.view_as(g), gdt=gdt, zero_infs=True, zero_nans=True, clip_sigma=3.0, grad_scale=0.5)
    b = _run(torch, bs, g=zeroed.view_as(g), gdt=gdt, clip_sigma=3.0, grad_scale=0.5)
    for x, y in zip(a, b):
        assert torch.equal(x, y) and bool(torch.isfinite(x).all())
    c = _run(torch, bs, g=bad.view_as(g), gdt=gdt, clip_sigma=3.0, grad_scale=0.5)              # without the flags the planted values do arrive
    assert not bool(torch.isfinite(c[0]).all())


@pytest.mark.parametrize("p16dt", ("f16", "bf16"))
def test_param16_is_param_rounded_once(env, p16dt):
    torch, _ = env
    for bs in (8, 32):
        p, m, v, p16 = _run(torch, bs, p16dt=p16dt, **SETTINGS)
        assert torch.equal(p16, p.to(p16.dtype))


def test_identical_calls_give_identical_bits(env):
    torch, _ = env
    gate = torch.from_numpy(OR.gate_pattern(BLOCKS, np.random.RandomState(9))).cuda()
    for bs in (8, 32):
        a = _run(torch, bs, p16dt="bf16", gate=gate, **SETTINGS)
        b = _run(torch, bs, p16dt="bf16", gate=gate, **SETTINGS)
        for x, y in zip(a, b):
            assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------------------- moving average
@pytest.mark.parametrize("edt", ("f32", "f16", "bf16"))
@pytest.mark.parametrize("bs", (8, 32, 0))
def test_ema(env, bs, edt):
    torch, _ = env
    from blocksparse_amd import ema_step
    n = BLOCKS * bs * bs if bs else 4097
    rng = np.random.RandomState(17 + bs)
    p0 = rng.normal(0.0, 0.01, n).astype(np.float32)
    e0 = orc.round_to(p0 + rng.normal(0.0, 0.003, n).astype(np.float32), edt).astype(np.float32)
    gate0 = OR.gate_pattern(BLOCKS, rng) if bs else None
    shape = (BLOCKS, bs, bs) if bs else None
    for misalign in (0, 1):
        p, e = _dev(torch, p0, shape=shape, misalign=misalign), _dev(torch, e0, edt, shape, misalign)
        version = e._version
        ema_step(e, p, 0.99, gate=torch.from_numpy(gate0).cuda() if bs else None)
        assert e._version > version
        got = P.to_host(e).reshape(-1)
        P.assert_blocks(got, OR.ema(e0, p0, 0.99, gate0, bs), edt, BLOCKS if bs else 1, ctx=("ema", bs, edt, misalign))
        if bs:
            off = np.repeat(gate0 == 0, bs * bs)
            assert np.array_equal(got[off], e0[off]) and not np.array_equal(got[~off], e0[~off])


# ---------------------------------------------------------------------------------------------------------------- global norm
NORM_SIZES = (1, 63, 4097, 37 * 1024 + 3, 300001)


@functools.lru_cache(maxsize=None)
def _norm_input(size, dt):
    x = orc.round_to(np.random.RandomState(size % 1000 + len(dt)).normal(0.0, 0.1, size).astype(np.float32), dt).astype(np.float32)
    x.setflags(write=False)
    return x, OR.sum_squared(x, 0.5)


@pytest.mark.parametrize("dt", ("f32", "f16", "bf16"))
@pytest.mark.parametrize("size", NORM_SIZES)
def test_global_norm_one_tensor(env, size, dt):
    torch, _ = env
    from blocksparse_amd import clip_by_global_norm, global_norm
    x, ss = _norm_input(size, dt)
    want, _ = OR.clip([ss], 1.0)
    norms = []
    for misalign in (0, 1):
        t = _dev(torch, x, dt, misalign=misalign)
        for clip_norm in (want * 0.25, want * 4.0):
            norm, scale = clip_by_global_norm([t], clip_norm=clip_norm, grad_scale=0.5)
            again = clip_by_global_norm([t], clip_norm=clip_norm, grad_scale=0.5)
            assert norm.dtype == torch.float32 and norm.dim() == 0 and norm.is_cuda and scale.is_cuda
            n32, s32 = np.float32(norm.item()), np.float32(scale.item())
            assert n32 == np.float32(again[0].item()) and s32 == np.float32(again[1].item())              # repeated calls: the same bits
            print("norm size %d %s misalign %d: rel %.3e" % (size, dt, misalign, abs(float(n32) - want) / want))
            assert abs(float(n32) - want) <= 2e-6 * want, (size, dt, misalign, float(n32), want)
            assert s32 == np.float32(clip_norm) / max(n32, np.float32(clip_norm))                            # IEEE division: exact
            norms.append(float(n32))
        assert np.float32(global_norm([t], grad_scale=0.5).item()) == np.float32(norms[-1])
    assert abs(norms[0] - norms[-1]) <= 2e-6 * want


@pytest.mark.parametrize("cnt", (3, 70))
def test_global_norm_many_tensors(env, cnt):
    torch, _ = env
    from blocksparse_amd import clip_by_global_norm
    dts = ("f32", "f16", "bf16")
    sizes = (4097, 63, 37 * 1024 + 3) if cnt == 3 else tuple(1 + (7 * i) % 40 for i in range(cnt))
    host = [_norm_input(s, dts[i % 3]) for i, s in enumerate(sizes)]
    want, want_scale = OR.clip([ss for _, ss in host], 1.0)
    ts = [_dev(torch, x, dts[i % 3], misalign=i % 2) for i, (x, _) in enumerate(host)]
    norm, scale = clip_by_global_norm(ts, clip_norm=1.0, grad_scale=0.5)
    again = clip_by_global_norm(ts, clip_norm=1.0, grad_scale=0.5)
    assert torch.equal(norm, again[0]) and torch.equal(scale, again[1])
    assert abs(norm.item() - want) <= 2e-6 * want, (cnt, norm.item(), want)
    assert abs(scale.item() - want_scale) <= 2e-6 * want_scale


@pytest.mark.parametrize("dt", ("f32", "bf16"))
def test_global_norm_with_a_planted_inf(env, dt):
    torch, _ = env
    from blocksparse_amd import clip_by_global_norm
    x, _ = _norm_input(4097, dt)
    bad = np.array(x)
    bad[[7, 4096]] = np.inf, -np.inf
    bad[100] = np.nan
    ts = [_dev(torch, _norm_input(63, dt)[0], dt), _dev(torch, bad, dt)]
    norm, scale = clip_by_global_norm(ts, clip_norm=1.0)
    assert scale.item() == 0.0 and not np.isfinite(norm.item())
    norm, scale = clip_by_global_norm(ts, clip_norm=1.0, zero_infs=True, zero_nans=True)
    fin = np.array(bad)
    fin[~np.isfinite(fin)] = 0.0
    want, want_scale = OR.clip([OR.sum_squared(_norm_input(63, dt)[0]), OR.sum_squared(fin)], 1.0)
    assert abs(norm.item() - want) <= 2e-6 * want and abs(scale.item() - want_scale) <= 2e-6 * want_scale


# ---------------------------------------------------------------------------------------------------------------- capture
def test_captured_step_equals_the_eager_sequence(env):
    """clip -> Adam (with a bf16 working copy) -> moving average recorded in one graph on one stream; three replays with new gradients in
    the static buffer, the second holding an Inf.  Each replay leaves the bits of the eager sequence; the Inf replay leaves param, moments
    and working copy as they were (the average still moves towards the unchanged param, as it does eagerly)."""
    torch, _ = env
    from blocksparse_amd import adam_step, clip_by_global_norm, ema_step
    bs = 32
    gate = torch.from_numpy(OR.gate_pattern(BLOCKS, np.random.RandomState(2))).cuda()
    grads = []
    for i in range(3):
        g = _inputs(BLOCKS * bs * bs, "bf16", 40 + i)[3]
        if i == 1:
            g[12345] = np.inf
        grads.append(_dev(torch, g, "bf16", (BLOCKS, bs, bs)))

    def fresh():
        (p, m, v), _g = _state(torch, bs)
        return dict(p=p, m=m, v=v, p16=p.to(torch.bfloat16), e=p.clone(), g=torch.zeros_like(grads[0]))

    def sequence(s):
        _norm, scale = clip_by_global_norm([s["g"]], clip_norm=1.0)
        adam_step(s["p"], s["g"], s["m"], s["v"], LR, gate=gate, norm_scale=scale, param16=s["p16"], clip_sigma=3.0)
        ema_step(s["e"], s["p"], 0.99, gate=gate)

    eager, cap = fresh(), fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                         # first-call host work stays out of the capture
        sequence(fresh())
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sequence(cap)
    torch.cuda.synchronize()
    keys = ("p", "m", "v", "p16", "e")
    start = fresh()
    for k in keys:                                        # (capturing ran nothing)
        assert torch.equal(cap[k], start[k]), k
    for i, g in enumerate(grads):
        before = {k: cap[k].clone() for k in keys}
        cap["g"].copy_(g)
        graph.replay()
        eager["g"].copy_(g)
        sequence(eager)
        torch.cuda.synchronize()
        for k in keys:
            assert torch.equal(cap[k], eager[k]), (i, k)
        changed = [k for k in keys if not torch.equal(cap[k], before[k])]
        if i == 1:
            assert all(torch.equal(cap[k], before[k]) for k in ("p", "m", "v", "p16")), changed
        else:
            assert set(changed) == set(keys), changed


# ---------------------------------------------------------------------------------------------------------------- caches
def _f32_operator(env):
    """bsize 32, feature axis 1, fp32 with the plan forced (the caller sets the kernel variant): the kernel that multiplies with prepared
    bf16 pieces of W, cached per weights version -- the construction of tests/test_host_state_gpu.py."""
    torch, lib = env
    from blocksparse_amd import BlocksparseMatMul
    lay = P.random_layout(40, 40, 0.2, seed=5)
    b = BlocksparseMatMul(lay, block_size=32, feature_axis=1)
    gen = P.gen(torch, 2)
    w = torch.randn(b.w_shape, device="cuda", generator=gen) * 0.05
    x = torch.randn(b.i_shape(256), device="cuda", generator=gen) * 0.1
    dw = torch.randn(b.w_shape, device="cuda", generator=gen) * 0.1
    return lay, b, w, x, dw


def _fprop_follows(env, mutate):
    torch, lib = env
    lib.set_kernel_variant(3)
    try:
        lay, b, w, x, dw = _f32_operator(env)
        y0 = b.fprop(x, w)
        assert lib.last_kernel() == lib.K_XCOL32_F32SPLIT and lib.OP_FPROP in b._prepared_w and b._prepared_w[lib.OP_FPROP][0]() is w      # else: vacuous
        w_old, version = w.clone(), w._version
        mutate(w, dw)
        torch.cuda.synchronize()
        assert not torch.equal(w, w_old)
        assert w._version > version, "a write through the C ABI must move the version counter"
        y1 = b.fprop(x, w)
        assert lib.last_kernel() == lib.K_XCOL32_F32SPLIT
        t = orc.build_layout_luts(lay, 32)
        ref = orc.fprop_fast(t, P.to_host(x).astype(np.float64), P.to_host(w).astype(np.float64), 1, np.float64)
        l2, mx = P.errors(P.to_host(y1), ref)
        stale, _ = P.errors(P.to_host(y0), ref)
        print("fprop after the write: L2 %.3e (the result of the old weights: %.3e)" % (l2, stale))
        assert stale > 1e-3                                    # (the write moved the result far beyond the bar: a stale cache cannot pass)
        assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (l2, mx)
    finally:
        lib.set_kernel_variant(0)


def test_fprop_after_an_optimizer_step_uses_the_stepped_weights(env):
    torch, lib = env

    def step(w, dw):
        from blocksparse_amd import AdamOptimizer
        w.grad = dw
        opt = AdamOptimizer([w], learning_rate=1e-2)
        opt.step()
        assert opt.steps == 1 and float(opt.get_slot(w, "Var").abs().sum()) > 0
    _fprop_follows(env, step)


def test_fprop_after_l2_decay_uses_the_decayed_weights(env):
    def decay(w, dw):
        from blocksparse_amd import blocksparse_l2_decay
        blocksparse_l2_decay(w, rate=0.5)
    _fprop_follows(env, decay)


def test_prune_moves_the_gate_version(env):
    torch, lib = env
    from blocksparse_amd import blocksparse_prune
    w = torch.randn(BLOCKS, 8, 8, device="cuda", generator=P.gen(torch, 1))
    for kw in (dict(sparsity=0.5), dict(threshold=2.5)):
        gate = torch.ones(BLOCKS, device="cuda")
        version = gate._version
        blocksparse_prune(w, gate, 0, **kw)
        assert gate._version > version and 0 < float(gate.sum()) < BLOCKS


# ---------------------------------------------------------------------------------------------------------------- the classes
def test_optimizer_and_ema_classes(env):
    """AdamOptimizer over a gated block-sparse weight and a flat bias: three steps against the float64 reference with the host step-size
    correction; the working copies; a state_dict round trip; new blocks at their own rate; Ema keyed by param."""
    torch, lib = env
    from blocksparse_amd import AdamOptimizer, Ema, optimize
    bs = 16
    p0, b0 = _inputs(BLOCKS * bs * bs, "f32", 77)[0], _inputs(63, "f32", 78)[0]
    # plain N(0, 0.1) gradients: the moments start at zero here, so v is (1 - beta2) g^2 with no floor under it, and MAX_BAR is max|diff| over
    # mean|ref| -- the x 50 outliers of _inputs() would put single elements of v thousands of times above that mean, where half an fp32 ulp
    # of the element itself (6e-8 relative) already exceeds 2e-5 of the mean.  The parity tests above keep the outliers (their v has a floor).
    rs = np.random.RandomState(79)
    g0, gb0 = rs.normal(0.0, 0.1, p0.size).astype(np.float32), rs.normal(0.0, 0.1, 63).astype(np.float32)
    gate0 = OR.gate_pattern(BLOCKS, np.random.RandomState(4))
    sel0 = np.zeros(BLOCKS, dtype=np.float32)
    sel0[[4, 9]] = 1.0
    w, bias = _dev(torch, p0, shape=(BLOCKS, bs, bs)), _dev(torch, b0)
    w.gate = torch.from_numpy(gate0).cuda()
    w.grad, bias.grad = _dev(torch, g0, shape=(BLOCKS, bs, bs)), _dev(torch, gb0)
    opt = AdamOptimizer([w, bias], learning_rate=LR, clip_sigmas=3.0, gated=True, working_dtype=torch.bfloat16)
    ema = Ema(0.99, gated=True)
    assert torch.equal(opt.working_copy(w), w.to(torch.bfloat16)) and ema.average(w) is None
    rw, rm, rv = p0, np.zeros_like(p0), np.zeros_like(p0)
    rb, rbm, rbv = b0, np.zeros_like(b0), np.zeros_like(b0)
    re_w = p0.astype(np.float64)
    for t in range(1, 4):
        sel = {0: torch.from_numpy(sel0).cuda()} if t == 3 else None
        opt.step(lr_select=sel, lr_new=5 * LR if sel else None)
        ema.apply([w, bias])
        c = optimize.lr_correction(t, 0.9, 0.999)
        rw, rm, rv = OR.adam(rw, rm, rv, g0, LR * c, gate=gate0, bsize=bs, clip_sigma=3.0, lr_select=sel0 if sel else None, lr_new=5 * LR * c)
        rb, rbm, rbv = OR.adam(rb, rbm, rbv, gb0, LR * c, clip_sigma=3.0)
        re_w = OR.ema(rw if t == 1 else re_w, rw, 0.99, gate0, bs)          # (an average starts as a copy of its param at the first apply)
    assert opt.steps == 3
    for got, ref in ((w, rw), (opt.get_slot(w, "Mean"), rm), (opt.get_slot(w, "Var"), rv), (bias, rb), (opt.get_slot(bias, "Var"), rbv)):
        l2, mx = P.errors(P.to_host(got).reshape(-1), ref)
        print("classes, %d elements: L2 %.3e max %.3e" % (ref.size, l2, mx))
        assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (l2, mx)
    live = torch.from_numpy(gate0 != 0).cuda()
    assert torch.equal(opt.working_copy(w)[live], w.to(torch.bfloat16)[live]) and torch.equal(opt.working_copy(bias), bias.to(torch.bfloat16))
    assert P.errors(P.to_host(ema.average(w)).reshape(-1), re_w)[0] <= P.L2_BAR["f32"] and ema.average(bias).shape == bias.shape
    state = opt.state_dict()
    other = AdamOptimizer([w.clone(), bias.clone()], learning_rate=LR)
    other.load_state_dict(state)
    assert other.steps == 3 and torch.equal(other.slots[0]["Mean"], opt.slots[0]["Mean"]) and torch.equal(other.slots[1]["Var"], opt.slots[1]["Var"])
    with pytest.raises(ValueError):
        optimize.adam_step(bias, bias.grad, opt.slots[1]["Mean"], opt.slots[1]["Var"], LR, gate=w.gate)      # a flat tensor takes no gate
