"""Memory-contract tier of the weight-update kernels (include/bsmm_optim.h), the contract of tests/test_memory_bounds_gpu.py: every tensor
a kernel may touch sits between poisoned guards (tests/_guard.py); after the call no guard byte has changed, every element of a live block
and every workspace slot of the tensor has been stored, the gated-off blocks -- poisoned in grad, mean, var, param and the average before
the call, so that no result may depend on them -- still hold their poison, and the values are those of tests/_optimize_ref.py.  The calls go
through the C ABI so that the test decides where each tensor lies: aligned (the 16-byte path) and one element off (the element path)."""
import ctypes

import numpy as np
import pytest

import _guard as GD
import _optimize_ref as OR
import _parity as P
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu
CODE = {"f32": 0, "f16": 1, "bf16": 2}
BLOCKS = 37
# bsize (0: flat, 4097 elements), gradient type, type of the working copy and of the average
CASES = [(8, "f32", "bf16"), (32, "bf16", "f16"), (64, "f16", "bf16"), (0, "bf16", "f32")]
SETTINGS = dict(grad_scale=0.5, saturate=2.0, clip_sigma=3.0)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from blocksparse_amd import _lib
    return torch, _lib, _lib.load()


def _td(torch, dtype):
    return getattr(torch, P.TORCH_DT[dtype])


@pytest.mark.parametrize("misalign", (0, 1))
@pytest.mark.parametrize("case", CASES, ids=["bs%d-%s-%s" % c for c in CASES])
def test_adam_and_ema_stay_inside(env, case, misalign):
    torch, _lib, L = env
    bs, gdt, odt = case
    n = BLOCKS * bs * bs if bs else 4097
    rng = np.random.RandomState(bs + misalign)
    g0 = orc.round_to(rng.normal(0.0, 0.1, n).astype(np.float32), gdt).astype(np.float32)
    p0, m0 = rng.normal(0.0, 0.01, n).astype(np.float32), rng.normal(0.0, 0.01, n).astype(np.float32)
    v0 = rng.uniform(0.0, 1e-2, n).astype(np.float32)
    e0 = orc.round_to(p0 + rng.normal(0.0, 0.003, n).astype(np.float32), odt).astype(np.float32)
    gate0 = OR.gate_pattern(BLOCKS, rng) if bs else None
    live = np.repeat(gate0 != 0, bs * bs) if bs else np.ones(n, dtype=bool)
    rp, rm, rv = OR.adam(p0, m0, v0, g0, 1e-3, gate=gate0, bsize=bs, norm_scale=0.7, **SETTINGS)
    re = OR.ema(e0, rp, 0.99, gate0, bs)
    poison = lambda a: np.where(live, a, np.float32(np.nan))
    arena = GD.GuardArena(torch, "cuda")
    p, m, v = (arena.place(poison(a), name, misalign) for a, name in ((p0, "param"), (m0, "mean"), (v0, "var")))
    g = arena.place(poison(g0), "grad", misalign, _td(torch, gdt))
    e = arena.place(poison(e0), "ema", misalign, _td(torch, odt))
    p16 = arena.alloc(n, _td(torch, odt if odt != "f32" else "bf16"), "param16", misalign)
    gate = arena.place(gate0, "gate", misalign) if bs else None
    ns = arena.place(np.array([0.7], dtype=np.float32), "norm_scale", misalign)
    a = _lib.BsmmAdamArgs()
    a.param, a.mean, a.var, a.grad, a.param16 = p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), p16.data_ptr()
    a.gate, a.norm_scale, a.stream = (gate.data_ptr() if bs else None), ns.data_ptr(), _lib.raw_stream(p.device)
    a.size, a.bsize, a.grad_dtype, a.param16_dtype = n, bs, CODE[gdt], CODE[odt if odt != "f32" else "bf16"]
    a.lr, a.beta1, a.beta2, a.epsilon, a.grad_scale, a.clip_sigma, a.saturate = 1e-3, 0.9, 0.999, 1e-8, 0.5, 3.0, 2.0
    _lib.check(L.bsmm_adam(ctypes.byref(a)), "bsmm_adam")
    _lib.check(L.bsmm_ema(e.data_ptr(), p.data_ptr(), gate.data_ptr() if bs else None, 0.99, n, bs, CODE[odt], a.stream), "bsmm_ema")
    arena.check()
    lv = torch.from_numpy(live).cuda()
    for t, ref, name in ((p, rp, "param"), (m, rm, "mean"), (v, rv, "var")):
        GD.assert_stored(torch, t[lv], name + " (live blocks)")
        assert GD.poisoned(torch, t[~lv]) == int((~live).sum()), name                                  # gated-off blocks: still poison
        l2, mx = P.errors(P.to_host(t)[live], ref[live])
        assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (case, misalign, name, l2, mx)
    GD.assert_stored(torch, p16[lv], "param16 (live blocks)")
    assert GD.poisoned(torch, p16[~lv]) == int((~live).sum())
    assert torch.equal(p16[lv], p[lv].to(p16.dtype))
    GD.assert_stored(torch, e[lv], "ema (live blocks)")
    assert GD.poisoned(torch, e[~lv]) == int((~live).sum())
    got, want = P.to_host(e).copy(), re.copy()
    got[~live] = want[~live] = 0.0                                                                      # (compared above: both hold the poison)
    P.assert_blocks(got, want, odt, BLOCKS if bs else 1, ctx=("ema", case, misalign))
    assert P.to_host(gate).tolist() == gate0.tolist() if bs else True
    arena.release()


@pytest.mark.parametrize("misalign", (0, 1))
def test_global_norm_stays_inside(env, misalign):
    torch, _lib, L = env
    rng = np.random.RandomState(5 + misalign)
    specs = [(37 * 64 * 64, "bf16"), (4097, "f32"), (63, "f16")]
    host = [orc.round_to(rng.normal(0.0, 0.1, n).astype(np.float32), dt).astype(np.float32) for n, dt in specs]
    arena = GD.GuardArena(torch, "cuda")
    xs = [arena.place(h, "x%d" % i, misalign, _td(torch, dt)) for i, (h, (_, dt)) in enumerate(zip(host, specs))]
    need = int(L.bsmm_sum_squared_workspace_bytes(3))
    assert need % 12 == 0
    ws = arena.alloc(need // 4, torch.float32, "workspace")
    norm, scale = arena.alloc(1, torch.float32, "norm", misalign), arena.alloc(1, torch.float32, "scale", misalign)
    st = _lib.raw_stream(ws.device)
    per = need // 12
    for i in (1, 0, 2):                                                                                 # any order: each call stores its own slots, all of them
        _lib.check(L.bsmm_sum_squared(xs[i].data_ptr(), specs[i][0], CODE[specs[i][1]], 0.5, 2.0, 0, 0, i, 3, ws.data_ptr(), need, st), "bsmm_sum_squared")
        GD.assert_stored(torch, ws[i * per:(i + 1) * per], "slots of tensor %d" % i)
        got = float(ws[i * per:(i + 1) * per].double().sum())
        want = OR.sum_squared(host[i], 0.5, 2.0)
        assert abs(got - want) <= 4e-6 * want, (i, got, want)                                           # (the sum of squares: twice the norm's 2e-6)
        if i == 1:
            assert GD.poisoned(torch, ws) == 2 * per                                                    # ... and no others
    _lib.check(L.bsmm_clip_norm(ws.data_ptr(), need, 3, 1.0, norm.data_ptr(), scale.data_ptr(), st), "bsmm_clip_norm")
    arena.check()
    want, want_scale = OR.clip([OR.sum_squared(h, 0.5, 2.0) for h in host], 1.0)
    assert abs(norm.item() - want) <= 2e-6 * want and abs(scale.item() - want_scale) <= 2e-6 * want_scale
    arena.release()
