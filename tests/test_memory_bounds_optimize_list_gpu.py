"""Memory-contract tier of the tensor-list weight update (include/bsmm_optim_list.h), the contract of
tests/test_memory_bounds_optimize_gpu.py on tests/_guard.py: every tensor of a four-row list -- bsize 8, bsize 64, flat 4097, flat 1 -- and
the table, the step state, the workspace, the norm and the scale sit between poisoned guards.  Gated-off blocks are poisoned in grad,
mean, var, param and the average beforehand (the sum of squares knows no gates: it runs with zero_nans, which turns the poison into the
zeros the reference counts).  After one sum_squared_list -> clip_norm -> advance -> adam_list -> ema_list through the C ABI no guard byte
has changed, every live element, every workspace slot of every row and the state have been stored, the gated-off blocks still hold their
poison, the table's bytes are what the host built, and the values are inside the fp32 bars against tests/_optimize_ref.py."""
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
# bsize (0: flat), flat size, gradient type, type of the working copy (None: no copy), type of the average
ROWS = [(8, 0, "f32", "bf16", "bf16"), (64, 0, "f16", "bf16", "f32"), (0, 4097, "bf16", "f16", "f16"), (0, 1, "f32", None, "f32")]
SETTINGS = dict(grad_scale=0.5, saturate=2.0, clip_sigma=3.0)
LR, DECAY, B1, B2 = 1e-3, 0.99, 0.9, 0.999


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from blocksparse_amd import _lib
    return torch, _lib, _lib.load()


def _td(torch, dtype):
    return getattr(torch, P.TORCH_DT[dtype])


@pytest.mark.parametrize("misalign", (0, 1))
def test_list_stages_stay_inside(env, misalign):
    torch, _lib, L = env
    arena = GD.GuardArena(torch, "cuda")
    rows = (_lib.BsmmOptTensor * len(ROWS))()
    host, dev = [], []
    for i, (bs, size, gdt, wdt, edt) in enumerate(ROWS):
        n = BLOCKS * bs * bs if bs else size
        rng = np.random.RandomState(10 * i + misalign)
        g0 = orc.round_to(rng.normal(0.0, 0.1, n).astype(np.float32), gdt).astype(np.float32)
        p0, m0 = rng.normal(0.0, 0.01, n).astype(np.float32), rng.normal(0.0, 0.01, n).astype(np.float32)
        v0 = rng.uniform(0.0, 1e-2, n).astype(np.float32)
        e0 = orc.round_to(p0 + rng.normal(0.0, 0.003, n).astype(np.float32), edt).astype(np.float32)
        gate0 = OR.gate_pattern(BLOCKS, rng) if bs else None
        live = np.repeat(gate0 != 0, bs * bs) if bs else np.ones(n, dtype=bool)
        poison = lambda a: np.where(live, a, np.float32(np.nan))
        tag = "row%d " % i
        p, m, v = (arena.place(poison(a), tag + name, misalign) for a, name in ((p0, "param"), (m0, "mean"), (v0, "var")))
        g = arena.place(poison(g0), tag + "grad", misalign, _td(torch, gdt))
        e = arena.place(poison(e0), tag + "ema", misalign, _td(torch, edt))
        p16 = arena.alloc(n, _td(torch, wdt), tag + "param16", misalign) if wdt else None
        gate = arena.place(gate0, tag + "gate", misalign) if bs else None
        r = rows[i]
        r.param, r.mean, r.var, r.grad, r.ema = p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), e.data_ptr()
        r.param16 = p16.data_ptr() if wdt else None
        r.gate = gate.data_ptr() if bs else None
        r.size, r.bsize, r.grad_dtype, r.param16_dtype, r.ema_dtype = n, bs, CODE[gdt], CODE[wdt] if wdt else 0, CODE[edt]
        host.append((p0, m0, v0, g0, e0, gate0, live))
        dev.append((p, m, v, g, e, p16, gate))
    cnt = len(ROWS)
    info = _lib.BsmmOptList()
    nbytes = int(L.bsmm_opt_list_bytes(cnt))
    buf = (ctypes.c_ubyte * nbytes)()
    _lib.check(L.bsmm_opt_list_build(rows, cnt, buf, nbytes, ctypes.byref(info)), "bsmm_opt_list_build")
    table0 = np.frombuffer(bytes(buf), dtype=np.uint8)
    table = arena.place(table0, "table")
    state = arena.alloc(4, torch.int32, "state", misalign)
    state[0] = 0                                                         # the caller's part: the steps taken so far; the rest stays poison
    lr = arena.place(np.array([LR], dtype=np.float32), "lr", misalign)
    need = int(L.bsmm_sum_squared_workspace_bytes(cnt))
    ws = arena.alloc(need // 4, torch.float32, "workspace")
    norm, scale = arena.alloc(1, torch.float32, "norm", misalign), arena.alloc(1, torch.float32, "scale", misalign)
    sums = [OR.sum_squared(np.where(h[6], h[3], 0.0), 0.5, 2.0) for h in host]
    want_norm, _ = OR.clip(sums, 1.0)
    clip_norm = 0.7 * want_norm
    s = _lib.BsmmAdamSettings()
    s.beta1, s.beta2, s.epsilon, s.grad_scale, s.clip_sigma, s.saturate, s.zero_infs, s.zero_nans = B1, B2, 1e-8, 0.5, 3.0, 2.0, 0, 1
    st = _lib.raw_stream(ws.device)
    pinfo = ctypes.byref(info)
    _lib.check(L.bsmm_sum_squared_list(pinfo, table.data_ptr(), 0.5, 2.0, 0, 1, ws.data_ptr(), need, st), "bsmm_sum_squared_list")
    _lib.check(L.bsmm_clip_norm(ws.data_ptr(), need, cnt, clip_norm, norm.data_ptr(), scale.data_ptr(), st), "bsmm_clip_norm")
    _lib.check(L.bsmm_opt_advance(state.data_ptr(), lr.data_ptr(), None, B1, B2, 0, st), "bsmm_opt_advance")
    _lib.check(L.bsmm_adam_list(pinfo, table.data_ptr(), state.data_ptr(), scale.data_ptr(), ctypes.byref(s), st), "bsmm_adam_list")
    _lib.check(L.bsmm_ema_list(pinfo, table.data_ptr(), DECAY, st), "bsmm_ema_list")
    arena.check()
    assert np.array_equal(table.cpu().numpy(), table0)
    # workspace, norm, scale, state
    per = need // 4 // cnt
    for i in range(cnt):
        GD.assert_stored(torch, ws[i * per:(i + 1) * per], "slots of row %d" % i)
        got = float(ws[i * per:(i + 1) * per].double().sum())
        assert abs(got - sums[i]) <= 4e-6 * sums[i], (i, got, sums[i])                                   # (the sum of squares: twice the norm's 2e-6)
    want_norm, want_scale = OR.clip(sums, clip_norm)
    assert abs(norm.item() - want_norm) <= 2e-6 * want_norm and abs(scale.item() - want_scale) <= 2e-6 * want_scale
    assert state.tolist()[0] == 1 and state.tolist()[3] == 0
    lr_t, lr_new_t = state[1:3].view(torch.float32).tolist()
    want_lr = np.float32(np.float64(np.float32(LR)) * (np.sqrt(1.0 - B2) / (1.0 - B1)))
    assert abs(lr_t - float(want_lr)) <= float(np.spacing(want_lr)) and lr_new_t == lr_t
    assert lr.item() == np.float32(LR)
    # the tensors
    allgot, allref = {"param": [], "mean": [], "var": []}, {"param": [], "mean": [], "var": []}
    for i, ((bs, size, gdt, wdt, edt), (p0, m0, v0, g0, e0, gate0, live), (p, m, v, g, e, p16, gate)) in enumerate(zip(ROWS, host, dev)):
        dead = int((~live).sum())
        assert not bs or dead >= 2 * bs * bs
        rp, rm, rv = OR.adam(p0, m0, v0, g0, lr_t, gate=gate0, bsize=bs, norm_scale=scale.item(), beta1=B1, beta2=B2, **SETTINGS)
        re = OR.ema(e0, rp, DECAY, gate0, bs)
        lv = torch.from_numpy(live).cuda()
        for t, ref, name in ((p, rp, "param"), (m, rm, "mean"), (v, rv, "var")):
            GD.assert_stored(torch, t[lv], "row %d %s (live blocks)" % (i, name))
            assert GD.poisoned(torch, t[~lv]) == dead, (i, name)                                         # gated-off blocks: still poison
            allgot[name].append(P.to_host(t)[live])
            allref[name].append(ref[live])
            if live.sum() >= 63:
                l2, mx = P.errors(P.to_host(t)[live], ref[live])
                assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (i, misalign, name, l2, mx)
        assert GD.poisoned(torch, g[~lv]) == dead and GD.poisoned(torch, g[lv]) == 0
        if wdt:
            GD.assert_stored(torch, p16[lv], "row %d param16 (live blocks)" % i)
            assert GD.poisoned(torch, p16[~lv]) == dead
            assert torch.equal(p16[lv], p[lv].to(p16.dtype))
        GD.assert_stored(torch, e[lv], "row %d ema (live blocks)" % i)
        assert GD.poisoned(torch, e[~lv]) == dead
        got, want = P.to_host(e).copy(), re.copy()
        got[~live] = want[~live] = 0.0                                                                   # (compared above: both hold the poison)
        P.assert_blocks(got, want, edt, BLOCKS if bs else 1, ctx=("ema", i, misalign))
        assert P.to_host(gate).tolist() == gate0.tolist() if bs else True
    for name in allgot:
        l2, mx = P.errors(np.concatenate(allgot[name]), np.concatenate(allref[name]))
        assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (misalign, name, l2, mx)
    arena.release()
