"""Memory-contract tier of the Adafactor kernels (include/bsmm_adafactor.h), the contract of tests/test_memory_bounds_optimize_gpu.py: every
tensor a kernel may touch sits between poisoned guards (tests/_guard.py); after the call no guard byte has changed and every element of
param, param16, cv and rv of a live block or row has been stored.  The workspace is all NaN before the call and the results are finite and
equal to the reference: every slot the call read, the call itself had stored.  The gated-off blocks -- poisoned in grad, param, cv and rv
before the call, so that no result may depend on them -- still hold their poison.  Values are those of tests/_adafactor_ref.py.  The calls
go through the C ABI so that the test decides where each tensor lies: aligned (the 16-byte path) and one element off (the element path)."""
import ctypes

import numpy as np
import pytest

import _adafactor_ref as AR
import _guard as GD
import _optimize_ref as OR
import _parity as P
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu
CODE = {"f32": 0, "f16": 1, "bf16": 2}
BLOCKS = 37
# form, rows, cols / bsize, gradient type, type of the working copy
CASES = [("2d", 33, 1028, "bf16", "f16"), ("1d", 1, 4100, "f16", "bf16"), ("block", BLOCKS, 32, "bf16", "bf16"), ("block", BLOCKS, 8, "f32", "f16")]
KW = dict(lr=1e-3, decay=0.75, grad_scale=0.5, saturate=2.0, norm_scale=0.7)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    from blocksparse_amd import _lib
    return torch, _lib, _lib.load()


def _td(torch, dtype):
    return getattr(torch, P.TORCH_DT[dtype])


@pytest.mark.parametrize("misalign", (0, 1))
@pytest.mark.parametrize("case", CASES, ids=["%s-%dx%d-%s-%s" % c for c in CASES])
def test_adafactor_stays_inside(env, case, misalign):
    torch, _lib, L = env
    form, rows, second, gdt, odt = case
    bs = second if form == "block" else 0
    cols = bs * bs if bs else second
    n, ncv, nrv = rows * cols, (rows * bs if bs else cols), (rows * bs if bs else (rows if form == "2d" else 0))
    rng = np.random.RandomState(rows + second + misalign)
    g0 = rng.normal(0.0, 0.1, n).astype(np.float32)
    g0[::97] *= 50.0
    g0 = orc.round_to(g0, gdt).astype(np.float32)
    p0 = rng.normal(0.0, 0.01, n).astype(np.float32)
    cv0, rv0 = rng.uniform(0.0, 1e-2, ncv).astype(np.float32), rng.uniform(0.0, 1e-2, max(nrv, 1)).astype(np.float32)
    gate0 = OR.gate_pattern(rows, rng) if bs else None
    live = np.repeat(gate0 != 0, cols) if bs else np.ones(n, dtype=bool)
    ls = np.repeat(gate0 != 0, bs) if bs else None
    if bs:
        rp, rcv, rrv, _ = AR.blocks(p0, cv0, rv0, g0, rows, bs, gate=gate0, **KW)
    else:
        rp, rcv, rrv, _ = AR.dense(p0, cv0, rv0 if nrv else None, g0, rows, cols, **KW)
    poison = lambda a, mask: a if mask is None else np.where(mask, a, np.float32(np.nan))
    arena = GD.GuardArena(torch, "cuda")
    p = arena.place(poison(p0, live if bs else None), "param", misalign)
    g = arena.place(poison(g0, live if bs else None), "grad", misalign, _td(torch, gdt))
    cv = arena.place(poison(cv0, ls), "cv", misalign)
    rv = arena.place(poison(rv0, ls), "rv", misalign) if nrv else None
    p16 = arena.alloc(n, _td(torch, odt), "param16", misalign)
    gate = arena.place(gate0, "gate", misalign) if bs else None
    ns = arena.place(np.array([KW["norm_scale"]], dtype=np.float32), "norm_scale", misalign)
    need = int(L.bsmm_adafactor_workspace_bytes(rows, cols, bs))
    assert need > 0 and need % 4 == 0
    ws = arena.alloc(need // 4, torch.float32, "workspace", misalign)                     # all NaN: nothing may be read before it is stored
    a = _lib.BsmmAdafactorArgs()
    a.param, a.cv, a.grad, a.param16 = p.data_ptr(), cv.data_ptr(), g.data_ptr(), p16.data_ptr()
    a.rv = rv.data_ptr() if nrv else None
    a.gate, a.norm_scale = (gate.data_ptr() if bs else None), ns.data_ptr()
    a.workspace, a.workspace_bytes, a.stream = ws.data_ptr(), need, _lib.raw_stream(p.device)
    a.rows, a.cols, a.bsize, a.grad_dtype, a.param16_dtype = rows, cols, bs, CODE[gdt], CODE[odt]
    a.lr, a.decay, a.epsilon, a.clip_thresh, a.grad_scale, a.saturate = KW["lr"], KW["decay"], 1e-30, 1.0, KW["grad_scale"], KW["saturate"]
    _lib.check(L.bsmm_adafactor(ctypes.byref(a)), "bsmm_adafactor")
    arena.check()
    lv = torch.from_numpy(live).cuda()
    checks = [(p, rp, "param", live), (cv, rcv, "cv", ls)] + ([(rv, rrv, "rv", ls)] if nrv else [])
    for t, ref, name, mask in checks:
        mask = np.ones(t.numel(), dtype=bool) if mask is None else mask
        m = torch.from_numpy(mask).cuda()
        GD.assert_stored(torch, t[m], name + " (live)")                                  # stored, finite: no NaN of the workspace arrived
        assert GD.poisoned(torch, t[~m]) == int((~mask).sum()), name                     # gated-off blocks: still poison
        got = P.to_host(t)[mask]
        if name == "param":
            l2, mx = P.errors(got, ref[mask])
            assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (case, misalign, name, l2, mx)
        else:
            rel = float(np.max(np.abs(got.astype(np.float64) - ref[mask]) / ref[mask]))
            assert rel <= 2e-5, (case, misalign, name, rel)
    GD.assert_stored(torch, p16[lv], "param16 (live)")
    assert GD.poisoned(torch, p16[~lv]) == int((~live).sum())
    assert torch.equal(p16[lv], p[lv].to(p16.dtype))
    assert GD.poisoned(torch, g[~lv]) == int((~live).sum())
    assert P.to_host(gate).tolist() == gate0.tolist() if bs else True
    arena.release()
