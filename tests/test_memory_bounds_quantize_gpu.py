"""Memory-contract tier of the simulated float formats (include/bsmm_quant.h), the contract of tests/test_memory_bounds_select_gpu.py: every
tensor a kernel may touch sits between poisoned guards (tests/_guard.py) and the outputs are poisoned; after each call no guard byte has
changed, every output element has been stored, and the values are the definition's.  The calls go through the C ABI so that the test decides
where each tensor lies: aligned placements and placements 2 and 4 bytes off (the kernels pick 16-byte or element accesses from the pointers;
fp32 tensors move by one element).  Sizes sit around each unit boundary; the workspace and stats_out are poisoned; the exponent word lies
between guards of its own."""
import ctypes

import numpy as np
import pytest

import _guard as GD
import _parity as P
import _quantize_ref as QR

pytestmark = pytest.mark.gpu
CODE = {"f32": 0, "f16": 1, "bf16": 2}
SIZES = [1, 7, 8, 9, 31, 32, 33, 2047, 2048, 2049, 3 * 2048 + 8]
CASES = [(n, d, off) for n in SIZES for d in ("f32", "bf16") for off in (0, 2, 4) if not (d == "f32" and off == 2)]
SEED = 77


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from blocksparse_amd import _lib, quantize
    return torch, _lib, _lib.load(), quantize


def _values(n, dtype, seed):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=n) * np.exp(rng.uniform(-10.0, 6.0, n))).astype(np.float32)
    if n > 40:
        x[5], x[6], x[33] = np.inf, 0.0, -np.inf
    if dtype == "bf16":
        return QR.to_bf16(x)
    return x.astype(np.float16).astype(np.float32) if dtype == "f16" else x


@pytest.mark.parametrize("case", CASES, ids=["n%d-%s-off%d" % c for c in CASES])
def test_quantize_entry_points_stay_inside(env, case):
    torch, _lib, L, Q = env
    n, dtype, off = case
    td = getattr(torch, P.TORCH_DT[dtype])
    mis = off // (4 if dtype == "f32" else 2)
    X = _values(n, dtype, n + off)
    arena = GD.GuardArena(torch, "cuda")
    x = arena.place(X, "x", mis, td)
    state = arena.place(np.array([SEED, 9], dtype=np.int64), "state")
    emax = arena.place(np.array([8], dtype=np.int32), "emax")
    stream = _lib.raw_stream(x.device)
    need = int(L.bsmm_quant_workspace_bytes(n))
    ws = arena.alloc(need // 8, torch.float64, "workspace")
    spec = Q.QuantizeSpec(4, 3, 8, stochastic=2, bias_pad=1)
    args = lambda s: Q._args(s, CODE[dtype], x.device, workspace=ws)
    # out of place (the output with the input's misalignment, and aligned), in place, and the block-scaled mode where n allows it
    y_off, y_al = arena.alloc(n, td, "y_off", mis), arena.alloc(n, td, "y_aligned", 0)
    inplace = arena.place(X, "inplace", mis, td)
    a = args(spec)
    for y in (y_off, y_al, inplace):
        src = inplace if y is inplace else x
        _lib.check(L.bsmm_quantize(src.data_ptr(), y.data_ptr(), state.data_ptr(), emax.data_ptr(), n, ctypes.byref(a)), "bsmm_quantize")
    gspec = Q.QuantizeSpec(4, 3, 8, group=32, bias_pad=0)
    y_group = None
    if n % 32 == 0:
        y_group = arena.alloc(n, td, "y_group", mis)
        ag = args(gspec)
        _lib.check(L.bsmm_quantize(x.data_ptr(), y_group.data_ptr(), None, None, n, ctypes.byref(ag)), "bsmm_quantize group")
    # the statistics, then the exponent update (which reads the exponent word for its thresholds and stores it once)
    stats, stats2 = arena.alloc(8, torch.float32, "stats"), arena.alloc(8, torch.float32, "stats_update")
    _lib.check(L.bsmm_tensor_stats(x.data_ptr(), n, CODE[dtype], 1.0, 1e-3, stats.data_ptr(), ws.data_ptr(), need, stream), "bsmm_tensor_stats")
    _lib.check(L.bsmm_quant_update_emax(x.data_ptr(), n, ctypes.byref(a), emax.data_ptr(), stats2.data_ptr()), "bsmm_quant_update_emax")
    torch.cuda.synchronize()
    arena.check()
    want = Q.quantize_test(X, spec, 8, seed=SEED, offset=9)
    nan_free = not np.isnan(want).any()
    for name, t in (("y_off", y_off), ("y_aligned", y_al), ("inplace", inplace)):
        if nan_free:
            GD.assert_stored(torch, t, name)
        assert QR.same_bits(P.to_host(t), want), (case, name)
    if y_group is not None:
        GD.assert_stored(torch, y_group, "y_group")
        assert QR.same_bits(P.to_host(y_group), Q.quantize_test(X, gspec)), (case, "group")
    GD.assert_stored(torch, stats, "stats")
    GD.assert_stored(torch, stats2, "stats_update")
    got, ref = stats.cpu().numpy().astype(np.float64), Q.tensor_stats_test(X, 1.0, 1e-3)
    assert got[2] == ref[2] and got[5] == ref[5] and got[6] == n and got[3] == np.float32(ref[3]) and got[4] == np.float32(ref[4]), (case, got, ref)
    assert abs(got[0] - ref[0]) <= P.L2_BAR["f32"] * ref[0] and abs(got[1] - ref[1]) <= P.L2_BAR["f32"] * ref[1], (case, got, ref)
    want_e, M = QR.emax_loop(X, 4, 1, 0, 4.0, 8)
    assert int(emax.item()) == want_e == Q.quantize_emax_test(X, spec, 8)           # (M = max|x|: an fp32 value, its exponent is exact)
    assert state.tolist() == [SEED, 9] and np.array_equal(P.to_host(x).view(np.uint32), X.view(np.uint32))          # the inputs are as they were
    arena.release()


@pytest.mark.parametrize("n", [2049, 3 * 2048 + 8])
def test_fp16_statistics_stay_inside(env, n):
    torch, _lib, L, Q = env
    X = _values(n, "f16", n)
    for mis in (0, 1, 2):
        arena = GD.GuardArena(torch, "cuda")
        x = arena.place(X, "x", mis, torch.float16)
        need = int(L.bsmm_quant_workspace_bytes(n))
        ws, stats = arena.alloc(need // 8, torch.float64, "workspace"), arena.alloc(8, torch.float32, "stats")
        emax = arena.place(np.array([3], dtype=np.int32), "emax")
        _lib.check(L.bsmm_tensor_stats(x.data_ptr(), n, CODE["f16"], 65504.0, 2.0 ** -24, stats.data_ptr(), ws.data_ptr(), need, _lib.raw_stream(x.device)),
                   "bsmm_tensor_stats")
        a = Q._args(Q.QuantizeSpec(5, 2), CODE["f16"], x.device, workspace=ws)
        _lib.check(L.bsmm_quant_update_emax(x.data_ptr(), n, ctypes.byref(a), emax.data_ptr(), None), "bsmm_quant_update_emax")
        torch.cuda.synchronize()
        arena.check()
        GD.assert_stored(torch, stats, "stats")
        got, ref = stats.cpu().numpy().astype(np.float64), Q.tensor_stats_test(X)
        assert got[2] == ref[2] and got[5] == ref[5] == 2 and got[6] == n and abs(got[0] - ref[0]) <= P.L2_BAR["f32"] * ref[0], (n, mis, got, ref)
        assert int(emax.item()) == Q.quantize_emax_test(X, Q.QuantizeSpec(5, 2), 3)
        arena.release()
