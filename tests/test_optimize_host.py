"""CPU tier of the weight-update operators (include/bsmm_optim.h, blocksparse_amd/optimize.py): the exported symbols, the struct mirror,
argument checks that answer before anything is launched, the host arithmetic (workspace size, step-size correction) and the float64
reference helper of the GPU tests against a per-element loop.  No compute calls here."""
import ctypes
import os
import re

import numpy as np
import pytest

import _optimize_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import _lib
    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "bsmm_optim.h")).read()


def test_optim_header_symbols_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(bsmm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.OPTIM_SYMBOLS), declared ^ set(lib.OPTIM_SYMBOLS)
    for other in (lib.SYMBOLS, lib.DIST_SYMBOLS, lib.SPARSITY_SYMBOLS, lib.BST_SYMBOLS):
        assert not declared & set(other)
    L = lib.load()
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in declared:
        assert hasattr(L, s), s
        getattr(raw, s)
    assert L.bsmm_version() == lib.ABI_VERSION          # new symbols only: bsmm.h and its version stay as they were


def test_adam_struct_layout_matches_header(lib):
    body = re.search(r"typedef struct bsmm_adam_args \{(.*?)\} bsmm_adam_args;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.search(r"(\w+)\s*;", ln).group(1) for ln in body.splitlines() if ";" in ln]
    assert names == [f[0] for f in lib.BsmmAdamArgs._fields_]
    kinds = {"ptr": 0, "size_t": 0, "int32_t": 0, "float": 0}
    for ln in body.splitlines():
        if ";" in ln:
            kinds["ptr" if "*" in ln else re.search(r"(size_t|int32_t|float)", ln).group(1)] += 1
    assert kinds == {"ptr": 9, "size_t": 1, "int32_t": 5, "float": 8}
    assert ctypes.sizeof(lib.BsmmAdamArgs) == 9 * 8 + 8 + 5 * 4 + 8 * 4 + 4      # (+ 4: tail padding to the pointers' alignment)
    assert lib.BsmmAdamArgs.size.offset == 72 and lib.BsmmAdamArgs.lr.offset == 100


def test_optim_sources_read_no_environment_and_keep_no_state():
    src = ""
    for f in ("bsmm_optim.hip", "bsmm_optim_kernels.h"):
        src += open(os.path.join(ROOT, "blocksparse_amd", "csrc", f)).read()
    src = re.sub(r"//[^\n]*", "", src)                     # (the comments may say what the code does not do)
    for word in ("getenv", "hipMalloc", "hipFree", "Synchronize", "atomic", "static "):
        assert word not in src, word
    assert "fast-math" not in open(os.path.join(ROOT, "blocksparse_amd", "build.py")).read()      # IEEE sqrt and division


def _adam_args(lib, **kw):
    a = lib.BsmmAdamArgs()
    for f in ("param", "mean", "var", "grad"):
        setattr(a, f, 256)
    a.size, a.bsize, a.grad_dtype, a.lr, a.beta1, a.beta2, a.epsilon, a.grad_scale = 4 * 1024, 32, lib.F32, 1e-3, 0.9, 0.999, 1e-8, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_checks_answer_before_any_launch(lib):
    L = lib.load()
    one = ctypes.c_void_p(256)           # a non-null, aligned dummy address: never dereferenced
    ARG, UNSUP, WS = -1, -2, -3
    adam = lambda **kw: L.bsmm_adam(ctypes.byref(_adam_args(lib, **kw)))
    assert L.bsmm_adam(None) == ARG
    for f in ("param", "mean", "var", "grad"):
        assert adam(**{f: None}) == ARG, f
    assert adam(size=0) == ARG
    assert adam(size=4 * 1024 + 8) == ARG                          # no multiple of bsize^2
    assert adam(size=63, bsize=8) == ARG
    assert adam(bsize=0, gate=256) == ARG                          # a flat tensor takes no gate ...
    assert adam(bsize=0, lr_select=256) == ARG                     # ... and no lr select
    assert adam(bsize=12, size=144) == UNSUP
    assert adam(bsize=-8) == UNSUP
    assert adam(grad_dtype=3) == UNSUP
    assert adam(param16=256, param16_dtype=lib.F32) == UNSUP
    assert adam(param16=256, param16_dtype=9) == UNSUP
    # ema
    assert L.bsmm_ema(None, one, None, 0.999, 1024, 32, lib.F32, None) == ARG
    assert L.bsmm_ema(one, None, None, 0.999, 1024, 32, lib.F32, None) == ARG
    assert L.bsmm_ema(one, one, None, 0.999, 0, 32, lib.F32, None) == ARG
    assert L.bsmm_ema(one, one, None, 0.999, 1000, 32, lib.F32, None) == ARG
    assert L.bsmm_ema(one, one, one, 0.999, 1024, 0, lib.F32, None) == ARG
    assert L.bsmm_ema(one, one, None, 0.999, 1024, 24, lib.F32, None) == UNSUP
    assert L.bsmm_ema(one, one, None, 0.999, 1024, 32, 5, None) == UNSUP
    # sum of squares / clip
    need = L.bsmm_sum_squared_workspace_bytes(3)
    assert need > 0
    ss = lambda x=one, size=100, dt=lib.BF16, idx=0, cnt=3, ws=one, nb=need: L.bsmm_sum_squared(x, size, dt, 1.0, 0.0, 0, 0, idx, cnt, ws, nb, None)
    assert ss(x=None) == ARG
    assert ss(size=0) == ARG
    assert ss(idx=-1) == ARG and ss(idx=3) == ARG and ss(cnt=0) == ARG
    assert ss(dt=4) == UNSUP
    assert ss(ws=None) == WS
    assert ss(nb=need - 1) == WS
    assert L.bsmm_clip_norm(one, need, 3, 1.0, None, one, None) == ARG
    assert L.bsmm_clip_norm(one, need, 3, 1.0, one, None, None) == ARG
    assert L.bsmm_clip_norm(one, need, 0, 1.0, one, one, None) == ARG
    assert L.bsmm_clip_norm(None, need, 3, 1.0, one, one, None) == WS
    assert L.bsmm_clip_norm(one, need - 1, 3, 1.0, one, one, None) == WS


def test_workspace_bytes_monotone_in_the_tensor_count(lib):
    L = lib.load()
    assert L.bsmm_sum_squared_workspace_bytes(0) == 0 and L.bsmm_sum_squared_workspace_bytes(-5) == 0
    last = 0
    for cnt in list(range(1, 80)) + [1000, 4096]:
        b = L.bsmm_sum_squared_workspace_bytes(cnt)
        assert b >= last and b > 0 and b % 4 == 0, (cnt, b, last)
        last = b


def test_lr_correction_matches_the_accumulators():
    from blocksparse_amd import optimize
    for b1, b2 in ((0.9, 0.999), (0.8, 0.98)):
        for t in range(1, 6):
            want = OR.lr_correction_loop(t, b1, b2)
            assert abs(optimize.lr_correction(t, b1, b2) - want) <= 1e-13 * want, (t, b1, b2)
            assert optimize.lr_correction(t, b1, b2, zero_init_variables=True) == OR.lr_correction_loop(t, b1, b2, True) == 1.0


def test_cpu_tensors_are_rejected_loudly():
    import torch
    from blocksparse_amd import adam_step, ema_step, clip_by_global_norm, AdamOptimizer
    w = torch.zeros(4, 8, 8)
    for call in (lambda: adam_step(w, w, w, w, 1e-3), lambda: ema_step(w, w, 0.9), lambda: clip_by_global_norm([w]), lambda: AdamOptimizer([w])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_reference_helper_against_a_per_element_loop():
    """tests/_optimize_ref.py (vectorised float64) against the definitions written out element by element: 5 blocks of 8 x 8, every option."""
    rng = np.random.RandomState(3)
    bs, blocks = 8, 5
    n = blocks * bs * bs
    p, m = rng.normal(0, 0.01, n).astype(np.float32), rng.normal(0, 0.01, n).astype(np.float32)
    v = rng.uniform(0, 1e-2, n).astype(np.float32)
    g = rng.normal(0, 0.1, n).astype(np.float32)
    g[::7] *= 50
    g[3], g[70], g[130], g[200] = np.inf, -np.inf, np.nan, np.inf
    m[::53] = v[::53] = 0
    gate = np.array([0, 1, 1, 0, 1], dtype=np.float32)
    sel = np.array([0, 1, 0, 1, 0], dtype=np.float32)
    settings = [dict(), dict(grad_scale=0.5, norm_scale=0.7, saturate=2.0, clip_sigma=3.0, zero_infs=True, zero_nans=True),
                dict(zero_infs=True, zero_nans=True), dict(saturate=2.0), dict(norm_scale=0.0), dict(zero_nans=True, clip_sigma=3.0, saturate=1.0)]
    for kw in settings:
        for extra in (dict(), dict(gate=gate, bsize=bs), dict(gate=gate, bsize=bs, lr_select=sel, lr_new=5e-3), dict(bsize=bs, lr_select=sel, lr_new=5e-3)):
            a = OR.adam(p, m, v, g, 1e-3, **kw, **extra)
            b = OR.adam_loop(p, m, v, g, 1e-3, **kw, **extra)
            for x, y, name in zip(a, b, "pmv"):
                np.testing.assert_allclose(x, y, rtol=1e-12, atol=0, equal_nan=True, err_msg=str((name, kw, sorted(extra))))
    a = OR.adam(p, m, v, g, 1e-3, gate=gate, bsize=bs, zero_infs=True, zero_nans=True)
    for x, old in zip(a, (p, m, v)):
        assert np.array_equal(x.reshape(blocks, -1)[gate == 0], old.astype(np.float64).reshape(blocks, -1)[gate == 0])
        assert not np.array_equal(x.reshape(blocks, -1)[1], old.astype(np.float64).reshape(blocks, -1)[1])
    e = rng.normal(0, 0.01, n).astype(np.float32)
    for gt in (None, gate):
        np.testing.assert_allclose(OR.ema(e, p, 0.99, gt, bs), OR.ema_loop(e, p, 0.99, gt, bs), rtol=1e-13)
    fin = g.copy()
    fin[~np.isfinite(fin)] = 0
    want = sum((min(max(float(x), -2.0), 2.0) * 0.5) ** 2 for x in fin)
    np.testing.assert_allclose(OR.sum_squared(g, 0.5, 2.0, True, True), want, rtol=1e-12)
    assert OR.clip([OR.sum_squared(g)], 1.0)[1] == 0.0 and not np.isfinite(OR.clip([OR.sum_squared(g)], 1.0)[0])
    assert OR.clip([9.0, 16.0], 1.0) == (5.0, 0.2) and OR.clip([0.25], 1.0) == (0.5, 1.0)
    assert OR.gate_pattern(37, np.random.RandomState(0))[[0, 4, 36]].tolist() == [0.0, 1.0, 0.0]
