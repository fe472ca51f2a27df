"""CPU tier of the layer epilogue (include/bsmm_ew.h, blocksparse_amd/ewops.py): the exported symbols, the struct mirror against the header,
argument checks that answer before anything is launched, the workspace arithmetic, Philox4x32-10 known answers, the NumPy mask definition
against a per-element loop, and the float64 helper of the GPU tests against a per-element loop.  No compute calls here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _ewops_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1
SEED = (1 << 40) + 12345          # above 2^32: both key words are in use; chosen on the CPU (see test_keep_share_is_binomial)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import _lib
    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "bsmm_ew.h")).read()


def test_ew_header_symbols_exported_and_version_unchanged(lib):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(bsmm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.EW_SYMBOLS), declared ^ set(lib.EW_SYMBOLS)
    others = set(lib.SYMBOLS) | set(lib.DIST_SYMBOLS) | set(lib.SPARSITY_SYMBOLS) | set(lib.OPTIM_SYMBOLS) | set(lib.OPTIM_LIST_SYMBOLS) | \
        set(lib.NORM_SYMBOLS) | set(lib.BST_SYMBOLS)
    assert not declared & others
    L = lib.load()
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in declared:
        assert hasattr(L, s), s
        getattr(raw, s)
    assert L.bsmm_version() == lib.ABI_VERSION == 128
    import blocksparse_amd
    for name in ("bias_relu", "fast_gelu", "dropout", "bias_dropout", "set_entropy"):
        assert getattr(blocksparse_amd, name) is getattr(blocksparse_amd.ewops, name)
    for name in ("bias_relu_fwd", "bias_relu_bwd", "dropout_mask", "apply_dropout_mask", "bias_dropout_fwd", "bias_dropout_bwd", "entropy_state",
                 "bias_relu_test", "bias_relu_grad_test", "dropout_mask_test", "bias_dropout_test", "bias_dropout_grad_test"):
        assert callable(getattr(blocksparse_amd.ewops, name)), name
    for macro, value in (("BSMM_ACT_NONE", lib.ACT_NONE), ("BSMM_ACT_RELU", lib.ACT_RELU), ("BSMM_ACT_FAST_GELU", lib.ACT_FAST_GELU),
                         ("BSMM_EW_BIAS_ACT", lib.EW_BIAS_ACT), ("BSMM_EW_BIAS_ACT_GRAD", lib.EW_BIAS_ACT_GRAD),
                         ("BSMM_EW_BIAS_ACT_DROPOUT", lib.EW_BIAS_ACT_DROPOUT), ("BSMM_EW_BIAS_ACT_DROPOUT_GRAD", lib.EW_BIAS_ACT_DROPOUT_GRAD)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == value, macro


def test_struct_mirror_matches_the_header(lib):
    body = re.search(r"typedef struct bsmm_ew_args \{(.*?)\} bsmm_ew_args;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "void*": ctypes.c_void_p, "size_t": ctypes.c_size_t}
    fields = [(m.group(2), ctype[m.group(1)]) for m in re.finditer(r"(int32_t|float|void\*|size_t)\s+(\w+)\s*;", body)]
    assert [f[0] for f in fields] == ["K", "N", "axis", "dtype", "act", "generate", "threshold", "scale", "workspace", "workspace_bytes", "stream"]
    assert [(n, t) for n, t in fields] == [(f[0], f[1]) for f in lib.BsmmEwArgs._fields_]
    A = lib.BsmmEwArgs
    # what a C compiler lays out: eight 4-byte members, then three 8-byte members
    assert [getattr(A, n).offset for n, _ in fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48] and ctypes.sizeof(A) == 56


def test_ew_sources_read_no_environment_and_keep_no_state():
    src = ""
    for f in ("bsmm_ew.hip", "bsmm_ew_kernels.h"):
        src += open(os.path.join(ROOT, "blocksparse_amd", "csrc", f)).read()
    src = re.sub(r"//[^\n]*", "", src)                     # (the comments may say what the code does not do)
    for word in ("getenv", "hipMalloc", "hipFree", "Synchronize", "atomic", "static int", "static float", "static bool", "trace"):
        assert word not in src, word


def _args(lib, K=64, N=16, axis=0, dtype=2, act=0, generate=1, threshold=32768, ws=256, ws_bytes=None, which=1):
    a = lib.BsmmEwArgs(K=K, N=N, axis=axis, dtype=dtype, act=act, generate=generate, threshold=threshold, scale=2.0, workspace=None,
                       workspace_bytes=0, stream=None)
    if ws_bytes is None:
        ws_bytes = lib.load().bsmm_ew_workspace_bytes(ctypes.byref(a), which)
    a.workspace, a.workspace_bytes = ws, ws_bytes
    return a


def test_argument_checks_answer_before_any_launch(lib):
    """Every call here is wrong in exactly one way (the addresses are dummies that are never dereferenced), so none may reach a launch."""
    L = lib.load()
    one = ctypes.c_void_p(256)
    ref = lambda a: ctypes.byref(a) if a is not None else None
    calls = {
        "bias_act": (lambda a, x=one, b=one, y=one: L.bsmm_bias_act(x, b, y, ref(a)), ("x", "b", "y"), 0, False),
        "bias_act_grad": (lambda a, dy=one, xy=one, b=one, dx=one, db=one: L.bsmm_bias_act_grad(dy, xy, b, dx, db, ref(a)),
                          ("dy", "xy", "b", "dx", "db"), 1, False),
        "fused": (lambda a, x=one, b=one, state=one, mask=one, y=one: L.bsmm_bias_act_dropout(x, b, None, state, mask, y, ref(a)),
                  ("x", "b", "state", "mask", "y"), 2, True),
        "fused_grad": (lambda a, dy=one, x=one, b=one, mask=one, dx=one, db=one: L.bsmm_bias_act_dropout_grad(dy, x, b, mask, dx, db, ref(a)),
                       ("dy", "x", "b", "mask", "dx", "db"), 3, False),
    }
    for axis in (0, 1):
        for name, (call, ptrs, which, drops) in calls.items():
            N = 20000 if axis == 0 else 16               # (axis 0 needs a workspace only when a row is cut over workgroups)
            ok = dict(axis=axis, which=which, act=2, N=N)
            assert call(None) == ARG
            for p in ptrs:
                assert call(_args(lib, **ok), **{p: None}) == ARG, (axis, name, p)
            for bad in (dict(K=0), dict(N=0), dict(K=-4), dict(N=-1), dict(K=1 << 16, N=1 << 15), dict(K=46341, N=46341), dict(dtype=3),
                        dict(dtype=-1), dict(act=3), dict(act=-1)):
                assert call(_args(lib, **dict(ok, **bad))) == ARG, (axis, name, bad)
            if drops:
                assert call(_args(lib, threshold=65537, **ok)) == ARG
                assert call(_args(lib, threshold=-1, **ok)) == ARG
                assert call(_args(lib, generate=2, **ok)) == ARG
                assert call(_args(lib, **ok), mask=ctypes.c_void_p(258)) == ARG          # a mask 2 bytes off
            if name == "fused_grad":
                assert call(_args(lib, **ok), mask=ctypes.c_void_p(258)) == ARG
            need = L.bsmm_ew_workspace_bytes(ctypes.byref(_args(lib, **ok)), which)
            if which in (1, 3):
                assert need > 0
                assert call(_args(lib, ws=None, **ok)) == ARG
                assert call(_args(lib, ws_bytes=need - 1, **ok)) == ARG
                assert call(_args(lib, ws=258, **ok)) == ARG           # not 4-byte aligned
            else:
                assert need == 0
        for name, (call, ptrs, which, drops) in calls.items():
            assert call(_args(lib, axis=2, which=which)) == ARG
            assert call(_args(lib, axis=-1, which=which)) == ARG
    # what is optional: x_or_y and dx of a plain bias gradient are not; with an activation they are required (checked above with act=2)
    # the fused forward wants a bias as soon as there is an activation, and a state only when it generates
    assert L.bsmm_bias_act_dropout(one, None, None, one, one, one, ctypes.byref(_args(lib, act=1))) == ARG
    assert L.bsmm_bias_act_dropout(one, one, None, None, one, one, ctypes.byref(_args(lib, generate=1))) == ARG
    assert L.bsmm_bias_act_dropout(one, one, None, ctypes.c_void_p(260), one, one, ctypes.byref(_args(lib, generate=1))) == ARG   # state 4 bytes off
    # the two calls without a struct
    big = 1 << 31
    for bad in (dict(mask=None), dict(state=None), dict(n=0), dict(n=-5), dict(n=big), dict(threshold=-1), dict(threshold=65537),
                dict(mask=ctypes.c_void_p(258)), dict(state=ctypes.c_void_p(260))):
        kw = dict(mask=one, state=one, n=100, threshold=100)
        kw.update(bad)
        assert L.bsmm_dropout_mask(kw["mask"], kw["state"], kw["n"], kw["threshold"], None) == ARG, bad
    for bad in (dict(x=None), dict(mask=None), dict(y=None), dict(n=0), dict(n=big), dict(dtype=3), dict(dtype=-1), dict(mask=ctypes.c_void_p(258))):
        kw = dict(x=one, mask=one, y=one, n=100, dtype=2)
        kw.update(bad)
        assert L.bsmm_dropout_apply(kw["x"], kw["mask"], kw["y"], kw["n"], 2.0, kw["dtype"], None) == ARG, bad


def test_workspace_bytes(lib):
    L = lib.load()
    wb = lambda which, **kw: L.bsmm_ew_workspace_bytes(ctypes.byref(_args(lib, ws_bytes=0, **kw)), which)
    assert L.bsmm_ew_workspace_bytes(None, 1) == 0
    Ns = list(range(1, 70)) + [96, 255, 256, 257, 511, 512, 513, 1024, 1043, 4096, 8191, 8192, 8193, 8200, 16384, 16385, 65536, 1 << 18]
    Ks = list(range(1, 70)) + [255, 256, 257, 511, 512, 1024, 1031, 2048, 2049, 4096, 8192, 8193]
    for axis in (0, 1):
        for which in (0, 2, 4, -1):
            assert wb(which, axis=axis, N=20000) == 0                       # the forward calls and unknown calls
        for which in (1, 3):
            assert wb(which, K=0, axis=axis) == 0 and wb(which, N=0, axis=axis) == 0 and wb(which, K=-8, N=-8, axis=axis) == 0
            assert wb(which, axis=axis, dtype=9) == 0 and wb(which, axis=axis, act=7) == 0 and wb(which, axis=2) == 0
            assert wb(which, axis=axis, K=1 << 16, N=1 << 15) == 0
            for dtype in (0, 2):
                for K in (1, 7, 8, 24, 48, 256, 2049, 8193):
                    last = 0
                    for N in (n for n in Ns if K * n < 1 << 31):
                        b = wb(which, K=K, N=N, axis=axis, dtype=dtype)
                        assert b >= last and b % 4 == 0, (which, axis, dtype, K, N, b, last)
                        last = b
                for N in (1, 24, 64, 513, 8192, 8193, 1 << 17):
                    last = 0
                    for K in Ks:
                        b = wb(which, K=K, N=N, axis=axis, dtype=dtype)
                        assert b >= last, (which, axis, dtype, K, N, b, last)
                        last = b
            assert wb(which, axis=axis, K=64, N=100000) == wb(4 - which, axis=axis, K=64, N=100000)       # both gradients need the same
    assert wb(1, axis=0, N=8192) == 0 and wb(1, axis=0, N=8193) > 0 and wb(1, axis=1, N=1) > 0


def test_python_argument_errors(lib):
    import torch
    from blocksparse_amd import bias_dropout, bias_relu, dropout, ewops
    x, b = torch.zeros(4, 8), torch.zeros(8)
    with pytest.raises(ValueError):
        bias_relu(x, b, relu=True, fast_gelu=True)
    with pytest.raises(ValueError):
        bias_dropout(x, b, 0.5, relu=True, fast_gelu=True)
    with pytest.raises(NotImplementedError):
        dropout(x, 0.5, mask_shape=(4, 1))
    for kp in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            dropout(x, kp)
        with pytest.raises(ValueError):
            bias_dropout(x, b, kp)
        with pytest.raises(ValueError):
            ewops.dropout_mask_test(10, 1, 0, kp)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bias_relu(x, b)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dropout(x, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ewops.bias_dropout_fwd(x, b, 0.5)
    assert ewops._keep(0.8) == (52429, float(np.float32(1.25))) and ewops._keep(1.0) == (65536, 1.0)
    assert "ignored" in bias_relu.__doc__ and "atomics" in bias_relu.__doc__


KNOWN = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def test_philox_known_answers():
    from blocksparse_amd import ewops
    for counter, key, want in KNOWN:
        assert ER.philox(counter, key) == want
        got = ewops.philox4x32_10(counter, key)
        assert tuple(int(v[0]) for v in got) == want
        w = ER.philox_np(*[np.array([c], dtype=np.uint64) for c in counter[:2]], counter[2], counter[3], key[0], key[1])
        assert tuple(int(v[0]) for v in w) == want


def test_mask_definition_against_a_per_element_loop():
    from blocksparse_amd import ewops
    for n in (1, 7, 8, 9, 31, 32, 33, 65):
        for offset in (0, (1 << 33) + 7):
            for kp in (0.8, 0.5):
                th = ER.threshold_of(kp)
                bits = [ER.keep_bit_loop(i, SEED, offset, th) for i in range(n)]
                words = ER.pack(bits)
                got = ewops.dropout_mask_test(n, SEED, offset, kp)
                assert got.dtype == np.int32 and got.shape == ((n + 31) // 32,)
                assert np.array_equal(got.view(np.uint32), words), (n, offset, kp)
                assert np.array_equal(ER.mask_words(n, SEED, offset, kp), words)
                if n % 32:
                    assert int(got.view(np.uint32)[-1]) >> (n % 32) == 0            # pad bits are zero
                assert np.array_equal(ewops.unpack_mask(got, n), np.array(bits)) and np.array_equal(ER.unpack(words, n), np.array(bits))
    # other offsets and other seeds give other masks
    a = ewops.dropout_mask_test(4096, SEED, 0, 0.5)
    assert not np.array_equal(a, ewops.dropout_mask_test(4096, SEED, 1, 0.5)) and not np.array_equal(a, ewops.dropout_mask_test(4096, SEED + (1 << 32), 0, 0.5))


def test_keep_share_is_binomial():
    """2^20 bits: the kept share within 5 binomial standard deviations of threshold / 65536.  Deterministic for SEED (observed on the CPU:
    0.80004 at keep_prob 0.8 and 0.49972 at 0.5, that is 0.10 and -0.57 standard deviations)."""
    from blocksparse_amd import ewops
    n = 1 << 20
    for kp in (0.8, 0.5):
        p = ER.threshold_of(kp) / 65536.0
        share = ewops.unpack_mask(ewops.dropout_mask_test(n, SEED, 0, kp), n).mean()
        sd = math.sqrt(p * (1 - p) / n)
        print(kp, share, (share - p) / sd)
        assert abs(share - p) <= 5 * sd, (kp, share)


def test_thresholds_zero_and_all():
    from blocksparse_amd import ewops
    for n in (1, 31, 32, 33, 1000):
        assert ER.keep_bits(n, SEED, 3, 0).sum() == 0 and ER.keep_bits(n, SEED, 3, 65536).all()
        full = ewops.dropout_mask_test(n, SEED, 3, 1.0)
        assert np.array_equal(full.view(np.uint32), ER.pack(np.ones(n, dtype=bool)))
        assert not ewops.unpack_mask(ewops._pack(ewops._keep_bits(n, SEED, 3, 0)), n).any()


def test_reference_helper_against_a_per_element_loop():
    rng = np.random.default_rng(11)
    K, N, scale = 5, 7, 1.25
    sig = lambda z: 1.0 / (1.0 + math.exp(-1.702 * z))
    for axis in (0, 1):
        shape = (K, N) if axis == 0 else (N, K)
        x, dy, r = rng.normal(size=shape), rng.normal(size=shape), rng.normal(size=shape)
        b = rng.normal(size=K)
        kept = rng.random(K * N) < 0.7
        for a in (0, 1, 2):
            y, dx, db = np.zeros(shape), np.zeros(shape), np.zeros(K)
            for k in range(K):
                for n in range(N):
                    idx = (k, n) if axis == 0 else (n, k)
                    flat = idx[0] * shape[1] + idx[1]
                    z = x[idx] + b[k]
                    v = z if a == 0 else (max(z, 0.0) if a == 1 else z * sig(z))
                    y[idx] = (v * scale if kept[flat] else 0.0) + r[idx]
                    g = dy[idx] * scale if kept[flat] else 0.0
                    d = 1.0 if a == 0 else ((1.0 if z > 0 else 0.0) if a == 1 else sig(z) + 1.702 * z * sig(z) * (1 - sig(z)))
                    dx[idx] = g * d
                    db[k] += g * d
            np.testing.assert_allclose(ER.forward(x, b, axis, a, kept, scale, r), y, rtol=1e-12, atol=1e-14)
            dx2, db2 = ER.backward(dy, x, b, axis, a, kept, scale)
            np.testing.assert_allclose(dx2, dx, rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(db2, db, rtol=1e-12, atol=1e-13)
    # saturation stays finite; ranks above 2 flatten as the operator does
    z = np.array([-100.0, -30.0, 30.0, 100.0])
    assert np.isfinite(ER.act(z, 2)).all() and np.isfinite(ER.act_grad(z, 2)).all()
    x3, b6, b5 = rng.normal(size=(6, 2, 5)), rng.normal(size=6), rng.normal(size=5)
    np.testing.assert_array_equal(ER.forward(x3, b6, 0, 2), ER.forward(x3.reshape(6, 10), b6, 0, 2).reshape(x3.shape))
    np.testing.assert_array_equal(ER.forward(x3, b5, -1, 1), ER.forward(x3.reshape(12, 5), b5, 1, 1).reshape(x3.shape))
    np.testing.assert_array_equal(ER.backward(x3, x3, b6, 0, 2)[1], ER.backward(x3.reshape(6, 10), x3.reshape(6, 10), b6, 0, 2)[1])


def test_numpy_functions_agree_with_the_helper():
    from blocksparse_amd import ewops
    rng = np.random.default_rng(12)
    for axis, shape, K in ((0, (6, 10), 6), (-1, (10, 6), 6), (0, (6, 2, 5), 6), (-1, (3, 4, 5), 5)):
        x, dy, r = (rng.normal(size=shape) for _ in range(3))
        b = rng.normal(size=K)
        n = x.size
        mask = ewops.dropout_mask_test(n, 9, 2, 0.75)
        kept = ER.keep_bits(n, 9, 2, ER.threshold_of(0.75))
        scale = ER.scale_of(0.75)
        for a, kw in ((0, {}), (1, dict(relu=True)), (2, dict(fast_gelu=True))):
            np.testing.assert_allclose(ewops.bias_relu_test(x, b, axis, **kw), ER.forward(x, b, axis, a), rtol=1e-12, atol=1e-14)
            dx, db = ewops.bias_relu_grad_test(dy, x, b, axis, **kw)
            wdx, wdb = ER.backward(dy, x, b, axis, a)
            np.testing.assert_allclose(dx, wdx, rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(db, wdb, rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(ewops.bias_dropout_test(x, b, mask, 0.75, axis, residual=r, **kw), ER.forward(x, b, axis, a, kept, scale, r),
                                       rtol=1e-12, atol=1e-14)
            dx, db = ewops.bias_dropout_grad_test(dy, x, b, mask, 0.75, axis, **kw)
            wdx, wdb = ER.backward(dy, x, b, axis, a, kept, scale)
            np.testing.assert_allclose(dx, wdx, rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(db, wdb, rtol=1e-12, atol=1e-13)
