"""CPU tier of the fused LSTM gates (include/bsmm_lstm.h, blocksparse_amd/lstm.py): the exported symbols, the struct mirror against the
header, argument checks that answer before anything is launched, and the two definitions the GPU tests lean on -- the package's NumPy
functions and the float64 helper tests/_lstm_ref.py -- against a per-element Python loop and against central differences.  No compute calls
here."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest

import _lstm_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import _lib
    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "bsmm_lstm.h")).read()


def test_lstm_header_symbols_exported_and_version_unchanged(lib):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(bsmm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.LSTM_SYMBOLS) == {"bsmm_lstm_gates", "bsmm_lstm_gates_grad"}, declared ^ set(lib.LSTM_SYMBOLS)
    others = set(lib.SYMBOLS) | set(lib.DIST_SYMBOLS) | set(lib.SPARSITY_SYMBOLS) | set(lib.OPTIM_SYMBOLS) | set(lib.OPTIM_LIST_SYMBOLS) | \
        set(lib.NORM_SYMBOLS) | set(lib.EW_SYMBOLS) | set(lib.ENDS_SYMBOLS) | set(lib.BST_SYMBOLS)
    assert not declared & others
    L = lib.load()
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in declared:
        assert hasattr(L, s), s
        getattr(raw, s)
    assert L.bsmm_version() == lib.ABI_VERSION == 128
    import blocksparse_amd
    assert blocksparse_amd.fused_lstm_gates is blocksparse_amd.lstm.fused_lstm_gates
    for name in ("fused_lstm_gates_fwd", "fused_lstm_gates_bwd", "fused_lstm_gates_test", "fused_lstm_gates_grad_test"):
        assert callable(getattr(blocksparse_amd.lstm, name)), name


def test_struct_mirror_matches_the_header(lib):
    body = re.search(r"typedef struct bsmm_lstm_args \{(.*?)\} bsmm_lstm_args;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "void*": ctypes.c_void_p}
    fields = []
    for m in re.finditer(r"(int32_t|int64_t|float|void\*)\s+([\w\s,]+);", body):
        fields += [(n.strip(), ctype[m.group(1)]) for n in m.group(2).split(",")]
    assert [f[0] for f in fields] == ["K", "N", "axis", "dtype", "gate_ld", "dgate_ld", "forget_bias", "stream"]
    assert fields == [(f[0], f[1]) for f in lib.BsmmLstmArgs._fields_]
    A = lib.BsmmLstmArgs
    # what a C compiler lays out: four 4-byte members, two 8-byte members, a float and 4 bytes of padding, a pointer
    assert [getattr(A, n).offset for n, _ in fields] == [0, 4, 8, 12, 16, 24, 32, 40] and ctypes.sizeof(A) == 48


def test_lstm_sources_read_no_environment_and_keep_no_state():
    src = ""
    for f in ("bsmm_lstm.hip", "bsmm_lstm_kernels.h"):
        src += open(os.path.join(ROOT, "blocksparse_amd", "csrc", f)).read()
    src = re.sub(r"//[^\n]*", "", src)                     # (the comments may say what the code does not do)
    for word in ("getenv", "hipMalloc", "hipFree", "Synchronize", "atomic", "static int", "static float", "static bool", "trace"):
        assert word not in src, word
    from blocksparse_amd import build
    assert "bsmm_lstm.hip" in build.SOURCES


def _args(lib, K=64, N=16, axis=1, dtype=2, gate_ld=None, dgate_ld=None):
    return lib.BsmmLstmArgs(K=K, N=N, axis=axis, dtype=dtype, gate_ld=K if gate_ld is None else gate_ld,
                            dgate_ld=K if dgate_ld is None else dgate_ld, forget_bias=1.0, stream=None)


def test_argument_checks_answer_before_any_launch(lib):
    """Every call here is wrong in exactly one way (the addresses are dummies that are never dereferenced), so none may reach a launch."""
    L = lib.load()
    one = ctypes.c_void_p(256)
    ref = lambda a: ctypes.byref(a) if a is not None else None
    fwd_names = ("c", "i", "u", "f", "o", "c_next", "h_next")
    bwd_names = ("c", "i", "u", "f", "o", "dc", "di", "du", "df", "d_o")

    def fwd(a, **p):
        q = {n: one for n in fwd_names}
        q.update(p)
        return L.bsmm_lstm_gates(q["c"], q["i"], q["u"], q["f"], q["o"], p.get("bias", one), q["c_next"], q["h_next"], ref(a))

    def bwd(a, **p):
        q = {n: one for n in bwd_names}
        q.update(p)
        return L.bsmm_lstm_gates_grad(q["c"], q["i"], q["u"], q["f"], q["o"], p.get("bias", one), p.get("eh", one), p.get("ec", one), q["dc"], q["di"],
                                      q["du"], q["df"], q["d_o"], ref(a))

    for call, names in ((fwd, fwd_names), (bwd, bwd_names)):
        assert call(None) == ARG
        for axis in (0, 1):
            for n in names:
                assert call(_args(lib, axis=axis), **{n: None}) == ARG, (call.__name__, axis, n)
            for bad in (dict(K=0), dict(N=0), dict(K=-4), dict(N=-1), dict(K=1 << 16, N=1 << 15), dict(K=46341, N=46341), dict(dtype=3),
                        dict(dtype=-1), dict(K=1 << 29, N=1, gate_ld=1 << 31, dgate_ld=1 << 31), dict(K=(1 << 31) - 1, N=1, gate_ld=1 << 31, dgate_ld=1 << 31)):
                assert call(_args(lib, **dict(dict(axis=axis), **bad))) == ARG, (call.__name__, axis, bad)
        assert call(_args(lib, axis=2)) == ARG and call(_args(lib, axis=-1)) == ARG
        assert call(_args(lib, axis=1, K=64, gate_ld=63)) == ARG
        assert call(_args(lib, axis=1, K=64, gate_ld=0)) == ARG and call(_args(lib, axis=1, K=64, gate_ld=-256)) == ARG
    assert bwd(_args(lib, axis=1, K=64, dgate_ld=63)) == ARG
    assert bwd(_args(lib), eh=None, ec=None) == ARG                      # both gradients absent


def _loop_cell(c, i, u, f, o, b, fb):
    """One cell, on Python floats: (c_next, h_next) and the activations."""
    sig = lambda x: 1.0 / (1.0 + math.exp(-x))
    si, tu, sf, so = sig(i + b[0]), math.tanh(u + b[1]), sig(f + b[2] + fb), sig(o + b[3])
    cn = sf * c + si * tu
    ca = math.tanh(cn)
    return cn, so * ca, (si, tu, sf, so, ca)


def _loop(C, H, B, EH, EC, fb, axis):
    """The definition, element by element, on (K, N) / (N, K) arrays."""
    K = C.shape[0 if axis == 0 else 1]
    cn, hn, dc = np.zeros(C.shape), np.zeros(C.shape), np.zeros(C.shape)
    dh, db = np.zeros(H.shape), np.zeros(4 * K)
    for idx in itertools.product(*(range(s) for s in C.shape)):
        k = idx[0] if axis == 0 else idx[1]
        at = lambda q: (q * K + idx[0], idx[1]) if axis == 0 else (idx[0], q * K + idx[1])
        b = [0.0] * 4 if B is None else [B[q * K + k] for q in range(4)]
        cn[idx], hn[idx], (si, tu, sf, so, ca) = _loop_cell(C[idx], H[at(0)], H[at(1)], H[at(2)], H[at(3)], b, fb)
        eh, ec = (0.0 if EH is None else EH[idx]), (0.0 if EC is None else EC[idx])
        dC = eh * so * (1 - ca * ca) + ec
        for q, g in enumerate((dC * tu * si * (1 - si), dC * si * (1 - tu * tu), dC * C[idx] * sf * (1 - sf), eh * ca * so * (1 - so))):
            dh[at(q)] = g
            db[q * K + k] += g
        dc[idx] = dC * sf
    return cn, hn, dc, dh, db


@pytest.mark.parametrize("axis", (0, 1))
def test_definitions_against_a_per_element_loop(axis):
    from blocksparse_amd import lstm
    rng = np.random.default_rng(21 + axis)
    K, N, fb = 3, 5, 0.75
    shape, hshape = ((K, N), (4 * K, N)) if axis == 0 else ((N, K), (N, 4 * K))
    C, EH, EC = (rng.normal(size=shape) for _ in range(3))
    H, B = rng.normal(size=hshape), rng.normal(size=4 * K)
    ax = 0 if axis == 0 else -1
    for bias in (None, B):
        for eh, ec in ((EH, EC), (EH, None), (None, EC)):
            cn, hn, dc, dh, db = _loop(C, H, bias, eh, ec, fb, axis)
            gates = LR.split(H, ax)
            rcn, rhn = LR.forward(C, gates, bias, fb, ax)
            rdc, rd, rdb = LR.backward(C, gates, eh, ec, bias, fb, ax)
            pcn, phn = lstm.fused_lstm_gates_test(C, H, bias=bias, forget_bias=fb, axis=ax)
            got = lstm.fused_lstm_gates_grad_test(C, H, eh=eh, ec=ec, bias=bias, forget_bias=fb, axis=ax)
            for name, want, a, b in (("c_next", cn, rcn, pcn), ("h_next", hn, rhn, phn), ("dc", dc, rdc, got[0]), ("dh", dh, LR.fuse(rd, ax), got[1])):
                np.testing.assert_allclose(a, want, rtol=1e-12, atol=1e-14, err_msg=name)
                np.testing.assert_allclose(b, want, rtol=1e-12, atol=1e-14, err_msg=name)
            if bias is None:
                assert rdb is None and len(got) == 2
            else:
                np.testing.assert_allclose(rdb, db, rtol=1e-12, atol=1e-13)
                np.testing.assert_allclose(got[2], db, rtol=1e-12, atol=1e-13)
    with pytest.raises(ValueError):
        lstm.fused_lstm_gates_grad_test(C, H, axis=ax)              # both gradients absent
    # ranks above 2 flatten as the operator does
    C3, H3 = (C.reshape(K, 1, N), H.reshape(4 * K, 1, N)) if axis == 0 else (C.reshape(1, N, K), H.reshape(1, N, 4 * K))
    np.testing.assert_array_equal(lstm.fused_lstm_gates_test(C3, H3, bias=B, axis=ax)[1].reshape(shape), lstm.fused_lstm_gates_test(C, H, bias=B, axis=ax)[1])
    np.testing.assert_array_equal(LR.forward(C3, LR.split(H3, ax), B, 1.0, ax)[0].reshape(shape), LR.forward(C, LR.split(H, ax), B, 1.0, ax)[0])


@pytest.mark.parametrize("axis", (0, 1))
def test_helper_gradient_against_central_differences(axis):
    """L = sum(wh * h_next) + sum(wc * c_next): the helper's gradients with eh = wh, ec = wc against (L(x + d) - L(x - d)) / 2d in float64.
    d = 1e-6: the truncation term is ~d^2 = 1e-12 and the rounding term ~1e-16 / d = 1e-10 of values of order 1."""
    rng = np.random.default_rng(31 + axis)
    K, N, fb, d = 3, 4, 1.0, 1e-6
    ax = 0 if axis == 0 else -1
    shape, hshape = ((K, N), (4 * K, N)) if axis == 0 else ((N, K), (N, 4 * K))
    C, WH, WC = (rng.normal(size=shape) for _ in range(3))
    H, B = rng.normal(size=hshape), rng.normal(size=4 * K)

    def loss(c, h, b):
        cn, hn = LR.forward(c, LR.split(h, ax), b, fb, ax)
        return float((WH * hn).sum() + (WC * cn).sum())

    dc, dg, db = LR.backward(C, LR.split(H, ax), WH, WC, B, fb, ax)
    for name, x, grad in (("c", C, dc), ("h", H, LR.fuse(dg, ax)), ("b", B, db)):
        num = np.zeros(x.shape)
        for idx in itertools.product(*(range(s) for s in x.shape)):
            hi, lo = x.copy(), x.copy()
            hi[idx] += d
            lo[idx] -= d
            pick = lambda v: (v if name == "c" else C, v if name == "h" else H, v if name == "b" else B)
            num[idx] = (loss(*pick(hi)) - loss(*pick(lo))) / (2 * d)
        np.testing.assert_allclose(grad, num, rtol=1e-6, atol=1e-8, err_msg=name)


def test_forget_bias_and_bias_add_to_f_as_defined():
    from blocksparse_amd import lstm
    rng = np.random.default_rng(41)
    K, N = 4, 6
    C, H, B = rng.normal(size=(N, K)), rng.normal(size=(N, 4 * K)), rng.normal(size=4 * K)
    shifted = H.copy()
    shifted[:, 2 * K:3 * K] += B[2 * K:3 * K] + 0.625                      # f + b_f + fb by hand, nothing else
    only_f = np.zeros(4 * K)
    only_f[2 * K:3 * K] = B[2 * K:3 * K]
    for fn in (lambda c, h, **kw: lstm.fused_lstm_gates_test(c, h, **kw), lambda c, h, bias=None, forget_bias=1.0: LR.forward(c, LR.split(h, -1), bias, forget_bias)):
        want = fn(C, shifted, forget_bias=0.0)
        got = fn(C, H, bias=only_f, forget_bias=0.625)
        for a, b in zip(got, want):
            np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-15)
        assert np.abs(fn(C, H, forget_bias=0.0)[0] - fn(C, H, forget_bias=1.0)[0]).max() > 1e-3      # the default is not a no-op
    assert lstm.fused_lstm_gates.__kwdefaults__["forget_bias"] == 1.0 and lstm.fused_lstm_gates_test.__kwdefaults__["forget_bias"] == 1.0


@pytest.mark.parametrize("axis", (0, 1))
def test_four_tensor_form_equals_the_fused_form_on_slices(axis):
    from blocksparse_amd import lstm
    rng = np.random.default_rng(51 + axis)
    K, N = 5, 3
    ax = 0 if axis == 0 else -1
    shape, hshape = ((K, N), (4 * K, N)) if axis == 0 else ((N, K), (N, 4 * K))
    C, EH, EC, H = rng.normal(size=shape), rng.normal(size=shape), rng.normal(size=shape), rng.normal(size=hshape)
    parts = [np.ascontiguousarray(p) for p in LR.split(H, ax)]
    assert all(p.shape == shape for p in parts)
    for a, b in zip(lstm.fused_lstm_gates_test(C, *parts, axis=ax), lstm.fused_lstm_gates_test(C, H, axis=ax)):
        np.testing.assert_array_equal(a, b)
    four = lstm.fused_lstm_gates_grad_test(C, *parts, eh=EH, ec=EC, axis=ax)
    dc, dh = lstm.fused_lstm_gates_grad_test(C, H, eh=EH, ec=EC, axis=ax)
    assert len(four) == 5
    np.testing.assert_array_equal(four[0], dc)
    np.testing.assert_array_equal(LR.fuse(four[1:], ax), dh)
    with pytest.raises(ValueError):
        lstm.fused_lstm_gates_test(C, *parts, bias=np.zeros(4 * K), axis=ax)
    with pytest.raises(ValueError):
        lstm.fused_lstm_gates_test(C, parts[0], parts[1], axis=ax)


def test_saturated_inputs_give_finite_limits():
    """Every combination of 0 and +-65504 (the largest fp16) in c and the four gates: finite results, the limits of sigmoid and tanh."""
    from blocksparse_amd import lstm
    vals = np.array(list(itertools.product((0.0, 65504.0, -65504.0), repeat=5)))
    C, parts = vals[:, :1], [vals[:, q:q + 1] for q in range(1, 5)]
    E = np.ones_like(C)
    with np.errstate(over="raise", invalid="raise", divide="raise"):
        outs = LR.forward(C, parts) + lstm.fused_lstm_gates_test(C, *parts)
        dc, dg, _ = LR.backward(C, parts, E, E)
        grads = (dc,) + dg + lstm.fused_lstm_gates_grad_test(C, *parts, eh=E, ec=E)
    for a in outs + grads:
        assert np.isfinite(a).all()
    for cn, hn in (outs[:2], outs[2:]):
        sat = lambda v: np.where(v > 0, 1.0, np.where(v < 0, 0.0, 0.5))
        tsat = lambda v: np.sign(v)
        want_cn = np.where(vals[:, 3] == 0, 1.0 / (1.0 + math.exp(-1.0)), sat(vals[:, 3])) * vals[:, 0] + sat(vals[:, 1]) * tsat(vals[:, 2])
        np.testing.assert_allclose(cn[:, 0], want_cn, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(hn[:, 0], sat(vals[:, 4]) * np.tanh(want_cn), rtol=1e-12, atol=1e-12)
    for a, b in zip(grads[:5], grads[5:]):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)


def test_python_argument_errors(lib):
    import torch
    from blocksparse_amd import fused_lstm_gates, lstm
    c, h = torch.zeros(4, 8), torch.zeros(4, 32)
    with pytest.raises(ValueError):
        fused_lstm_gates(c)                                       # no gate tensor
    with pytest.raises(ValueError):
        fused_lstm_gates(c, h, h)                                 # neither one nor four
    with pytest.raises(ValueError):
        fused_lstm_gates(c, c, c, c, c, bias=torch.zeros(32))     # a bias with four tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fused_lstm_gates(c, h)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lstm.fused_lstm_gates_fwd(c, c, c, c, c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        lstm.fused_lstm_gates_bwd(c, h, eh=c)
