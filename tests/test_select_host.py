"""CPU tier of the fused row selection (include/bsmm_select.h, blocksparse_amd/select.py): the exported symbols, the struct mirror against the
header, argument checks that answer before anything is launched, ``select_path`` on both sides of every threshold, and the definitions the
GPU tests lean on -- the package's NumPy functions and the float64 helpers of tests/_select_ref.py -- against per-element loops and against
the reference's own results (golden/select.npz).  An integer model of the selection the kernels run is checked against ``np.lexsort`` under
the pinned order on named rows, and four mutants of it must each fail one of them.  No compute calls here."""
import ctypes
import os
import re

import numpy as np
import pytest

import _select_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "select.npz"))


def _header():
    return open(os.path.join(ROOT, "include", "bsmm_select.h")).read()


def test_select_header_symbols_exported_and_version_unchanged(lib):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(bsmm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.SELECT_SYMBOLS) == {"bsmm_select_path", "bsmm_rectified_top_k", "bsmm_masked_top_k_softmax", "bsmm_masked_softmax_grad",
                                                   "bsmm_sparse_relu", "bsmm_select_relu_grad"}, declared ^ set(lib.SELECT_SYMBOLS)
    others = set(lib.SYMBOLS) | set(lib.DIST_SYMBOLS) | set(lib.SPARSITY_SYMBOLS) | set(lib.OPTIM_SYMBOLS) | set(lib.OPTIM_LIST_SYMBOLS) | \
        set(lib.NORM_SYMBOLS) | set(lib.EW_SYMBOLS) | set(lib.ENDS_SYMBOLS) | set(lib.BST_SYMBOLS) | set(lib.LSTM_SYMBOLS)
    assert not declared & others
    L = lib.load()
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in declared:
        assert hasattr(L, s), s
        getattr(raw, s)
    assert L.bsmm_version() == lib.ABI_VERSION == 128
    import blocksparse_amd
    for name in ("rectified_top_k", "masked_top_k_softmax", "masked_softmax", "softmax", "sparse_relu", "select_path"):
        assert getattr(blocksparse_amd, name) is getattr(blocksparse_amd.select, name), name
    for op in ("rectified_top_k", "masked_top_k_softmax", "masked_softmax", "sparse_relu"):
        for suffix in ("_fwd", "_bwd", "_test", "_grad_test"):
            assert callable(getattr(blocksparse_amd.select, op + suffix)), op + suffix
    assert callable(blocksparse_amd.select.softmax_test)


def test_struct_mirror_and_constants_match_the_header(lib):
    body = re.search(r"typedef struct bsmm_select_args \{(.*?)\} bsmm_select_args;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "void*": ctypes.c_void_p}
    fields = []
    for m in re.finditer(r"(int32_t|int64_t|float|void\*)\s+([\w\s,]+);", body):
        fields += [(n.strip(), ctype[m.group(1)]) for n in m.group(2).split(",")]
    assert [f[0] for f in fields] == ["R", "K", "k", "mask_rows", "dtype", "rebase", "scale", "alpha", "stream"]
    assert fields == [(f[0], f[1]) for f in lib.BsmmSelectArgs._fields_]
    A = lib.BsmmSelectArgs
    # what a C compiler lays out: eight 4-byte members, a pointer
    assert [getattr(A, n).offset for n, _ in fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32] and ctypes.sizeof(A) == 40
    defs = dict((n, int(v)) for n, v in re.findall(r"#define (BSMM_SELECT_\w+) (\d+)", _header()))
    assert (defs["BSMM_SELECT_WAVE8_MAX"], defs["BSMM_SELECT_WAVE16_MAX"], defs["BSMM_SELECT_GROUP2_MAX"], defs["BSMM_SELECT_MAX_K"]) == \
        (lib.SELECT_WAVE8_MAX, lib.SELECT_WAVE16_MAX, lib.SELECT_GROUP2_MAX, lib.SELECT_MAX_K) == SR.THRESHOLDS + (SR.MAX_K,)
    for name, code in (("WAVE8", "wave8"), ("WAVE16", "wave16"), ("GROUP2", "group2"), ("GROUP4", "group4")):
        assert lib.SELECT_PATHS[defs["BSMM_SELECT_PATH_" + name]] == code and lib.SELECT_PATHS[defs["BSMM_SELECT_PATH_" + name] + 1] == code + "-wide"


def test_select_sources_read_no_environment_and_keep_no_state():
    src = ""
    for f in ("bsmm_select.hip", "bsmm_select_kernels.h"):
        src += open(os.path.join(ROOT, "blocksparse_amd", "csrc", f)).read()
    src = re.sub(r"//[^\n]*", "", src)                     # (the comments may say what the code does not do)
    for word in ("getenv", "hipMalloc", "hipFree", "Synchronize", "atomic", "static int", "static float", "static bool", "trace"):
        assert word not in src, word
    from blocksparse_amd import build
    assert "bsmm_select.hip" in build.SOURCES


def test_select_path_on_both_sides_of_every_threshold(lib):
    from blocksparse_amd import select_path
    import torch
    L = lib.load()
    names = ("wave8", "wave16", "group2", "group4")
    for dtype, td, V in (("f32", torch.float32, 4), ("f16", torch.float16, 8), ("bf16", torch.bfloat16, 8)):
        for i, T in enumerate(SR.THRESHOLDS):
            for K, want in ((T - 1, names[i]), (T, names[i]), (T + 1, names[i + 1])):
                for aligned in (True, False):
                    full = want + ("-wide" if aligned and K % V == 0 else "")
                    assert select_path(K, dtype, aligned) == select_path(K, td, aligned) == SR.path_name(K, dtype, aligned) == full, (K, dtype, aligned)
        assert select_path(1, dtype) == "wave8" and select_path(SR.MAX_K, dtype) == "group4-wide" and select_path(SR.MAX_K, dtype, False) == "group4"
        assert select_path(V, dtype) == "wave8-wide" and select_path(V + 1, dtype) == "wave8"
        with pytest.raises(ValueError):
            select_path(SR.MAX_K + 1, dtype)
        with pytest.raises(ValueError):
            select_path(0, dtype)
    with pytest.raises(ValueError):
        select_path(64, torch.float64)
    assert L.bsmm_select_path(SR.MAX_K + 1, 0, 1) == UNSUPPORTED and L.bsmm_select_path(0, 0, 1) == ARG and L.bsmm_select_path(64, 3, 1) == ARG


def _args(lib, R=4, K=64, k=3, mask_rows=1, dtype=2):
    return lib.BsmmSelectArgs(R=R, K=K, k=k, mask_rows=mask_rows, dtype=dtype, rebase=1, scale=1.0, alpha=1.0, stream=None)


def test_argument_checks_answer_before_any_launch(lib):
    """Every call here is wrong in exactly one way (the addresses are dummies that are never dereferenced), so none may reach a launch."""
    L = lib.load()
    one = ctypes.c_void_p(256)
    ref = lambda a: ctypes.byref(a) if a is not None else None
    calls = {
        "rect": (("x", "y"), lambda q, a: L.bsmm_rectified_top_k(q["x"], q["y"], ref(a))),
        "topk": (("x", "y"), lambda q, a: L.bsmm_masked_top_k_softmax(q["x"], q.get("mask"), q["y"], ref(a))),
        "grad": (("dy", "y", "dx"), lambda q, a: L.bsmm_masked_softmax_grad(q["dy"], q["y"], q.get("mask"), q["dx"], ref(a))),
        "srelu": (("x", "y"), lambda q, a: L.bsmm_sparse_relu(q["x"], q["y"], ref(a))),
        "relu_grad": (("dz", "y", "dx"), lambda q, a: L.bsmm_select_relu_grad(q["dz"], q["y"], q["dx"], ref(a))),
    }
    for name, (ptrs, call) in calls.items():
        q = {n: one for n in ptrs}
        assert call(q, None) == ARG, name
        for n in ptrs:
            assert call(dict(q, **{n: None}), _args(lib)) == ARG, (name, n)
        for bad in (dict(R=0), dict(K=0), dict(R=-1), dict(K=-4), dict(R=1 << 20, K=1 << 11), dict(R=1 << 30, K=2), dict(dtype=3), dict(dtype=-1)):
            assert call(q, _args(lib, **bad)) == ARG, (name, bad)
        if name in ("rect", "topk"):
            for bad in (dict(k=0), dict(k=-1), dict(k=65), dict(K=5000, k=5001)):
                assert call(q, _args(lib, **bad)) == ARG, (name, bad)
        if name in ("topk", "grad"):
            for bad in (dict(mask_rows=0), dict(mask_rows=-1), dict(mask_rows=3), dict(mask_rows=8)):
                assert call(dict(q, mask=one), _args(lib, **bad)) == ARG, (name, bad)
            assert call(dict(q, mask=one), _args(lib, K=SR.MAX_K + 1, mask_rows=2)) == UNSUPPORTED
        if name != "relu_grad":                               # a row too long for the registers: unsupported, not a bad argument
            assert call(q, _args(lib, K=SR.MAX_K + 1)) == UNSUPPORTED, name
            assert call(q, _args(lib, K=1 << 20, R=1)) == UNSUPPORTED, name
            assert call(dict(q, **{ptrs[0]: None}), _args(lib, K=SR.MAX_K + 1)) == ARG, name


def test_python_argument_errors(lib):
    import torch
    from blocksparse_amd import select as S
    x = torch.zeros(2, 3, 5, 8)
    for call in (lambda: S.rectified_top_k(x, 2), lambda: S.masked_top_k_softmax(x, 2), lambda: S.masked_softmax(x), lambda: S.softmax(x),
                 lambda: S.sparse_relu(x), lambda: S.rectified_top_k_fwd(x, 2), lambda: S.masked_softmax_bwd(x, x), lambda: S.relu_rule_bwd(x, x)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # the mask patterns: judged on shapes alone (a meta tensor has a shape and a dtype and no memory)
    xm = torch.empty(2, 3, 5, 8, device="meta")
    ok = lambda shape: S._mask_rows(xm, torch.empty(shape, device="meta"), "t")
    assert ok((1, 1, 1, 8)) == 1 and ok((1, 1, 5, 8)) == 5 and ok((1, 3, 5, 8)) == 15 and ok((2, 3, 5, 8)) == 30
    for shape in ((8,), (5, 8), (1, 3, 1, 8), (2, 1, 1, 8), (1, 1, 5, 1), (1, 1, 1, 4), (2, 1, 5, 8), (1, 1, 1, 1, 8)):
        with pytest.raises(ValueError):
            ok(shape)
    with pytest.raises(ValueError):
        S._mask_rows(xm, torch.empty((1, 1, 1, 8), device="meta", dtype=torch.float16), "t")


# ---- the order and the selection ------------------------------------------------------------------------------------------------------------
def _loop_order(v, masked):
    """The pinned order of one row by pairwise comparison: insertion into a list, element by element."""
    def first(a, b):                 # does index a come before index b?
        ma, mb = bool(masked[a]), bool(masked[b])
        if ma != mb:
            return mb
        if not ma:
            na, nb = np.isnan(v[a]), np.isnan(v[b])
            if na != nb:
                return na
            if not na and v[a] != v[b]:          # (-0.0 == 0.0)
                return v[a] > v[b]
        return a < b
    out = []
    for i in range(len(v)):
        pos = 0
        while pos < len(out) and first(out[pos], i):
            pos += 1
        out.insert(pos, i)
    return np.array(out)


def test_order_helper_and_keys_against_pairwise_comparison():
    from blocksparse_amd import select as S
    for name, (v, k, masked) in SR.named_cases().items():
        m = np.zeros(len(v), dtype=bool) if masked is None else masked
        want = _loop_order(v, m)
        np.testing.assert_array_equal(SR.order(v, masked), want, err_msg=name)
        keys = S.select_keys(v, masked).astype(np.int64)
        np.testing.assert_array_equal(np.argsort(-keys, kind="stable"), want, err_msg=name)
        np.testing.assert_array_equal(keys, SR.model_keys(v, masked), err_msg=name)
        sel, kth = S.select_top_k(v, k, masked)
        assert sel.sum() == k and set(np.nonzero(sel)[0]) == set(want[:k]) and int(kth[0]) == keys[want[k - 1]], name
    # the extremes of the key map
    v = np.array([np.nan, np.inf, 3.0, 1e-45, 0.0, -0.0, -1e-45, -3.0, -np.inf, -np.nan], dtype=np.float32)
    keys = S.select_keys(v).astype(np.int64)
    assert keys[0] == keys[9] == 0xffffffff and keys[4] == keys[5] and (np.diff(keys[:9]) <= 0).all() and keys[8] > 0


@pytest.mark.parametrize("geom", [(8, 8, 1), (8, 4, 1), (16, 8, 1), (16, 4, 2), (16, 8, 4)], ids=lambda g: "EL%d-V%d-NW%d" % g)
def test_selection_model_equals_lexsort_on_the_named_rows(geom):
    EL, V, NW = geom
    for name, (v, k, masked) in SR.named_cases().items():
        want = SR.selected(v, k, masked)
        for kk in sorted({1, 2, k, len(v) - 1, len(v)}):
            np.testing.assert_array_equal(SR.model_select(v, kk, masked, EL, V, NW), SR.selected(v, kk, masked), err_msg="%s k=%d" % (name, kk))
        # the same row at the far end of the team's registers: the tie prefix crosses chunks and waves
        cap = NW * 64 * EL
        long_v = np.full(cap, -7.0, dtype=np.float32)
        at = np.sort(np.random.default_rng(len(name)).choice(cap, len(v), replace=False))
        long_v[at] = v
        long_m = None
        if masked is not None:
            long_m = np.ones(cap, dtype=bool)
            long_m[at] = masked
        np.testing.assert_array_equal(SR.model_select(long_v, k, long_m, EL, V, NW), SR.selected(long_v, k, long_m), err_msg=name + " spread")
        assert want.sum() == k


@pytest.mark.parametrize("mutant, case", [("tie_reversed", "tie_across_kth"), ("strict", "tie_across_kth"), ("neg_zero_below", "pm_zero"),
                                          ("masked_by_value", "many_masked")])
def test_each_mutant_of_the_model_fails_its_named_row(mutant, case):
    """tie rule reversed, > for >= at the threshold, -0 ordered below +0, masked elements ordered by value."""
    v, k, masked = SR.named_cases()[case]
    want = SR.selected(v, k, masked)
    np.testing.assert_array_equal(SR.model_select(v, k, masked), want)
    assert not np.array_equal(SR.model_select(v, k, masked, **{mutant: True}), want), (mutant, case)


def test_tied_and_zero_data_sets_tie_across_the_kth_position():
    rng = np.random.default_rng(3)
    for K, k in ((5, 2), (64, 17), (65, 64), (513, 1), (1000, 999)):
        for rows, allowed in ((SR.tied_rows(3, K, k, rng), [1.0]), (SR.zero_rows(3, K, k, rng), [0.0])):
            o = SR.order(rows)
            a, b = np.take_along_axis(rows, o[:, k - 1:k], 1), np.take_along_axis(rows, o[:, k:k + 1], 1)
            assert (a == b).all() and np.isin(a, allowed).all(), (K, k)
        m = SR.sparse_mask(4, K, k, rng)
        assert ((m != 0).sum(axis=1) < k).all()
    for dtype in ("f32", "f16", "bf16"):
        rows = SR.distinct_rows(2, SR.MAX_K, dtype, rng)
        assert all(len(np.unique(r)) == SR.MAX_K for r in rows) and np.abs(rows).max() < 1


# ---- the definitions ------------------------------------------------------------------------------------------------------------------------
def _loop_topk_softmax(x, k, mask, scale):
    R, K = x.shape
    y = np.zeros((R, K))
    for r in range(R):
        m = np.ones(K, dtype=np.float32) if mask is None else mask[r % mask.shape[0]]
        v = [float(np.float32(np.float32(x[r, i] * m[i]) * np.float32(scale))) for i in range(K)]
        o = _loop_order(np.array(v), m == 0)[:k]
        live = [i for i in o if m[i] != 0]
        if not live:
            continue
        vmax = max(v[i] for i in range(K) if m[i] != 0)
        s = sum(np.exp(v[i] - vmax) for i in live)
        for i in live:
            y[r, i] = np.exp(v[i] - vmax) / s
    return y


def test_definitions_against_per_element_loops():
    from blocksparse_amd import select as S
    rng = np.random.default_rng(11)
    R, K = 6, 13
    x = SR.round_in(rng.normal(size=(R, K)), "f16")
    x[2, 4] = x[2, 9] = x[2, 1]                                   # ties
    mask = np.where(rng.random((3, K)) < 0.4, 0.0, rng.choice([1.0, 0.5, 2.0], (3, K))).astype(np.float32)
    mask[1] = 0.0                                                 # rows 1 and 4: nothing unmasked
    for k in (1, 4, K):
        for mk, scale in ((None, 1.0), (mask, 0.5)):
            want = _loop_topk_softmax(x, k, mk, scale)
            full = None if mk is None else np.tile(mk, (2, 1))
            got64, _ = SR.topk_softmax(x, k, full, scale)
            np.testing.assert_allclose(got64, want, rtol=1e-12, atol=1e-15)
            np.testing.assert_allclose(S.masked_top_k_softmax_test(x, k, full, scale), want, rtol=2e-6, atol=1e-9)
            assert not got64[1].any() or mk is None
        # rectified top-k: element by element
        for rebase in (True, False):
            want = np.zeros((R, K))
            for r in range(R):
                o = _loop_order(x[r], np.zeros(K, dtype=bool))
                base = max(float(x[r, o[k - 1]]), 0.0) if rebase else 0.0
                for i in o[:k]:
                    want[r, i] = max(float(x[r, i]), base) - base
            np.testing.assert_array_equal(SR.rect(x, k, rebase), want)
            np.testing.assert_array_equal(S.rectified_top_k_test(x, k, rebase), want.astype(np.float32))
    np.testing.assert_array_equal(S.masked_softmax_test(x, None, 0.5), S.masked_top_k_softmax_test(x, K, None, 0.5))
    np.testing.assert_array_equal(S.softmax_test(x, 0.5), S.masked_softmax_test(x, None, 0.5))
    # gradient of the softmax and the ReLU rule
    y, _ = SR.topk_softmax(x, 4, np.tile(mask, (2, 1)), 0.5)
    dy = rng.normal(size=(R, K))
    want = np.zeros((R, K))
    for r in range(R):
        dot = sum(dy[r, j] * y[r, j] for j in range(K))
        for i in range(K):
            want[r, i] = (dy[r, i] - dot) * y[r, i] * mask[r % 3, i] * 0.5
    np.testing.assert_allclose(SR.softmax_grad(dy, y, np.tile(mask, (2, 1)), 0.5), want, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(S.masked_softmax_grad_test(dy, y, np.tile(mask, (2, 1)), 0.5), want, rtol=2e-5, atol=1e-7)
    np.testing.assert_array_equal(S.rectified_top_k_grad_test(dy, y), np.where(y > 0, dy, 0.0))
    np.testing.assert_array_equal(SR.relu_rule(dy, y), np.where(y > 0, dy, 0.0))
    # sparse ReLU: the population variance around the mean
    for alpha in (1.0, 0.5):
        want = np.zeros((R, K))
        for r in range(R):
            mean = sum(float(t) for t in x[r]) / K
            var = sum((float(t) - mean) ** 2 for t in x[r]) / K
            for i in range(K):
                want[r, i] = max(float(x[r, i]) - (mean + alpha * var ** 0.5), 0.0)
        np.testing.assert_allclose(SR.sparse_relu(x, alpha)[0], want, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(S.sparse_relu_test(x, alpha), want, rtol=1e-5, atol=1e-6)
    # a large offset separates the variance forms: E[x^2] - mean^2 in fp32 loses sigma altogether at mean 1e4, sigma 1
    big = (1e4 + rng.normal(size=(4, 256))).astype(np.float32)
    y64, cut, sigma = SR.sparse_relu(big, 1.0)
    np.testing.assert_allclose(S.sparse_relu_test(big, 1.0), y64, rtol=0, atol=2e-3)
    naive = np.sqrt(np.maximum(np.mean(big * big, axis=1, dtype=np.float32) - np.square(np.mean(big, axis=1, dtype=np.float32)), 0))
    assert np.abs(naive - sigma[:, 0]).max() > 0.1


def test_definitions_against_the_reference_results(golden):
    from blocksparse_amd import select as S
    ops = [str(o) for o in golden["ops"]]
    assert len(ops) == 12 and set(ops) == {"rect", "topk", "softmax"}
    for i, op in enumerate(ops):
        key = "c%d/" % i
        X = golden[key + "X"].astype(np.float32)
        M = golden[key + "M"] if key + "M" in golden.files else None
        k, scale, rebase = int(golden["ks"][i]), float(golden["scales"][i]), bool(golden["rebase"][i])
        Y = golden[key + "Y"]
        if op == "rect":
            np.testing.assert_array_equal(S.rectified_top_k_test(X, k, rebase), Y, err_msg=key)
            np.testing.assert_array_equal(SR.rect(X, k, rebase).astype(np.float32), Y, err_msg=key)
            continue
        kk = k if op == "topk" else X.shape[-1]
        got = S.masked_top_k_softmax_test(X, kk, M, scale) if op == "topk" else S.masked_softmax_test(X, M, scale)
        np.testing.assert_allclose(got, Y, rtol=2e-6, atol=1e-9, err_msg=key)
        assert np.array_equal(got != 0, Y != 0), key
        y64, sel = SR.topk_softmax(X, kk, M, scale)
        np.testing.assert_allclose(y64, Y, rtol=2e-6, atol=1e-9, err_msg=key)
        DY = golden[key + "DY"].astype(np.float32)
        # the reference sums dy * y in fp32: up to K = 65 terms of magnitude <= max|dy| ~ 4 carry K * 2^-24 * 4 ~ 1.6e-5 into (dy - sum),
        # which the factors y * m * scale <= 4 scale once more
        np.testing.assert_allclose(S.masked_softmax_grad_test(DY, Y, M, scale), golden[key + "DX"], rtol=1e-5, atol=6e-5, err_msg=key)
        np.testing.assert_allclose(SR.softmax_grad(DY, Y, M, scale), golden[key + "DX"], rtol=1e-5, atol=6e-5, err_msg=key)
