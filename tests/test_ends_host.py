"""CPU tier of the two operators at the ends of a model (include/bsmm_ends.h, blocksparse_amd/xent.py, blocksparse_amd/embed.py): the
exported symbols, the struct mirrors against the header, argument checks that answer before anything is launched, the workspace arithmetic,
the path report on both sides of every threshold, and the NumPy definitions (and the float64 helpers of the GPU tests) against per-element
loops, including the ignored row and indices outside the table.  No compute calls here."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _ends_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG = -1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import _lib
    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "bsmm_ends.h")).read()


def _macro(hdr, name):
    return float(re.search(r"#define %s ([0-9.]+)f?\b" % name, hdr).group(1))


def test_ends_header_symbols_exported_and_version_unchanged(lib):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(bsmm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.ENDS_SYMBOLS), declared ^ set(lib.ENDS_SYMBOLS)
    others = set(lib.SYMBOLS) | set(lib.DIST_SYMBOLS) | set(lib.SPARSITY_SYMBOLS) | set(lib.OPTIM_SYMBOLS) | set(lib.OPTIM_LIST_SYMBOLS) | \
        set(lib.NORM_SYMBOLS) | set(lib.EW_SYMBOLS) | set(lib.BST_SYMBOLS)
    assert not declared & others
    L = lib.load()
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in declared:
        assert hasattr(L, s), s
        getattr(raw, s)
    assert L.bsmm_version() == lib.ABI_VERSION == 128
    import blocksparse_amd
    assert blocksparse_amd.softmax_cross_entropy is blocksparse_amd.xent.softmax_cross_entropy
    assert blocksparse_amd.embedding_lookup is blocksparse_amd.embed.embedding_lookup
    for name in ("softmax_cross_entropy_fwd", "softmax_cross_entropy_bwd", "softmax_cross_entropy_test", "softmax_cross_entropy_grad_test", "xent_path"):
        assert callable(getattr(blocksparse_amd.xent, name)), name
    for name in ("embedding_lookup_fwd", "embedding_lookup_bwd", "embedding_lookup_test", "embedding_lookup_grad_test", "sort_order"):
        assert callable(getattr(blocksparse_amd.embed, name)), name
    for macro, value in (("BSMM_XENT_F16_SCALE", lib.XENT_F16_SCALE), ("BSMM_XENT_SHORT", lib.XENT_SHORT), ("BSMM_XENT_REG", lib.XENT_REG),
                         ("BSMM_XENT_REG_WIDE", lib.XENT_REG_WIDE), ("BSMM_XENT_LONG", lib.XENT_LONG), ("BSMM_XENT_VEC", lib.XENT_VEC),
                         ("BSMM_XENT_STRIDED", lib.XENT_STRIDED), ("BSMM_XENT_SHORT_MAX", lib.XENT_SHORT_MAX), ("BSMM_XENT_REG_MAX", lib.XENT_REG_MAX),
                         ("BSMM_XENT_WIDE_MAX", lib.XENT_WIDE_MAX), ("BSMM_XENT_MAX_GRID", lib.XENT_MAX_GRID), ("BSMM_EMBED_CHUNK", lib.EMBED_CHUNK),
                         ("BSMM_ENDS_XENT_FWD", lib.ENDS_XENT_FWD), ("BSMM_ENDS_XENT_BWD", lib.ENDS_XENT_BWD),
                         ("BSMM_ENDS_EMBED_FWD", lib.ENDS_EMBED_FWD), ("BSMM_ENDS_EMBED_GRAD", lib.ENDS_EMBED_GRAD)):
        assert _macro(hdr, macro) == value, macro
    assert blocksparse_amd.xent.XENT_F16_SCALE == ER.F16_SCALE == 2.0 ** 15 and ER.CHUNK == lib.EMBED_CHUNK


def _fields(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    out = []
    for m in re.finditer(r"((?:const\s+)?\w+\s*\*?)\s*(\w+)\s*;", body):
        t = m.group(1).replace("const", "").strip()
        out.append((m.group(2), ctypes.c_void_p if t.endswith("*") else ctype[t]))
    return out


def test_struct_mirrors_match_the_header(lib):
    fx = _fields("bsmm_xent_args")
    assert [f[0] for f in fx] == ["x", "labels", "loss", "g", "dy", "dx", "N", "K", "dtype", "reserved", "stream"]
    assert fx == [(f[0], f[1]) for f in lib.BsmmXentArgs._fields_]
    # what a C compiler lays out: six pointers, four 4-byte members, one pointer
    assert [getattr(lib.BsmmXentArgs, n).offset for n, _ in fx] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64] and ctypes.sizeof(lib.BsmmXentArgs) == 72
    fe = _fields("bsmm_embed_args")
    assert [f[0] for f in fe] == ["C", "K", "nIdx", "dtype", "workspace", "workspace_bytes", "stream"]
    assert fe == [(f[0], f[1]) for f in lib.BsmmEmbedArgs._fields_]
    assert [getattr(lib.BsmmEmbedArgs, n).offset for n, _ in fe] == [0, 4, 8, 12, 16, 24, 32] and ctypes.sizeof(lib.BsmmEmbedArgs) == 40


def test_ends_sources_read_no_environment_and_keep_no_state():
    src = ""
    for f in ("bsmm_ends.hip", "bsmm_ends_kernels.h"):
        src += open(os.path.join(ROOT, "blocksparse_amd", "csrc", f)).read()
    src = re.sub(r"//[^\n]*", "", src)                     # (the comments may say what the code does not do)
    for word in ("getenv", "hipMalloc", "hipFree", "Synchronize", "atomic", "static int", "static float", "static bool", "trace"):
        assert word not in src, word


def _xent(lib, **kw):
    d = dict(x=256, labels=256, loss=256, g=512, dy=256, dx=512, N=4, K=40, dtype=2, reserved=0, stream=None)
    d.update(kw)
    return lib.BsmmXentArgs(**d)


def _embed(lib, L, ws=256, ws_bytes=None, **kw):
    d = dict(C=10, K=40, nIdx=300, dtype=2)
    d.update(kw)
    a = lib.BsmmEmbedArgs(workspace=None, workspace_bytes=0, stream=None, **d)
    a.workspace = ws
    a.workspace_bytes = L.bsmm_ends_workspace_bytes(ctypes.byref(a), lib.ENDS_EMBED_GRAD) if ws_bytes is None else ws_bytes
    return a


def test_argument_checks_answer_before_any_launch(lib):
    """Every call here is wrong in exactly one way (the addresses are dummies that are never dereferenced), so none may reach a launch."""
    L = lib.load()
    sizes = (dict(N=0), dict(K=0), dict(N=-1), dict(K=-7), dict(N=1 << 16, K=1 << 15), dict(N=46341, K=46341), dict(dtype=3), dict(dtype=-1))
    for call, ptrs in ((L.bsmm_xent_fwd, ("x", "labels", "loss", "g")), (L.bsmm_xent_bwd, ("g", "dy", "dx"))):
        assert call(None) == ARG
        for p in ptrs:
            assert call(ctypes.byref(_xent(lib, **{p: None}))) == ARG, p
        for bad in sizes:
            assert call(ctypes.byref(_xent(lib, **bad))) == ARG, bad
    assert L.bsmm_xent_path(None) == ARG
    for bad in sizes:
        assert L.bsmm_xent_path(ctypes.byref(_xent(lib, **bad))) == ARG, bad
    # pointers that are not aligned to their element
    for bad in (dict(x=257), dict(g=513), dict(labels=258), dict(loss=258)):
        assert L.bsmm_xent_fwd(ctypes.byref(_xent(lib, **bad))) == ARG, bad
    assert L.bsmm_xent_fwd(ctypes.byref(_xent(lib, dtype=0, x=258))) == ARG
    for bad in (dict(g=513), dict(dx=513), dict(dy=258)):
        assert L.bsmm_xent_bwd(ctypes.byref(_xent(lib, **bad))) == ARG, bad
    # the embedding
    one = ctypes.c_void_p(256)
    esizes = (dict(C=0), dict(K=0), dict(nIdx=0), dict(C=-1), dict(K=-1), dict(nIdx=-5), dict(C=1 << 16, K=1 << 15), dict(nIdx=1 << 16, K=1 << 15),
              dict(dtype=3), dict(dtype=-1))
    fwd = lambda a, w=one, idx=one, y=one: L.bsmm_embed_fwd(w, idx, y, ctypes.byref(a) if a is not None else None)
    bwd = lambda a, dy=one, idx=one, order=one, dw=one: L.bsmm_embed_grad(dy, idx, order, dw, ctypes.byref(a) if a is not None else None)
    for call, ptrs in ((fwd, ("w", "idx", "y")), (bwd, ("dy", "idx", "order", "dw"))):
        assert call(None) == ARG
        for p in ptrs:
            assert call(_embed(lib, L), **{p: None}) == ARG, p
        for bad in esizes:
            assert call(_embed(lib, L, ws_bytes=1 << 40, **bad)) == ARG, bad
    assert fwd(_embed(lib, L), w=ctypes.c_void_p(257)) == ARG and fwd(_embed(lib, L), idx=ctypes.c_void_p(258)) == ARG
    assert fwd(_embed(lib, L, dtype=0), y=ctypes.c_void_p(258)) == ARG
    assert bwd(_embed(lib, L), dy=ctypes.c_void_p(257)) == ARG and bwd(_embed(lib, L), order=ctypes.c_void_p(258)) == ARG
    assert bwd(_embed(lib, L), dw=ctypes.c_void_p(258)) == ARG
    need = L.bsmm_ends_workspace_bytes(ctypes.byref(_embed(lib, L)), lib.ENDS_EMBED_GRAD)
    assert need > 0
    assert bwd(_embed(lib, L, ws=None)) == ARG
    assert bwd(_embed(lib, L, ws_bytes=need - 1)) == ARG
    assert bwd(_embed(lib, L, ws=258)) == ARG                   # not 4-byte aligned


def test_workspace_arithmetic(lib):
    L = lib.load()
    ws = lambda which, **kw: L.bsmm_ends_workspace_bytes(ctypes.byref(_embed(lib, L, ws_bytes=0, **kw)), which)
    for which in (lib.ENDS_XENT_FWD, lib.ENDS_XENT_BWD, lib.ENDS_EMBED_FWD, 4, -1):
        assert ws(which) == 0 and ws(which, K=4096, nIdx=65536) == 0
    assert L.bsmm_ends_workspace_bytes(None, lib.ENDS_EMBED_GRAD) == 0
    assert ws(lib.ENDS_EMBED_GRAD, K=0) == 0 and ws(lib.ENDS_EMBED_GRAD, nIdx=0) == 0
    # two rows of K floats per chunk of sorted positions; the table's height plays no part
    for K in (1, 5, 96, 1043, 2056):
        for n in (1, lib.EMBED_CHUNK - 1, lib.EMBED_CHUNK, lib.EMBED_CHUNK + 1, 3 * lib.EMBED_CHUNK + 5, 65536):
            assert ws(lib.ENDS_EMBED_GRAD, K=K, nIdx=n) == 2 * math.ceil(n / lib.EMBED_CHUNK) * K * 4
            assert ws(lib.ENDS_EMBED_GRAD, K=K, nIdx=n, C=50257 if K < 2000 else 300) == ws(lib.ENDS_EMBED_GRAD, K=K, nIdx=n)
    last = 0
    for n in range(1, 1000, 7):
        cur = ws(lib.ENDS_EMBED_GRAD, K=24, nIdx=n)
        assert cur >= last
        last = cur
    last = 0
    for K in range(1, 3000, 13):
        cur = ws(lib.ENDS_EMBED_GRAD, K=K, nIdx=1000)
        assert cur >= last
        last = cur


def test_xent_path_on_both_sides_of_every_threshold(lib):
    L = lib.load()
    S, R, W, G, V, T = lib.XENT_SHORT, lib.XENT_REG, lib.XENT_REG_WIDE, lib.XENT_LONG, lib.XENT_VEC, lib.XENT_STRIDED
    path = lambda **kw: L.bsmm_xent_path(ctypes.byref(_xent(lib, **kw)))
    # the 16-byte path: aligned x and g, K a multiple of 8
    for K, want in ((8, S), (1024, S), (1032, R), (8192, R), (8200, W), (32768, W), (32776, G), (65536, G), (1 << 20, G)):
        assert path(N=3, K=K) == want | V, K
        for dtype in (0, 1):
            assert path(N=3, K=K, dtype=dtype) == want | V, (K, dtype)
    # the element path, by size and by either pointer: its two register limits are half as large
    for K, want in ((1, S), (255, S), (1023, S), (1025, R), (4095, R), (4097, W), (8193, W), (16383, W), (16385, G), (70001, G)):
        assert path(N=3, K=K) == want, K
    for K, want in ((1024, S), (4096, R), (4104, W), (16384, W), (16392, G)):
        assert path(N=3, K=K, x=258) == want and path(N=3, K=K, g=516) == want and path(N=3, K=K, x=264, g=520) == want, K
    assert path(N=3, K=4096, x=1024, g=1024) == R | V            # in place
    # more rows than the grid has workgroups: four rows per workgroup on the short path, one elsewhere
    grid = lib.XENT_MAX_GRID
    assert path(N=4 * grid, K=8) == S | V and path(N=4 * grid + 1, K=8) == S | V | T
    assert path(N=grid, K=1032) == R | V and path(N=grid + 1, K=1032) == R | V | T
    assert path(N=grid + 1, K=8200) == W | V | T and path(N=grid + 1, K=40001) == G | T
    # only x and g are looked at
    assert path(N=3, K=64, labels=None, loss=None, dy=None, dx=None) == S | V


def test_numpy_xent_definitions_against_loops():
    from blocksparse_amd import xent
    rng = np.random.RandomState(5)
    x = rng.uniform(-20, 20, (2, 3, 7))
    labels = np.array([[0, 6, -1], [7, 3, 1 << 20]])
    dy = rng.standard_normal((2, 3))
    loss, g = xent.softmax_cross_entropy_test(x, labels)
    dx = xent.softmax_cross_entropy_grad_test(g, dy)
    rloss, rg, rp, rdist = ER.xent_ref(x.reshape(6, 7), labels.reshape(6))
    assert loss.shape == (2, 3) and g.shape == x.shape and dx.shape == x.shape and loss.dtype == np.float64
    for a in range(2):
        for b in range(3):
            row, t = x[a, b], int(labels[a, b])
            if not 0 <= t < 7:
                assert loss[a, b] == 0.0 and not g[a, b].any() and not dx[a, b].any()
                assert rloss[3 * a + b] == 0.0 and not rg[3 * a + b].any()
                continue
            m = max(row)
            s = sum(math.exp(v - m) for v in row)
            assert abs(loss[a, b] - (math.log(s) + m - row[t])) < 1e-12
            assert abs(rloss[3 * a + b] - loss[a, b]) < 1e-12
            for k in range(7):
                want = math.exp(row[k] - m) / s - (1.0 if k == t else 0.0)
                assert abs(g[a, b, k] - want) < 1e-14 and abs(rg[3 * a + b, k] - want) < 1e-14
                assert abs(dx[a, b, k] - want * dy[a, b]) < 1e-14
                assert abs(rp[3 * a + b, k] - math.exp(row[k] - m) / s) < 1e-14 and abs(rdist[3 * a + b, k] - (m - row[k])) < 1e-14
    # the loss of an improbable label is not clipped
    loss, _ = xent.softmax_cross_entropy_test(np.array([[60.0, 0.0, 0.0]]), np.array([1]))
    assert abs(loss[0] - 60.0) < 1e-9


def test_numpy_embedding_definitions_against_loops():
    from blocksparse_amd import embed
    rng = np.random.RandomState(6)
    C, K = 5, 3
    w = rng.standard_normal((C, K)).astype(np.float32)
    idx = np.array([[0, 4, -1, 2], [5, 2, 1 << 30, 2]])
    dy = rng.standard_normal((2, 4, K))
    y = embed.embedding_lookup_test(w, idx)
    dw = embed.embedding_lookup_grad_test(dy, idx, C)
    assert y.shape == (2, 4, K) and y.dtype == w.dtype and dw.shape == (C, K) and dw.dtype == np.float64
    want = np.zeros((C, K))
    for a in range(2):
        for b in range(4):
            i = int(idx[a, b])
            if 0 <= i < C:
                assert np.array_equal(y[a, b], w[i])
                for k in range(K):
                    want[i, k] += dy[a, b, k]
            else:
                assert not y[a, b].any()
    assert np.allclose(dw, want, rtol=0, atol=1e-14) and not dw[1].any() and not dw[3].any()
    flat = idx.reshape(-1)
    assert np.array_equal(ER.embed_fwd_ref(w, flat), y.reshape(8, K))
    rdw, named = ER.embed_grad_ref(dy.reshape(8, K), flat, C)
    assert np.allclose(rdw, want, rtol=0, atol=1e-14) and named.tolist() == [True, False, True, False, True]
    # the inverted index: ascending, ties in ascending position
    order = ER.stable_order(flat)
    assert order.tolist() == [2, 0, 3, 5, 7, 1, 4, 6]


def test_seeded_inputs_hold_what_the_gpu_tests_rely_on():
    for dtype in ("f32", "f16", "bf16"):
        X, labels, dy = ER.xent_inputs(16, 40, dtype, "uniform")
        assert np.array_equal(ER.rounded(X, dtype), X) and np.isfinite(dy).all() and (np.abs(dy) >= 0.5).all()
        assert (X[15] == X[15, 0]).all() and X[14].max() > 35.0
        assert labels[3] == -1 and labels[10] == 40 and ((labels >= 0) & (labels < 40)).sum() == 14
    for pattern in ER.PATTERNS:
        idx = ER.embed_indices(50, 300, pattern)
        assert idx.dtype == np.int64 and idx.size >= 1
    assert len(set(ER.embed_indices(50, 300, "permutation").tolist())) == 50
    eq = ER.embed_indices(50, 300, "equal")
    assert eq.size == 3 * ER.CHUNK + 5 and (eq == 49).all()
    sk = ER.embed_indices(50, 300, "skew")
    assert (sk == 25).mean() > 0.4
    st = np.sort(ER.embed_indices(50, 300, "straddle"))
    assert st[ER.CHUNK - 1] == st[ER.CHUNK] and st[2 * ER.CHUNK - 1] == st[2 * ER.CHUNK] and st[ER.CHUNK] != st[2 * ER.CHUNK]
    out = ER.embed_indices(50, 300, "outside")
    assert {-1, 50, 1 << 30} <= set(out.tolist())
    W, DY, DYX = ER.embed_values(50, 96, 300, "bf16")
    assert np.array_equal(DYX * 32, np.round(DYX * 32)) and np.abs(DYX).max() < 4


MASKED_KS = (10, 520, 1024, 1032, 4097, 8200, 16385, 32776)      # the K of the GPU test's cases


def test_xent_ref_indexes_the_label_and_keeps_its_bits_on_finite_inputs():
    """xent_ref once took x[label] as (x * onehot).sum(), which is NaN for a masked class; it indexes now.  On the seeded finite inputs
    of the GPU tests nothing may move by a bit."""
    def old(X, labels):
        x = np.asarray(X, dtype=np.float64)
        N, K = x.shape
        live = (labels >= 0) & (labels < K)
        m = x.max(axis=1)
        lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
        p = np.exp(x - lse[:, None])
        onehot = np.zeros((N, K))
        onehot[np.nonzero(live)[0], labels[live]] = 1.0
        return np.where(live, lse - (x * onehot).sum(axis=1), 0.0), np.where(live[:, None], p - onehot, 0.0), p, np.abs(x - m[:, None])

    for N, K in ((1, 1), (3, 10), (64, 256), (5, 257), (16, 1031), (3, 4097), (2, 16385), (2, 32776), (7, 4097)):
        for dtype in ("f32", "f16", "bf16"):
            for dist in ("normal", "uniform"):
                X, labels, _ = ER.xent_inputs(N, K, dtype, dist)
                for a, b in zip(ER.xent_ref(X, labels), old(X, labels)):
                    assert a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.int64), b.view(np.int64)), (N, K, dtype, dist)
    # the mask of the finite logits leaves the two criteria as they were when every logit is finite
    X, labels, _ = ER.xent_inputs(5, 257, "bf16", "uniform")
    _, g, p, dist = ER.xent_ref(X, labels)
    got = ER.rounded(g, "f32")
    assert ER.f32_g_ratio(got, g, p, dist) == ER.f32_g_ratio(got, g, p, dist, np.isfinite(X))
    ER.check_16bit(ER.rounded(g, "bf16"), g, "bf16", "mask of all", np.isfinite(X))


def test_masked_inputs_and_their_float64_reference():
    from blocksparse_amd import xent
    hot = ER.MASKED_LABEL_ROW
    for K in MASKED_KS:
        for dtype in ("f32", "f16", "bf16"):
            X, labels = ER.xent_masked_inputs(K, dtype)
            off = np.isneginf(X)
            assert X.shape == (6, K) and not np.isnan(X).any() and not np.isposinf(X).any() and np.array_equal(ER.rounded(X, dtype), X)
            assert (off.sum(axis=1) >= 1).all() and ((~off).sum(axis=1) >= 1).all()
            row = dict(zip(ER.MASKS, off))
            head = min(8 * 1024, K - 1)
            assert row["head"][:head].all() and not row["head"][head:].any()
            assert row["tail"][K - K // 3:].all() and not row["tail"][:K - K // 3].any()
            assert row["stripes"][:8].all() and (K < 16 or not row["stripes"][8:16].any())
            assert row["unit0"].sum() == min(8, K - 1) and row["unit0"][:min(8, K - 1)].all()
            assert row["single"].sum() == 1 and row["single"][5]
            assert (~row["only_label"]).sum() == 1 and not row["only_label"][labels[5]]
            masked_label = off[np.arange(6), labels]
            assert masked_label.tolist() == [i == hot for i in range(6)]
            loss, g, p, dist = ER.xent_ref(X, labels)
            assert np.isfinite(np.delete(loss, hot)).all() and loss[hot] == np.inf and (np.delete(loss, hot) >= 0).all()
            assert np.isfinite(g).all() and np.isfinite(p).all() and not p[off].any() and np.isinf(dist[off]).all() and np.isfinite(dist[~off]).all()
            assert g[hot, labels[hot]] == -1.0 and not g[off & (np.arange(K)[None, :] != labels[:, None])].any()
            assert np.allclose(p.sum(axis=1), 1.0, rtol=0, atol=1e-12) and abs(loss[5]) < 1e-12
            # the package's float64 definition says the same
            with np.errstate(invalid="ignore", divide="ignore"):
                ploss, pg = xent.softmax_cross_entropy_test(X, labels)
            assert np.array_equal(np.isfinite(ploss), np.isfinite(loss)) and ploss[hot] == np.inf
            assert np.allclose(np.delete(ploss, hot), np.delete(loss, hot), rtol=1e-12, atol=1e-12) and np.allclose(pg, g, rtol=0, atol=1e-14)
    # a row with no finite logit, with +inf or with NaN is NaN in that row only
    X = np.array([[0.0, 1.0, 2.0], [-np.inf] * 3, [0.0, np.inf, 1.0], [np.nan, 0.0, 1.0], [1.0, 2.0, 3.0]])
    loss = ER.xent_ref(X, np.array([0, 1, 2, 1, 2]))[0]
    with np.errstate(invalid="ignore"):
        ploss = xent.softmax_cross_entropy_test(X, np.array([0, 1, 2, 1, 2]))[0]
    for got in (loss, ploss):
        assert np.isnan(got).tolist() == [False, True, True, True, False]


def test_float32_model_of_the_streamed_recurrence():
    """A float32 NumPy model of xent_long_kernel (per-lane running maximum, rescale, merge of the 1024 lanes) on the masked inputs, on both
    access widths: it agrees with float64 at the fp32 loss bars -- and without the rule that a -inf logit adds nothing it is NaN on the
    rows head, unit0 and single, so the model can tell the two recurrences apart."""
    import _parity as P
    hot = ER.MASKED_LABEL_ROW
    for K, V, nan_rows in ((16385, 1, ("head", "unit0", "single")), (32776, 8, ("head", "unit0"))):
        X, labels = ER.xent_masked_inputs(K, "f32")
        want = ER.xent_ref(X, labels)[0]
        got = ER.xent_long_model_f32(X, labels, V)
        assert got.dtype == np.float32 and got[hot] == np.inf
        l2, mx = P.errors(np.delete(got, hot), np.delete(want, hot))
        print("K %d V %d: model loss L2 %.2e max %.2e" % (K, V, l2, mx))
        assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (K, V, l2, mx)
        before = ER.xent_long_model_f32(X, labels, V, skip_masked=False)
        for name in nan_rows:
            assert np.isnan(before[ER.MASKS.index(name)]), (K, V, name, before)
        assert before[ER.MASKS.index("tail")] == got[ER.MASKS.index("tail")]       # the control: masked classes behind finite ones
    # finite rows: the rule changes no bit
    X, labels, _ = ER.xent_inputs(2, 16385, "f32", "uniform")
    assert np.array_equal(ER.xent_long_model_f32(X, labels, 1), ER.xent_long_model_f32(X, labels, 1, skip_masked=False))
    assert P.errors(ER.xent_long_model_f32(X, labels, 1), ER.xent_ref(X, labels)[0])[0] <= P.L2_BAR["f32"]
