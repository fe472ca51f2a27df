"""CPU tier of Adafactor (include/bsmm_adafactor.h, blocksparse_amd/optimize.py): the exported symbols, the struct mirror, argument checks
that answer before anything is launched, the host arithmetic (workspace size, decay schedule), the float64 definitions of
tests/_adafactor_ref.py against per-element loops, and the float32 model of the kernels' summation order against every bar of the GPU
tier on every named case.  No compute calls here.

The mutant.  Summing x^2 in one sequential fp32 chain -- every other sum as the kernels do it -- misses the bars at (300, 520), where
the clip is active in the first two steps (float64 RMS 1.073 / 1.009 / 0.998): param L2 6.8e-6 (bar 2e-6), param max 1.4e-4 (bar 2e-5),
update L2 2.4e-5 (bar 1e-5).  The kernels' order gives 4.6e-8, 7.9e-7 and 1.6e-7 on the same case, so the case is not enlarged."""
import ctypes
import os
import re

import numpy as np
import pytest

import _adafactor_cases as AC
import _adafactor_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUP, WS = -1, -2, -3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import _lib
    return _lib


def _header():
    return open(os.path.join(ROOT, "include", "bsmm_adafactor.h")).read()


def test_adafactor_symbols_exported(lib):
    from blocksparse_amd import build
    import blocksparse_amd
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(bsmm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.ADAFACTOR_SYMBOLS), declared ^ set(lib.ADAFACTOR_SYMBOLS)
    L = lib.load()
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in declared:
        assert hasattr(L, s), s
        getattr(raw, s)
    assert L.bsmm_version() == lib.ABI_VERSION == 128          # new symbols only: bsmm.h and its version stay as they were
    assert "bsmm_adafactor.hip" in build.SOURCES
    for name in ("adafactor_step", "adafactor_decay", "AdafactorOptimizer"):
        assert hasattr(blocksparse_amd, name), name


def test_adafactor_struct_layout_matches_header(lib):
    body = re.search(r"typedef struct bsmm_adafactor_args \{(.*?)\} bsmm_adafactor_args;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    lines = [ln for ln in body.splitlines() if ";" in ln]
    names = [re.search(r"(\w+)\s*;", ln).group(1) for ln in lines]
    assert names == [f[0] for f in lib.BsmmAdafactorArgs._fields_]
    assert names == ["param", "cv", "rv", "grad", "param16", "gate", "norm_scale", "workspace", "workspace_bytes", "stream", "rows", "cols",
                     "bsize", "grad_dtype", "param16_dtype", "zero_infs", "zero_nans", "lr", "decay", "epsilon", "clip_thresh", "grad_scale",
                     "saturate"]
    kinds = {"ptr": 0, "size_t": 0, "int32_t": 0, "float": 0}
    for ln in lines:
        kinds["ptr" if "*" in ln else re.search(r"(size_t|int32_t|float)", ln).group(1)] += 1
    assert kinds == {"ptr": 9, "size_t": 3, "int32_t": 5, "float": 6}
    assert ctypes.sizeof(lib.BsmmAdafactorArgs) == 9 * 8 + 3 * 8 + 5 * 4 + 6 * 4 + 4      # (+ 4: tail padding to the pointers' alignment)
    A = lib.BsmmAdafactorArgs
    assert A.workspace_bytes.offset == 64 and A.stream.offset == 72 and A.rows.offset == 80 and A.bsize.offset == 96 and A.lr.offset == 116


def test_adafactor_sources_read_no_environment_and_keep_no_state():
    src = ""
    for f in ("bsmm_adafactor.hip", "bsmm_adafactor_kernels.h"):
        src += open(os.path.join(ROOT, "blocksparse_amd", "csrc", f)).read()
    src = re.sub(r"//[^\n]*", "", src)                     # (the comments may say what the code does not do)
    for word in ("getenv", "hipMalloc", "hipFree", "hipMemset", "Synchronize", "atomic", "asm"):
        assert word not in src, word


def _args(lib, **kw):
    a = lib.BsmmAdafactorArgs()
    for f in ("param", "cv", "rv", "grad", "workspace"):
        setattr(a, f, 256)                                  # non-null, aligned dummy addresses: never dereferenced
    a.rows, a.cols, a.bsize, a.grad_dtype = 8, 1024, 32, lib.F32
    a.lr, a.decay, a.epsilon, a.clip_thresh, a.grad_scale = 1e-3, 0.999, 1e-30, 1.0, 1.0
    a.workspace_bytes = 1 << 40
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_argument_checks_answer_before_any_launch(lib):
    L = lib.load()
    call = lambda **kw: L.bsmm_adafactor(ctypes.byref(_args(lib, **kw)))
    assert L.bsmm_adafactor(None) == ARG
    for f in ("param", "cv", "grad", "rv"):
        assert call(**{f: None}) == ARG, f
    assert call(bsize=0, rows=2, cols=5, rv=None) == ARG             # rows > 1 needs rv
    assert call(bsize=0, rows=3, cols=8, gate=256) == ARG            # a dense tensor takes no gate
    assert call(bsize=0, rows=1, cols=8, gate=256) == ARG
    assert call(rows=0) == ARG and call(cols=0) == ARG and call(bsize=0, rows=0, cols=4) == ARG
    assert call(cols=1000) == ARG and call(cols=64) == ARG            # cols != bsize^2
    assert call(bsize=12, cols=144) == UNSUP and call(bsize=-8, cols=64) == UNSUP
    assert call(rows=1 << 31) == UNSUP
    assert call(grad_dtype=3) == UNSUP and call(grad_dtype=-1) == UNSUP
    assert call(param16=256, param16_dtype=lib.F32) == UNSUP and call(param16=256, param16_dtype=9) == UNSUP
    assert call(clip_thresh=0.0) == ARG and call(clip_thresh=-1.0) == ARG and call(clip_thresh=float("nan")) == ARG
    for rows, cols, bsize in ((8, 1024, 32), (300, 520, 0), (1, 63, 0)):
        need = L.bsmm_adafactor_workspace_bytes(rows, cols, bsize)
        assert need > 0
        shape = dict(rows=rows, cols=cols, bsize=bsize)
        assert call(workspace=None, **shape) == WS
        assert call(workspace_bytes=need - 1, **shape) == WS
        assert call(workspace_bytes=0, **shape) == WS
        assert call(workspace=258, workspace_bytes=need, **shape) == WS                 # not 4-byte aligned


def test_workspace_bytes_monotone_and_aligned(lib):
    W = lib.load().bsmm_adafactor_workspace_bytes
    assert W(0, 5, 0) == 0 and W(5, 0, 0) == 0 and W(4, 1000, 32) == 0 and W(4, 144, 12) == 0 and W(1 << 31, 64, 8) == 0 and W(0, 64, 8) == 0
    assert W(1 << 62, 1 << 62, 0) == 0                                                   # overflows
    sizes = [1, 2, 3, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 4099, 65536, 1 << 20]
    for fixed in (1, 2, 300, 4099):
        for along in ("rows", "cols"):
            last = 0
            for n in sizes:
                b = W(n, fixed, 0) if along == "rows" else W(fixed, n, 0)
                assert b >= last and b > 0 and b % 4 == 0, (along, fixed, n, b, last)
                last = b
    for bs in (8, 16, 32, 64):
        last = 0
        for n in sizes:
            b = W(n, bs * bs, bs)
            assert b >= last and b > 0 and b % 4 == 0
            last = b
    # no full-size scratch: the 2-d form takes about 1 / 32 of the tensor, the other forms next to nothing
    assert W(4096, 4096, 0) <= 4096 * 4096 * 4 // 16 and W(1, 1 << 20, 0) <= 16384 and W(3277, 1024, 32) <= 16384 + 3277 * 4


def test_adafactor_decay_matches_the_accumulators():
    from blocksparse_amd import adafactor_decay
    for b2 in (0.999, 0.98):
        for t in range(1, 6):
            want = AR.decay_loop(t, b2)
            assert abs(adafactor_decay(t, b2) - want) <= 1e-12 * want, (t, b2)
            assert abs(want - b2 * (1 - b2 ** t) / (1 - b2 ** (2 * t))) <= 1e-12 * want
            assert adafactor_decay(t, b2, zero_init_variables=True) == AR.decay_loop(t, b2, True) == b2
    assert abs(adafactor_decay(1, 0.999) - 0.999 / 1.999) < 1e-12


def test_cpu_tensors_and_bad_shapes_are_rejected_loudly():
    import torch
    from blocksparse_amd import adafactor_step, AdafactorOptimizer
    w = torch.zeros(4, 8)
    for call in (lambda: adafactor_step(w, w, torch.zeros(8), torch.zeros(4)), lambda: AdafactorOptimizer([w])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


SETTINGS = [dict(), dict(grad_scale=0.5, norm_scale=0.7, saturate=2.0, zero_infs=True, zero_nans=True, lr=1e-3, decay=0.6, clip_thresh=0.5),
            dict(zero_infs=True, zero_nans=True, epsilon=1e-8), dict(saturate=1.0, zero_nans=True, decay=0.3), dict(norm_scale=0.0)]


def _same(a, b, ctx):
    for x, y, name in zip(a[:3], b[:3], ("p", "cv", "rv")):
        assert (x is None) == (y is None), (ctx, name)
        if x is not None:
            np.testing.assert_allclose(x, y, rtol=1e-11, atol=0, err_msg=str((ctx, name)))
    assert abs(a[3] - b[3]) <= 1e-11 * max(abs(b[3]), 1e-300), ctx


def test_float64_definitions_against_per_element_loops():
    rng = np.random.RandomState(3)
    for rows, cols in ((3, 5), (2, 7), (1, 6), (1, 1)):
        n = rows * cols
        p, g = rng.normal(0, 0.01, n).astype(np.float32), rng.normal(0, 0.1, n).astype(np.float32)
        g[::4] *= 50
        if n > 5:
            g[1], g[5] = np.inf, np.nan
        cv, rv = rng.uniform(0, 1e-2, cols).astype(np.float32), rng.uniform(0, 1e-2, rows).astype(np.float32)
        for kw in SETTINGS:
            planted = kw.get("zero_infs") and kw.get("zero_nans")                     # (without both flags the planted values would arrive)
            gg = g if planted else np.where(np.isfinite(g), g, np.float32(0.3))
            _same(AR.dense(p, cv, rv, gg, rows, cols, **kw), AR.dense_loop(p, cv, rv, gg, rows, cols, **kw), (rows, cols, kw))
    bs, nb = 8, 5
    n = nb * bs * bs
    p, g = rng.normal(0, 0.01, n).astype(np.float32), rng.normal(0, 0.1, n).astype(np.float32)
    g[::7] *= 50
    cv, rv = rng.uniform(0, 1e-2, nb * bs).astype(np.float32), rng.uniform(0, 1e-2, nb * bs).astype(np.float32)
    gate = np.array([0, 1, 1, 0, 1], dtype=np.float32)
    g[:bs * bs] = np.nan                                                                # a gated-off block is never read
    for kw in SETTINGS[:2] + SETTINGS[4:]:
        a = AR.blocks(p, cv, rv, g, nb, bs, gate=gate, **kw)
        _same(a, AR.blocks_loop(p, cv, rv, g, nb, bs, gate=gate, **kw), ("blocks", kw))
        for x, old, per in ((a[0], p, bs * bs), (a[1], cv, bs), (a[2], rv, bs)):
            assert np.array_equal(x.reshape(nb, per)[gate == 0], old.astype(np.float64).reshape(nb, per)[gate == 0])
    a = AR.blocks(p, cv, rv, g, nb, bs, gate=np.zeros(nb, dtype=np.float32))
    assert np.array_equal(a[0], p.astype(np.float64)) and np.array_equal(a[1], cv.astype(np.float64))
    ungated = AR.blocks(p[bs * bs:2 * bs * bs], cv[bs:2 * bs], rv[bs:2 * bs], g[bs * bs:2 * bs * bs], 1, bs)
    _same(ungated, AR.dense(p[bs * bs:2 * bs * bs], cv[bs:2 * bs], rv[bs:2 * bs], g[bs * bs:2 * bs * bs], bs, bs), "one block is a matrix")


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_float32_model_passes_every_bar_of_the_gpu_tier(name):
    c = AC.case(name)
    p, cv, rv = AC.model_steps(c)
    AC.check(c, p, cv, rv, "model")
    live = c.live
    assert np.array_equal(p[~live], c.p[~live]) and np.array_equal(cv[~c.live_slots], c.cv[~c.live_slots])      # gated-off blocks keep their bits
    if c.form == "2d":
        dead = np.zeros((c.rows, c.cols), dtype=bool)
        dead[c.rows // 2, :] = True
        assert np.array_equal(p[dead.reshape(-1)], c.p[dead.reshape(-1)])              # rows of zeros keep param's bits


def test_clip_coverage_of_the_named_cases():
    forms = lambda names: sorted(AC.case(n).form for n in names)
    assert forms(AC.CLIP_ACTIVE) == ["1d", "2d", "block"]
    assert forms(AC.CLIP_INACTIVE + AC.CLIP_INACTIVE_FIRST_STEP) == ["1d", "2d", "block"]
    for n in AC.CLIP_ACTIVE:
        assert min(AC.case(n).rms) > 1.0, (n, AC.case(n).rms)
    for n in AC.CLIP_INACTIVE:
        assert max(AC.case(n).rms) < 1.0, (n, AC.case(n).rms)
    for n in AC.CLIP_INACTIVE_FIRST_STEP:
        assert AC.case(n).rms[0] < 1.0, (n, AC.case(n).rms)


def test_sequential_x2_chain_mutant_misses_the_bars_at_300x520():
    c = AC.case("2d-300x520-clip")
    assert (c.rows, c.cols) == (300, 520) and c.rms[0] > 1.0 and c.rms[1] > 1.0
    fig = AC.figures(c, *AC.model_steps(c, x2_chain=True))
    print("mutant (x^2 in one chain) at (300, 520):", fig)
    missed = [k for k, _, _ in AC.failures(fig)]
    assert "param_l2" in missed and "update_l2" in missed, fig
    assert fig["cv_rel"] <= AC.MOMENT_BAR and fig["rv_rel"] <= AC.MOMENT_BAR           # (the moments do not pass through that sum)


def test_dead_row_and_column_on_zero_slots_give_finite_moments_and_zero_x():
    rows, cols = 6, 9
    rng = np.random.RandomState(8)
    g = rng.normal(0, 0.1, (rows, cols)).astype(np.float32)
    g[2, :] = 0
    g[:, 4] = 0
    p = rng.normal(0, 0.01, rows * cols).astype(np.float32)
    for fn in (AR.dense, AR.model_dense):
        p2, cv2, rv2, rms = fn(p, np.zeros(cols, np.float32), np.zeros(rows, np.float32), g, rows, cols, decay=0.5, lr=1e-3)
        assert np.isfinite(cv2).all() and np.isfinite(rv2).all() and (cv2 > 0).all() and (rv2 > 0).all() and np.isfinite(p2).all()
        moved = (np.asarray(p2, dtype=np.float64) != p).reshape(rows, cols)
        assert not moved[2, :].any() and not moved[:, 4].any() and moved[0, 0] and np.isfinite(rms) and rms > 0
    p2, cv2, _, _ = AR.model_dense(p[:cols], np.zeros(cols, np.float32), None, g[2], 1, cols, decay=0.5)
    assert np.isfinite(cv2).all() and np.array_equal(p2, p[:cols])                      # the 1-d form on a dead vector: x == 0 everywhere
