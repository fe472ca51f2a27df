"""CPU tier of the simulated float formats (include/bsmm_quant.h, blocksparse_amd/quantize.py): the exported symbols, the struct mirror against
the header, argument checks that answer before anything is launched, and the NumPy definition ``quantize_test`` -- integer arithmetic on
the bit patterns -- against a per-element loop in exact rational arithmetic (tests/_quantize_ref.py) and, with ties to even, bit for bit
against torch's CPU casts to float16, bfloat16, float8_e5m2 and float8_e4m3fn.  The schedule, the statistics and the exponent rule are
checked against per-element loops.  No compute calls here."""
import ctypes
import os
import re

import numpy as np
import pytest

import _quantize_ref as QR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARG, UNSUPPORTED = -1, -2
F32, F16, BF16 = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from blocksparse_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def Q(lib):
    from blocksparse_amd import quantize
    return quantize


@pytest.fixture(scope="module")
def data():
    return QR.dataset()


def _header():
    return open(os.path.join(ROOT, "include", "bsmm_quant.h")).read()


def test_quant_header_symbols_exported_and_version_unchanged(lib):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = set(re.findall(r"\b(bsmm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(lib.QUANT_SYMBOLS) == {"bsmm_quantize", "bsmm_tensor_stats", "bsmm_quant_update_emax", "bsmm_quant_workspace_bytes"}
    others = set(lib.SYMBOLS) | set(lib.DIST_SYMBOLS) | set(lib.SPARSITY_SYMBOLS) | set(lib.OPTIM_SYMBOLS) | set(lib.OPTIM_LIST_SYMBOLS) | \
        set(lib.ADAFACTOR_SYMBOLS) | set(lib.NORM_SYMBOLS) | set(lib.EW_SYMBOLS) | set(lib.ENDS_SYMBOLS) | set(lib.BST_SYMBOLS) | set(lib.LSTM_SYMBOLS) | \
        set(lib.SELECT_SYMBOLS)
    assert not declared & others
    L = lib.load()
    raw = ctypes.CDLL(lib.LIB_PATH)
    for s in declared:
        assert hasattr(L, s), s
        getattr(raw, s)
    assert L.bsmm_version() == lib.ABI_VERSION == 128
    import blocksparse_amd
    for name in ("QuantizeSpec", "QuantizeState", "log_stats", "quantize_fwd", "quantize_update_emax", "tensor_stats", "reset_quantize_states"):
        assert getattr(blocksparse_amd, name) is getattr(blocksparse_amd.quantize, name), name
    for name in ("quantize", "quantize_test", "tensor_stats_test", "quantize_emax_test", "quantize_schedule_test"):
        assert callable(getattr(blocksparse_amd.quantize, name)), name


def test_struct_mirror_and_constants_match_the_header(lib):
    body = re.search(r"typedef struct bsmm_quant_args \{(.*?)\} bsmm_quant_args;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    ctype = {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "void*": ctypes.c_void_p, "size_t": ctypes.c_size_t}
    fields = [(m.group(2), ctype[m.group(1)]) for m in re.finditer(r"(int32_t|float|void\*|size_t)\s+(\w+);", body)]
    assert [f[0] for f in fields] == ["ebits", "fbits", "emax", "denorm", "round_mode", "group", "bias_pad", "stat_mode", "dtype", "stdv_mul",
                                      "workspace", "workspace_bytes", "stream"]
    A = lib.BsmmQuantArgs
    assert fields == [(f[0], f[1]) for f in A._fields_]
    # what a C compiler lays out: ten 4-byte members, then three 8-byte ones
    assert [getattr(A, n).offset for n, _ in fields] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48, 56] and ctypes.sizeof(A) == 64
    defs = dict((n, int(v)) for n, v in re.findall(r"#define (BSMM_QUANT_\w+) (\d+)", _header()))
    assert (defs["BSMM_QUANT_LANE_ELEMS"], defs["BSMM_QUANT_WG_ELEMS"], defs["BSMM_QUANT_MAX_GRID"], defs["BSMM_QUANT_GROUP"]) == \
        (lib.QUANT_LANE_ELEMS, lib.QUANT_WG_ELEMS, lib.QUANT_MAX_GRID, lib.QUANT_GROUP) == (8, 2048, 2048, 32)
    assert (defs["BSMM_QUANT_NEAREST_AWAY"], defs["BSMM_QUANT_NEAREST_EVEN"], defs["BSMM_QUANT_STOCHASTIC"]) == \
        (lib.QUANT_NEAREST_AWAY, lib.QUANT_NEAREST_EVEN, lib.QUANT_STOCHASTIC) == (0, 1, 2)


def test_quant_sources_read_no_environment_and_keep_no_state():
    src = ""
    for f in ("bsmm_quant.hip", "bsmm_quant_kernels.h"):
        src += open(os.path.join(ROOT, "blocksparse_amd", "csrc", f)).read()
    src = re.sub(r"//[^\n]*", "", src)                     # (the comments may say what the code does not do)
    for word in ("getenv", "hipMalloc", "hipFree", "Synchronize", "atomic", "static int", "static float", "static bool", "log2", "logb", "frexp"):
        assert word not in src, word
    assert src.count("ew_philox(") == 2 and "0xD2511F53" not in src          # the library's one generator, called, not copied
    vec = open(os.path.join(ROOT, "blocksparse_amd", "csrc", "bsmm_vec.h")).read()
    ew = open(os.path.join(ROOT, "blocksparse_amd", "csrc", "bsmm_ew_kernels.h")).read()
    assert vec.count("void ew_philox(") == 1 and "void ew_philox(" not in ew
    from blocksparse_amd import build
    assert "bsmm_quant.hip" in build.SOURCES


def _args(lib, **kw):
    d = dict(ebits=4, fbits=3, emax=8, denorm=1, round_mode=0, group=0, bias_pad=2, stat_mode=0, dtype=F32, stdv_mul=4.0, workspace=None,
             workspace_bytes=0, stream=None)
    d.update(kw)
    return lib.BsmmQuantArgs(**d)


def test_argument_checks_answer_before_any_launch(lib):
    """Every call here is wrong in exactly one way (the addresses are dummies that are never dereferenced), so none may reach a launch."""
    L = lib.load()
    one, n = ctypes.c_void_p(256), 64
    quant = lambda a, x=one, y=one, st=one, em=None, n=n: L.bsmm_quantize(x, y, st, em, n, ctypes.byref(a) if a is not None else None)
    assert quant(None) == ARG and quant(_args(lib), x=None) == ARG and quant(_args(lib), y=None) == ARG
    for bad in (dict(ebits=0), dict(ebits=9), dict(fbits=-1), dict(fbits=24), dict(round_mode=-1), dict(round_mode=3), dict(denorm=2), dict(dtype=3),
                dict(dtype=-1), dict(dtype=BF16, fbits=8), dict(group=16), dict(group=64), dict(group=-32), dict(bias_pad=1000)):
        assert quant(_args(lib, **bad)) == ARG, bad
    for bad_n in (0, -5, 1 << 31, 1 << 40):
        assert quant(_args(lib), n=bad_n) == ARG, bad_n
    for bad_n in (1, 31, 33, 48):
        assert quant(_args(lib, group=32), n=bad_n) == ARG, bad_n
    assert quant(_args(lib, round_mode=2), st=None) == ARG and quant(_args(lib, round_mode=2), st=ctypes.c_void_p(260)) == ARG
    assert quant(_args(lib), em=ctypes.c_void_p(258)) == ARG
    assert quant(_args(lib), x=ctypes.c_void_p(258)) == ARG and quant(_args(lib, dtype=BF16), y=ctypes.c_void_p(257)) == ARG
    assert quant(_args(lib, dtype=F16)) == UNSUPPORTED
    assert quant(_args(lib, dtype=F16, ebits=0)) == ARG and quant(_args(lib, dtype=F16), n=0) == ARG          # a bad argument comes first
    # the statistics
    need = L.bsmm_quant_workspace_bytes(n)
    assert need == 32 and L.bsmm_quant_workspace_bytes(0) == 0 and L.bsmm_quant_workspace_bytes(1 << 31) == 0
    sizes = [L.bsmm_quant_workspace_bytes(v) for v in (1, 2048, 2049, 2048 * 2048, 2048 * 2048 + 1, (1 << 31) - 1)]
    assert sizes == [32, 32, 64, 32 * 2048, 32 * 2048, 32 * 2048]
    stats = lambda x=one, n=n, dt=F32, sat=1.0, ftz=0.5, out=one, ws=one, wb=need: L.bsmm_tensor_stats(x, n, dt, sat, ftz, out, ws, wb, None)
    for bad in (dict(x=None), dict(out=None), dict(ws=None), dict(n=0), dict(n=1 << 31), dict(dt=3), dict(sat=-1.0), dict(ftz=float("nan")),
                dict(wb=need - 1), dict(ws=ctypes.c_void_p(260)), dict(out=ctypes.c_void_p(258)), dict(n=2049)):
        assert stats(**bad) == ARG, bad
    upd = lambda a, x=one, em=one, out=None, n=n: L.bsmm_quant_update_emax(x, n, ctypes.byref(a) if a is not None else None, em, out)
    ok = dict(workspace=256, workspace_bytes=need)
    assert upd(None) == ARG and upd(_args(lib, **ok), x=None) == ARG and upd(_args(lib, **ok), em=None) == ARG
    for bad in (dict(ebits=0), dict(fbits=24), dict(stat_mode=2), dict(dtype=5), dict(dtype=BF16, fbits=8), dict(workspace=None),
                dict(workspace=260), dict(workspace_bytes=need - 1), dict(stdv_mul=float("nan"))):
        assert upd(_args(lib, **dict(ok, **bad))) == ARG, bad
    assert upd(_args(lib, **ok), em=ctypes.c_void_p(258)) == ARG and upd(_args(lib, **ok), n=0) == ARG and upd(_args(lib, **ok), n=2049) == ARG


def test_python_argument_errors(Q):
    import torch
    x = torch.zeros(64)
    spec = Q.QuantizeSpec()
    for call in (lambda: Q.quantize(x, spec), lambda: Q.quantize_fwd(x, spec), lambda: Q.tensor_stats(x), lambda: Q.log_stats(x, 1),
                 lambda: Q.quantize_update_emax(x, spec, torch.zeros(1, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    for bad in (dict(ebits=0), dict(ebits=9), dict(fbits=24), dict(stochastic=3), dict(group=16), dict(mode=2), dict(stochastic=1, nearest_even=True)):
        with pytest.raises(ValueError):
            Q.QuantizeSpec(**bad)
    s = Q.QuantizeSpec(5, 2, stochastic=2, group=32, nearest_even=False, logfile="a")
    c = Q.QuantizeSpec(copy=s)
    assert (c.ebits, c.fbits, c.emax, c.stoch, c.group, c.logfile, c.round_mode) == (5, 2, 15, 2, 32, "a", 2)
    assert Q.QuantizeSpec().emax == 7 and Q.QuantizeSpec(nearest_even=True).round_mode == 1 and Q.QuantizeSpec().round_mode == 0
    with pytest.raises(ValueError):
        Q.log_stats(x, 1, freq=48)


# ---- the definition -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("denorm", [True, False], ids=["denorm", "flush"])
@pytest.mark.parametrize("mode", [0, 1, 2], ids=["away", "even", "stochastic"])
def test_definition_equals_the_rational_loop(Q, data, mode, denorm):
    rng = np.random.default_rng(mode)
    r = rng.integers(0, 2 ** 32, data.size, dtype=np.uint64).astype(np.uint32)
    formats = QR.FORMATS + [(8, 7, 127), (5, 10, 16), (1, 3, 0), (3, 0, 4), (8, 23, 127), (4, 3, -200), (4, 3, 300), (2, 23, 1)]
    for ebits, fbits, emax in formats:
        spec = Q.QuantizeSpec(ebits, fbits, emax, stochastic=1 if mode == 2 else 0, denorm=denorm, nearest_even=mode == 1)
        sub = data if (ebits, fbits, emax) in QR.FORMATS else data[::7]
        rs = r[:sub.size]
        got = Q._round_bits(Q._bits(sub), spec, emax, rs).astype(np.uint32).view(np.float32)
        want = QR.q_loop_array(sub, ebits, fbits, emax, denorm, mode, rs)
        assert QR.same_bits(got, want), (ebits, fbits, emax, np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0][:5])
        if mode != 2:
            assert QR.same_bits(Q.quantize_test(sub, spec), want)
        # the sign survives every case, a NaN stays a NaN, and nothing stored is an fp32 subnormal or an inf
        assert np.array_equal(np.signbit(got), np.signbit(sub)) and np.array_equal(np.isnan(got), np.isnan(sub))
        mag = got.view(np.uint32) & 0x7fffffff
        assert ((mag == 0) | ((mag >= 0x00800000) & (mag < 0x7f800000)) | np.isnan(got)).all()


def test_random_words_are_the_philox_words(Q):
    import _ewops_ref as ER
    seed, offset = 0x123456789abcdef, (5 << 32) + 7
    got = Q.random_words(11, seed, offset)
    for i in range(11):
        w = ER.philox((i // 4, 0, offset & 0xffffffff, offset >> 32), (seed & 0xffffffff, seed >> 32))
        assert int(got[i]) == w[i % 4], i
    x = np.full(40, 1.046875, dtype=np.float32)
    spec = Q.QuantizeSpec(4, 3, 8, stochastic=2)
    want = QR.q_loop_array(x, 4, 3, 8, True, 2, Q.random_words(40, 3, 9))
    assert QR.same_bits(Q.quantize_test(x, spec, seed=3, offset=9), want)
    assert not QR.same_bits(Q.quantize_test(x, spec, seed=3, offset=10), want)


def test_small_grid_identity_and_extreme_formats(Q):
    xs = np.concatenate([np.linspace(0, 8, 4097), [np.inf, 1e30]]).astype(np.float32)
    for mode_kw in (dict(), dict(nearest_even=True)):
        got = Q.quantize_test(np.concatenate([xs, -xs]), Q.QuantizeSpec(2, 1, 2, **mode_kw))
        assert sorted(set(np.abs(got).tolist())) == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert [float(g) for g in QR.grid(2, 1, 2)] == [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    # fbits = 23 is the identity inside the range (ebits = 8: every normal fp32 value)
    rng = np.random.default_rng(1)
    x = (rng.normal(size=4096) * np.exp(rng.uniform(-80, 80, 4096))).astype(np.float32)
    x = x[np.abs(x) >= 2.0 ** -125]
    for kw in (dict(), dict(nearest_even=True), dict(stochastic=1)):
        assert QR.same_bits(Q.quantize_test(x, Q.QuantizeSpec(8, 23, 127, denorm=False, **kw)), x)
    inside = x[(np.abs(x) >= 2.0 ** -6) & (np.abs(x) < 2.0 ** 9)]
    assert inside.size > 100 and QR.same_bits(Q.quantize_test(inside, Q.QuantizeSpec(4, 23, 8, denorm=False)), inside)
    # ebits = 1: one binade (plus the subnormals); fbits = 0: powers of two
    got = np.abs(Q.quantize_test(xs, Q.QuantizeSpec(1, 2, 0)))
    assert sorted(set(got.tolist())) == [0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 1.75]
    got = np.abs(Q.quantize_test(xs, Q.QuantizeSpec(3, 0, 2)))
    assert sorted(set(got.tolist())) == [0.0] + [2.0 ** e for e in range(-4, 3)]


CASTS = [("float16", (5, 10, 16), 65504.0, 0.0), ("bfloat16", (8, 7, 127), 3.3e38, 2.0 ** -118), ("float8_e5m2", (5, 2, 16), 57344.0, 0.0),
         ("float8_e4m3fn", (4, 3, 8), 440.0, 0.0)]


@pytest.mark.parametrize("cast", CASTS, ids=[c[0] for c in CASTS])
def test_ties_to_even_equals_the_torch_cpu_casts_bit_for_bit(Q, cast):
    import torch
    name, (ebits, fbits, emax), below, floor = cast
    spec = Q.QuantizeSpec(ebits, fbits, emax, nearest_even=True)
    rng = np.random.default_rng(2)
    x = (rng.normal(size=200000) * np.exp(rng.uniform(-70.0 if floor else -30.0, 12.0, 200000))).astype(np.float32)
    x = np.clip(x, -np.nextafter(np.float32(below), np.float32(0)), np.nextafter(np.float32(below), np.float32(0)))
    if floor:
        x = np.where(np.abs(x) < floor, np.copysign(np.float32(floor), x), x).astype(np.float32)
    sets = [x]
    if fbits <= 3:                                           # all 63 488 finite fp16 bit patterns, clipped into the range
        h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
        h = h[np.isfinite(h)].astype(np.float32)
        assert h.size == 63488
        sets.append(np.clip(h, -np.nextafter(np.float32(below), np.float32(0)), np.nextafter(np.float32(below), np.float32(0))))
    for v in sets:
        assert (np.abs(v) < below).all() and (np.abs(v) >= floor).all() and np.isfinite(v).all()          # nothing had to be left out
        want = torch.from_numpy(v).to(getattr(torch, name)).float().numpy()
        got = Q.quantize_test(v, spec)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got.view(np.uint32) != want.view(np.uint32)).sum())


def _two_step(x, ebits, fbits, emax):
    """The mutant: round at the value's own exponent first, then onto the subnormal grid (what the reference does)."""
    first = QR.q_loop(x, 8, fbits, 127, False, 0)[0]
    return QR.q_loop(first, ebits, fbits, emax, True, 0)[0]


def test_one_rounding_in_the_subnormal_range(Q):
    x = np.float32(2.484375 * 2.0 ** -9)
    assert _two_step(x, 4, 3, 8) == 3 * 2.0 ** -9
    assert QR.q_loop(x, 4, 3, 8, True, 0)[0] == 2 * 2.0 ** -9
    assert float(Q.quantize_test(np.array([x]), Q.QuantizeSpec(4, 3, 8))[0]) == 2 * 2.0 ** -9


def test_ties_away_and_ties_even_differ_exactly_on_halfway_points_with_lo_even(Q, data):
    for ebits, fbits, emax in QR.FORMATS:
        maxf = float(QR.fmt(ebits, fbits, emax, True)[3])
        v = data[np.abs(data) < maxf]
        away = Q.quantize_test(v, Q.QuantizeSpec(ebits, fbits, emax))
        even = Q.quantize_test(v, Q.QuantizeSpec(ebits, fbits, emax, nearest_even=True))
        info = [QR.q_loop(t, ebits, fbits, emax, True, 0)[1:] for t in v]
        want = np.array([frac is not None and 2 * frac == 1 and lo % 2 == 0 for lo, frac in info])
        assert want.sum() >= 2 * (2 ** fbits) and np.array_equal(away.view(np.uint32) != even.view(np.uint32), want)


def test_idempotent_and_bf16_storage(Q, data):
    for ebits, fbits, emax in QR.FORMATS + [(8, 7, 127)]:
        for kw in (dict(), dict(nearest_even=True), dict(stochastic=1), dict(denorm=False)):
            spec = Q.QuantizeSpec(ebits, fbits, emax, **kw)
            once = Q.quantize_test(data, spec, seed=1)
            assert QR.same_bits(Q.quantize_test(once, spec, seed=2), once), (ebits, fbits, kw)
            # fbits <= 7: the result of a bf16 tensor's upcast is a bf16 value again, and the same whichever storage type carries it
            up = QR.to_bf16(data)
            got = Q.quantize_test(up, spec, seed=1)
            assert QR.same_bits(QR.to_bf16(got), got)


def test_group_mode_equals_slices_with_the_assigned_exponent(Q, data):
    rng = np.random.default_rng(4)
    x = (rng.normal(size=32 * 12) * np.repeat(np.exp(rng.uniform(-12, 12, 12)), 32)).astype(np.float32)
    x[32:64] = 0.0                                          # a run without a finite non-zero element: the spec's emax
    x[64:96] = [np.inf, -np.inf, np.nan] + [0.0] * 29
    x[100] = np.inf                                         # not in the max of its run
    x[130] = np.nan
    x[160:192] = 1e-40                                      # fp32 subnormals: e = -127
    for kw in (dict(bias_pad=0), dict(bias_pad=2, nearest_even=True), dict(bias_pad=-1, stochastic=1, denorm=False)):
        spec = Q.QuantizeSpec(4, 3, 5, group=32, **kw)
        flat = Q.QuantizeSpec(4, 3, 5, **kw)
        got = Q.quantize_test(x, spec, seed=7, offset=3)
        em = Q.group_emax_test(x, spec)
        r = Q.random_words(x.size, 7, 3)
        for g in range(12):
            run = x[32 * g:32 * g + 32]
            fin = np.abs(run[np.isfinite(run) & (run != 0)])
            if fin.size == 0:
                want_e = 5
            else:
                top = float(fin.max())
                want_e = (int(np.floor(np.log2(top))) if top >= 2.0 ** -126 else -127) + spec.bias_pad
            assert int(em[g]) == want_e, (g, em[g], want_e)
            want = QR.q_loop_array(run, 4, 3, want_e, spec.denorm, spec.round_mode, r[32 * g:32 * g + 32])
            assert QR.same_bits(got[32 * g:32 * g + 32], want), g
        assert em[1] == em[2] == 5
    with pytest.raises(ValueError):
        Q.quantize_test(x[:33], Q.QuantizeSpec(group=32))


def test_stochastic_share_follows_the_fraction(Q):
    n = 1 << 16
    spec = Q.QuantizeSpec(4, 3, 8, stochastic=1)
    x = np.full(n, 1.0 + 3.0 / 64.0, dtype=np.float32)      # step 1/8 at e = 0: t = 8 + 3/8
    for seed in (0, 1):
        got = Q.quantize_test(x, spec, seed=seed, offset=seed)
        assert set(got.tolist()) == {1.0, 1.125}
        share = (got == 1.125).mean()
        assert abs(share - 0.375) <= 5 * np.sqrt(0.375 * 0.625 / n), share
    exact = np.full(n, 1.125, dtype=np.float32)             # frac = 0 never rounds up
    assert (Q.quantize_test(exact, spec, seed=5) == 1.125).all()


def test_schedule(Q):
    assert Q.quantize_schedule_test(8, 48) == [1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 24, 28, 32, 40, 48]
    assert Q.quantize_schedule_test(1, 9) == list(range(1, 10))
    assert Q.quantize_schedule_test(0, 9) == []
    got = Q.quantize_schedule_test(1024, 20000)
    assert got[:8] == [1, 2, 3, 4, 5, 6, 8, 10] and all(b - a == 1024 for a, b in zip(got[-5:], got[-4:]))


def test_statistics_and_exponent_rule_against_loops(Q):
    rng = np.random.default_rng(6)
    x = (rng.normal(size=3000) * np.exp(rng.uniform(-20, 6, 3000))).astype(np.float32)
    x[5], x[17], x[99], x[100] = np.inf, np.nan, 0.0, -np.inf
    for sat, ftz in ((65504.0, 2.0 ** -24), (1.0, 1e-3), (0.0, 0.0)):
        np.testing.assert_allclose(Q.tensor_stats_test(x, sat, ftz), QR.stats_loop(x, sat, ftz), rtol=1e-12, atol=0)
    s = Q.tensor_stats_test(x)
    assert s[5] == 3 and s[6] == 3000 and np.isfinite(s[2]) and s[2] == np.abs(x[np.isfinite(x)]).max()          # an inf is counted and not maxed
    for kw in (dict(mode=0, bias_pad=2), dict(mode=1, bias_pad=0, stdv_mul=4.0), dict(mode=1, bias_pad=-3, stdv_mul=0.5)):
        spec = Q.QuantizeSpec(4, 3, 8, **kw)
        want, M = QR.emax_loop(x, 4, spec.bias_pad, spec.mode, spec.stdv_mul, 8)
        assert QR.clear_of_a_power_of_two(M) and Q.quantize_emax_test(x, spec, 8) == want
    spec = Q.QuantizeSpec(4, 3, 8)
    assert Q.quantize_emax_test(np.zeros(64, dtype=np.float32), spec, 3) == 3                  # all zeros: unchanged
    assert Q.quantize_emax_test(np.full(8, np.nan, dtype=np.float32), spec, -4) == -4          # nothing finite: unchanged
    assert Q.quantize_emax_test(np.full(8, 1e30, dtype=np.float32), Q.QuantizeSpec(5, 2), 0) == 101 and \
        Q.quantize_emax_test(np.full(8, 1e-38, dtype=np.float32), Q.QuantizeSpec(4, 3), 0) == -112          # clamped at nexp - 127
