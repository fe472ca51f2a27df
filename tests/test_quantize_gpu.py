"""GPU tier of the simulated float formats (include/bsmm_quant.h, blocksparse_amd/quantize.py).  Every quantized value is compared BIT FOR BIT
with ``quantize_test`` (the definition is integer arithmetic: there is no tolerance; where a NaN is expected a NaN must stand).  Sizes sit
around the units the header exports (a lane's 8 elements, a workgroup's 2048, the group of 32) and one lies past grid cap x workgroup span,
so the stride loop runs twice.  The statistics: counts and max exact, mean and deviation inside the fp32 bars of tests/_parity.py."""
import re
import os

import numpy as np
import pytest

import _parity as P
import _quantize_ref as QR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5eed5eed1234
_defs = dict((n, int(v)) for n, v in re.findall(r"#define (BSMM_QUANT_\w+) (\d+)", open(os.path.join(ROOT, "include", "bsmm_quant.h")).read()))
LANE, WG, CAP, GROUP = _defs["BSMM_QUANT_LANE_ELEMS"], _defs["BSMM_QUANT_WG_ELEMS"], _defs["BSMM_QUANT_MAX_GRID"], _defs["BSMM_QUANT_GROUP"]
SIZES = [1, LANE - 1, LANE, LANE + 1, GROUP - 1, GROUP, GROUP + 1, WG - 1, WG, WG + 1, CAP * WG + 1]
FORMATS = [(4, 3, 8), (5, 2, 16), (2, 1, 2), (8, 7, 127), (5, 10, 16)]


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from blocksparse_amd import quantize, ewops
    return torch, quantize, ewops


@pytest.fixture(scope="module")
def data():
    return QR.dataset()


def dev(torch, x, dtype):
    """float32 values (bf16: values bf16 holds) -> a device tensor of the storage type."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    return t.bfloat16() if dtype == "bf16" else t


def values(n, dtype, seed, data=None):
    rng = np.random.default_rng(seed)
    x = (rng.normal(size=n) * np.exp(rng.uniform(-14.0, 8.0, n))).astype(np.float32)
    if data is not None:
        x[:min(n, data.size)] = data[:n]
    return QR.to_bf16(x) if dtype == "bf16" else x


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("n", SIZES)
def test_sizes_around_every_unit(env, data, n, dtype):
    torch, Q, ewops = env
    x = values(n, dtype, n, data if n < CAP * WG else None)
    xd = dev(torch, x, dtype)
    big = n > CAP * WG
    specs = [Q.QuantizeSpec(4, 3, 8, stochastic=2)] if big else [Q.QuantizeSpec(4, 3, 8), Q.QuantizeSpec(5, 2, 16, stochastic=2, denorm=False)]
    for i, spec in enumerate(specs):
        ewops.set_entropy(SEED, offset=n + i)
        got = P.to_host(Q.quantize_fwd(xd, spec))
        assert QR.same_bits(got, Q.quantize_test(x, spec, seed=SEED, offset=n + i)), (n, dtype, i)
    m = n + (-n) % GROUP                                      # the next multiple of the group: the block-scaled mode
    if m != n and not (n % GROUP in (1, GROUP - 1)):
        return
    x = values(m, dtype, m + 1, data if not big else None)
    x[:GROUP] = 0.0
    spec = Q.QuantizeSpec(4, 3, 8, group=GROUP, bias_pad=0, nearest_even=True)
    assert QR.same_bits(P.to_host(Q.quantize_fwd(dev(torch, x, dtype), spec)), Q.quantize_test(x, spec)), (m, dtype, "group")


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_formats_modes_and_flush_on_the_data_set(env, data, dtype):
    torch, Q, ewops = env
    x = QR.to_bf16(data) if dtype == "bf16" else data
    xd = dev(torch, x, dtype)
    ran = 0
    for ebits, fbits, emax in FORMATS:
        if dtype == "bf16" and fbits > 7:
            with pytest.raises(ValueError):
                Q.quantize_fwd(xd, Q.QuantizeSpec(ebits, fbits, emax))
            continue
        for kw in (dict(), dict(nearest_even=True), dict(stochastic=1)):
            for denorm in (True, False):
                spec = Q.QuantizeSpec(ebits, fbits, emax, denorm=denorm, **kw)
                ewops.set_entropy(SEED, offset=ran)
                got = P.to_host(Q.quantize_fwd(xd, spec))
                assert QR.same_bits(got, Q.quantize_test(x, spec, seed=SEED, offset=ran)), (dtype, ebits, fbits, kw, denorm)
                ran += 1
    assert ran == (30 if dtype == "f32" else 24)
    with pytest.raises(ValueError):
        Q.quantize_fwd(xd.half(), Q.QuantizeSpec())


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_access_widths_and_in_place(env, data, dtype):
    torch, Q, ewops = env
    n = 3 * WG + 5
    x = values(n, dtype, 3, data)
    xd = dev(torch, x, dtype)
    off = torch.empty(n + 1, dtype=xd.dtype, device="cuda")[1:]          # one element off: the element path
    off.copy_(xd)
    assert xd.data_ptr() % 16 == 0 and off.data_ptr() % 16 != 0 and off.is_contiguous()
    for spec in (Q.QuantizeSpec(4, 3, 8), Q.QuantizeSpec(5, 2, 16, stochastic=1)):
        ewops.set_entropy(SEED, offset=1)
        wide = Q.quantize_fwd(xd, spec)
        ewops.set_entropy(SEED, offset=1)
        narrow = Q.quantize_fwd(off, spec)
        out_off = torch.empty(n + 1, dtype=xd.dtype, device="cuda")[1:]
        ewops.set_entropy(SEED, offset=1)
        Q.quantize_fwd(xd, spec, out=out_off)                          # aligned in, unaligned out
        ewops.set_entropy(SEED, offset=1)
        inplace = xd.clone()
        assert Q.quantize_fwd(inplace, spec, out=inplace) is inplace
        want = Q.quantize_test(x, spec, seed=SEED, offset=1)
        for name, t in (("wide", wide), ("narrow", narrow), ("out_off", out_off), ("inplace", inplace)):
            assert QR.same_bits(P.to_host(t), want), (dtype, name)
    g = Q.QuantizeSpec(4, 3, 8, group=GROUP)
    m = n - n % GROUP
    assert QR.same_bits(P.to_host(Q.quantize_fwd(off[:m], g)), Q.quantize_test(x[:m], g))


def _with_M(x, spec, target):
    """x scaled by a power-of-two-free factor so that the deciding quantity M sits at ``target`` (1.5 * 2^k: clear of every power of two)."""
    s = QR.stats_loop(x, 0.0, 0.0)
    M = s[0] + spec.stdv_mul * s[1] if spec.mode else s[2]
    return (x.astype(np.float64) * (target / M)).astype(np.float32)


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_exponent_sources(env, dtype):
    torch, Q, ewops = env
    rng = np.random.default_rng(8)
    n = 2 * WG + 77
    base = rng.normal(size=n).astype(np.float32)
    for kw, target in ((dict(mode=0, bias_pad=2), 1.5 * 2.0 ** -3), (dict(mode=1, bias_pad=0, stdv_mul=4.0), 1.5 * 2.0 ** 4), (dict(mode=0, bias_pad=-1), 1.5 * 2.0 ** 11)):
        spec = Q.QuantizeSpec(4, 3, 8, **kw)
        x = _with_M(base, spec, target)
        x = QR.to_bf16(x) if dtype == "bf16" else (x.astype(np.float16).astype(np.float32) if dtype == "f16" else x)
        want, M = QR.emax_loop(x, 4, spec.bias_pad, spec.mode, spec.stdv_mul, 8)
        assert QR.clear_of_a_power_of_two(M) and want == Q.quantize_emax_test(x, spec, 8) and want != 8
        xd = dev(torch, x, "f32").half() if dtype == "f16" else dev(torch, x, dtype)
        em = Q.emax_tensor(8)
        if dtype == "f16":                                    # the statistics take fp16; quantize does not
            Q.quantize_update_emax(xd, spec, em)
            assert int(em.item()) == want
            continue
        before = Q.quantize_fwd(xd, spec, em)
        Q.quantize_update_emax(xd, spec, em)                  # ... and no sync: the next launch reads what this one wrote
        after = Q.quantize_fwd(xd, spec, em)
        assert int(em.item()) == want
        assert QR.same_bits(P.to_host(before), Q.quantize_test(x, spec, 8)) and QR.same_bits(P.to_host(after), Q.quantize_test(x, spec, want))
        assert QR.same_bits(P.to_host(Q.quantize_fwd(xd, spec, want)), P.to_host(after))          # host emax == device emax
        assert not QR.same_bits(P.to_host(before), P.to_host(after))
    # nothing to go by: the exponent stays
    em = Q.emax_tensor(-3)
    for x in (np.zeros(100, dtype=np.float32), np.full(100, np.nan, dtype=np.float32)):
        Q.quantize_update_emax(dev(torch, x, "f32"), Q.QuantizeSpec(), em)
        assert int(em.item()) == -3


@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_statistics(env, dtype):
    torch, Q, ewops = env
    rng = np.random.default_rng(9)
    for n in (1, WG + 1, 70001):
        x = (rng.normal(size=n) * np.exp(rng.uniform(-12.0, 4.0, n))).astype(np.float32)
        if n > 100:
            x[3], x[50], x[51], x[n - 1], x[n - 2] = np.inf, np.nan, 0.0, -np.inf, -0.0
        x = QR.to_bf16(x) if dtype == "bf16" else (x.astype(np.float16).astype(np.float32) if dtype == "f16" else x)
        xd = dev(torch, x, "f32").half() if dtype == "f16" else dev(torch, x, dtype)
        for sat, ftz in ((65504.0, 2.0 ** -24), (0.5, 1e-3)):
            got = Q.tensor_stats(xd, sat, ftz).cpu().numpy().astype(np.float64)
            want = Q.tensor_stats_test(x, sat, ftz)
            assert got[2] == want[2] and got[5] == want[5] and got[6] == n and got[7] == 0, (n, got, want)
            assert got[3] == np.float32(want[3]) and got[4] == np.float32(want[4]), (n, got, want)          # exact counts, one division
            for i in (0, 1):
                assert abs(got[i] - want[i]) <= P.L2_BAR["f32"] * abs(want[i]), (n, i, got[i], want[i])
        again = Q.tensor_stats(xd, sat, ftz)
        assert np.array_equal(again.cpu().numpy().view(np.uint32), got.astype(np.float32).view(np.uint32))          # the same bits


def test_stochastic_stream(env):
    torch, Q, ewops = env
    n = 1 << 16
    x = np.full(n, 1.0 + 3.0 / 64.0, dtype=np.float32)
    xd = dev(torch, x, "f32")
    spec = Q.QuantizeSpec(4, 3, 8, stochastic=2)
    st = ewops.set_entropy(SEED, offset=40)
    a, b = Q.quantize_fwd(xd, spec), Q.quantize_fwd(xd, spec)
    assert st.tolist() == [SEED, 42] and not torch.equal(a, b)
    assert QR.same_bits(P.to_host(a), Q.quantize_test(x, spec, seed=SEED, offset=40)) and QR.same_bits(P.to_host(b), Q.quantize_test(x, spec, seed=SEED, offset=41))
    share = float((a == 1.125).float().mean())
    assert abs(share - 0.375) <= 5 * np.sqrt(0.375 * 0.625 / n), share
    ewops.set_entropy(SEED, offset=40)
    assert torch.equal(Q.quantize_fwd(xd, spec), a)
    ewops.set_entropy(SEED + 1, offset=40)
    assert not torch.equal(Q.quantize_fwd(xd, spec), a)
    ewops.set_entropy(SEED, offset=40)                        # the storage type does not move the stream
    assert torch.equal(Q.quantize_fwd(dev(torch, x, "bf16"), spec).float(), a)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_group_mode(env, dtype):
    torch, Q, ewops = env
    rng = np.random.default_rng(4)
    runs = 70
    x = (rng.normal(size=GROUP * runs) * np.repeat(np.exp(rng.uniform(-12, 12, runs)), GROUP)).astype(np.float32)
    x[32:64] = 0.0
    x[64:96] = [np.inf, -np.inf, np.nan] + [0.0] * 29
    x[100], x[130] = np.inf, np.nan
    x[160:192] = 1e-40
    x = QR.to_bf16(x) if dtype == "bf16" else x
    xd = dev(torch, x, dtype)
    for kw in (dict(bias_pad=0), dict(bias_pad=2, nearest_even=True), dict(bias_pad=-1, stochastic=1, denorm=False)):
        spec = Q.QuantizeSpec(4, 3, 5, group=GROUP, **kw)
        ewops.set_entropy(SEED, offset=3)
        got = P.to_host(Q.quantize_fwd(xd, spec))
        assert QR.same_bits(got, Q.quantize_test(x, spec, seed=SEED, offset=3)), (dtype, kw)
        em = Q.emax_tensor(-2)                                # the runs without a finite non-zero element follow the device exponent
        ewops.set_entropy(SEED, offset=3)
        got = P.to_host(Q.quantize_fwd(xd, spec, em))
        assert QR.same_bits(got, Q.quantize_test(x, spec, emax=-2, seed=SEED, offset=3)), (dtype, kw, "device emax")
    with pytest.raises(ValueError):
        Q.quantize_fwd(xd[:33], Q.QuantizeSpec(group=GROUP))


def test_autograd_and_log_stats(env, tmp_path):
    torch, Q, ewops = env
    rng = np.random.default_rng(12)
    n = 4000
    x = _with_M(rng.normal(size=n).astype(np.float32), Q.QuantizeSpec(), 1.5 * 2.0 ** 2)
    dy = _with_M(rng.normal(size=n).astype(np.float32), Q.QuantizeSpec(), 1.5 * 2.0 ** -9)
    qspec, b_qspec = Q.QuantizeSpec(4, 3, frequency=1), Q.QuantizeSpec(5, 2, frequency=1, bias_pad=1, nearest_even=True)
    state = Q.QuantizeState(qspec, b_qspec)
    assert int(state.emax_f.item()) == 7 and int(state.emax_b.item()) == 15
    xd = dev(torch, x, "f32").requires_grad_()
    y = Q.quantize(xd, qspec, b_qspec, state=state)
    y.backward(dev(torch, dy, "f32"))
    ef, eb = Q.quantize_emax_test(x, qspec, 7), Q.quantize_emax_test(dy, b_qspec, 15)
    assert (ef, eb) == (4, -8) and int(state.emax_f.item()) == ef and int(state.emax_b.item()) == eb          # each direction its own exponent
    assert QR.same_bits(P.to_host(y), Q.quantize_test(x, qspec, ef)) and QR.same_bits(P.to_host(xd.grad), Q.quantize_test(dy, b_qspec, eb))
    # frequency = 0: the exponent is left alone; the registry finds the state by name
    Q.reset_quantize_states()
    fixed = Q.QuantizeSpec(4, 3, frequency=0)
    y = Q.quantize(xd.detach(), fixed, name="site")
    assert QR.same_bits(P.to_host(y), Q.quantize_test(x, fixed)) and list(Q._states) == [(torch.cuda.current_device(), "site")]
    Q.quantize(xd.detach(), fixed, name="site")
    assert Q._states[(torch.cuda.current_device(), "site")].sched_f.count == 3
    # the schedule of frequency = 8 as the calls see it
    sched = Q.QuantizeSpec(4, 3, emax=-20, frequency=8)
    st8 = Q.QuantizeState(sched)
    collected = []
    for call in range(1, 13):
        st8.emax_f.fill_(-20)
        Q.quantize(xd.detach(), sched, state=st8)
        if int(st8.emax_f.item()) != -20:
            collected.append(call)
    assert collected == Q.quantize_schedule_test(8, 12) == [1, 2, 3, 4, 5, 6, 8, 10, 12]
    # a logfile: the reference's columns
    log = str(tmp_path / "quant.txt")
    logged = Q.QuantizeSpec(4, 3, frequency=1, logfile=log)
    Q.quantize(xd.detach(), logged, name="logged")
    lines = open(log).read().splitlines()
    assert lines[0].split("\t") == Q.quant_headers and len(lines) == 2
    cols = lines[1].split("\t")
    assert len(cols) == 12 and cols[-1] == "logged" and int(cols[-2]) == 1 and int(cols[2]) == ef and int(cols[4]) == 2 and int(cols[3]) == ef - 15 + 1 - 3
    # log_stats: values and gradients pass through, statistics on the logging steps
    Q.reset_quantize_states()
    slog = str(tmp_path / "stats.txt")
    xb = QR.to_bf16(x)
    xr = dev(torch, xb, "bf16").requires_grad_()
    for step in (1, 2, 3, 4, 8, 9):
        z = Q.log_stats(xr, step, freq=8, bfreq=8, logfile=slog, name="act")
        assert torch.equal(z.detach(), xr.detach())
    g = torch.ones_like(z)
    z.backward(g)
    assert torch.equal(xr.grad, g)
    lines = open(slog).read().splitlines()
    assert lines[0].split("\t") == Q.stat_headers and [int(l.split("\t")[-2]) for l in lines[1:]] == [1, 2, 4, 8]          # (the backward of step 9 does not log)
    got = Q.last_logged_stats("act").cpu().numpy()
    want = Q.tensor_stats_test(xb)
    assert got[2] == want[2] and abs(got[0] - want[0]) <= P.L2_BAR["f32"] * want[0]
    Q.reset_quantize_states()


def test_captured_step_follows_the_input_and_draws_fresh_bits(env):
    torch, Q, ewops = env
    rng = np.random.default_rng(13)
    n, o = WG + 40, 200
    spec = Q.QuantizeSpec(4, 3, 8, stochastic=2, bias_pad=1)
    base = rng.normal(size=n).astype(np.float32)
    fills = [_with_M(base, spec, 1.5 * 2.0 ** k) for k in (3, -6)]
    xd = dev(torch, fills[0], "f32")
    em = Q.emax_tensor(8)
    stats = torch.empty(8, dtype=torch.float32, device="cuda")

    def step():
        Q.quantize_update_emax(xd, spec, em, stats_out=stats)
        return Q.quantize_fwd(xd, spec, em)

    st = ewops.set_entropy(SEED, offset=o)
    step()
    torch.cuda.synchronize()
    ewops.set_entropy(SEED, offset=o)
    em.fill_(8)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = step()
    torch.cuda.synchronize()
    assert st.tolist() == [SEED, o] and int(em.item()) == 8               # capturing ran nothing
    seen = []
    for i in range(2):
        xd.copy_(torch.from_numpy(fills[i]))
        graph.replay()
        torch.cuda.synchronize()
        seen.append((P.to_host(y), int(em.item())))
    assert st.tolist() == [SEED, o + 2]
    for i, k in enumerate((3, -6)):
        want_e = Q.quantize_emax_test(fills[i], spec, 8 if i == 0 else seen[0][1])
        assert seen[i][1] == want_e == k + 1, (i, seen[i][1], want_e)
        assert QR.same_bits(seen[i][0], Q.quantize_test(fills[i], spec, want_e, seed=SEED, offset=o + i)), i
    again = Q.quantize_test(fills[1], spec, seen[1][1], seed=SEED, offset=o)
    assert not QR.same_bits(seen[1][0], again)                            # the second replay did not reuse the first one's bits


CASTS = [("float8_e4m3fn", (4, 3, 8), 440.0), ("float8_e5m2", (5, 2, 16), 57344.0)]


@pytest.mark.parametrize("cast", CASTS, ids=[c[0] for c in CASTS])
def test_ties_to_even_equals_the_torch_device_casts(env, cast):
    torch, Q, ewops = env
    name, (ebits, fbits, emax), below = cast
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16)
    h = h[np.isfinite(h)].astype(np.float32)
    lim = np.nextafter(np.float32(below), np.float32(0))
    rng = np.random.default_rng(14)
    r = (rng.normal(size=100000) * np.exp(rng.uniform(-30.0, 12.0, 100000))).astype(np.float32)
    x = np.clip(np.concatenate([h, r]), -lim, lim)
    assert (np.abs(x) < below).all() and x.size == 63488 + 100000
    xd = dev(torch, x, "f32")
    got = Q.quantize_fwd(xd, Q.QuantizeSpec(ebits, fbits, emax, nearest_even=True))
    want = xd.to(getattr(torch, name)).float()
    diff = (got.view(torch.int32) != want.view(torch.int32))
    assert not bool(diff.any()), (int(diff.sum()), xd[diff][:8].tolist(), got[diff][:8].tolist(), want[diff][:8].tolist())
