"""GPU tier of the fused LSTM gates (include/bsmm_lstm.h through blocksparse_amd/lstm.py) against the float64 helper tests/_lstm_ref.py on
inputs pre-rounded to the storage type.  The criterion is the ``check`` of tests/test_ewops_gpu.py: every output finite and, against the
float64 result rounded once to the storage type, inside the L2 and max bars of its dtype (tests/_parity.py).  Each shape is the smallest that
reaches a distinct code path (see PATHS)."""
import itertools

import numpy as np
import pytest

import _lstm_ref as LR
import _parity as P
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu

DTYPES = ("f32", "f16", "bf16")
FORMS = ("fused", "fused-bias", "four")
FB = 1.0
# (K, N, axis): what the case is there for.  A unit is 8 consecutive elements of a row on the 16-byte path (4 in fp32), one element otherwise;
# a workgroup takes 256 units and the grid has at most 2048 workgroups, so one pass of the grid is 524288 units.
PATHS = [
    (1, 1, 0), (1, 1, 1),                                # smallest
    (32, 32, 0), (32, 32, 1),                            # the reference test's size
    (5, 31, 1),                                          # element path; the slices of the fused tensor start at any element
    (31, 5, 0),                                          # the element path on axis 0
    (40, 96, 1), (96, 40, 0),                            # 16-byte path
    (36, 1043, 1),                                       # rows 16-byte aligned but the slices are not (16-bit): the element path, several workgroups
    (8, 3001, 1),                                        # many rows, few features
    (2056, 3, 1),                                        # wide rows
    (3, 8193, 0), (3, 8200, 0),                          # long rows on both paths
    (3, 174763, 0),                                      # 524289 elements on the element path: one unit more than one pass of the grid
    (520, 8066, 1),                                      # 4194320 elements = 524290 units of 8 on the 16-byte path: two units more than one pass
]                                                        #   (fp32: 1048580 units of 4, two passes and a rest)
IDS = ["K%d-N%d-a%d" % c for c in PATHS]
SMALL = [(5, 31, 1), (31, 5, 0), (40, 96, 1), (96, 40, 0), (36, 1043, 1), (3, 8200, 0)]
SMALL_IDS = ["K%d-N%d-a%d" % c for c in SMALL]
NAMES = ("c_next", "h_next", "dc", "di", "du", "df", "do")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from blocksparse_amd import lstm
    return torch, lstm


_cache = {}


def make_case(K, N, axis, dtype, shape=None):
    """Seeded inputs and, lazily, float64 results: computed once per case and shared, never modified."""
    key = (K, N, axis, dtype, shape)
    if key not in _cache:
        C, H, EH, EC, B = LR.make_inputs(K, N, axis, dtype, 1000 * K + 10 * N + axis, shape)
        _cache[key] = dict(C=C, H=H, EH=EH, EC=EC, B=B, ax=0 if axis == 0 else -1, ref={})
    return _cache[key]


def reference(c, bias, grads="both"):
    """The seven float64 outputs (c_next, h_next, dc, di, du, df, do) and db."""
    key = (bool(bias), grads)
    if key not in c["ref"]:
        b = c["B"] if bias else None
        gates = LR.split(c["H"], c["ax"])
        cn, hn = LR.forward(c["C"], gates, b, FB, c["ax"])
        dc, d, db = LR.backward(c["C"], gates, c["EH"] if grads in ("both", "eh") else None, c["EC"] if grads in ("both", "ec") else None, b, FB, c["ax"])
        c["ref"][key] = ((cn, hn, dc) + tuple(d), db)
    return c["ref"][key]


def at_offset(torch, t, off_bytes=0):
    """A contiguous copy of ``t`` whose first element lies ``off_bytes`` past a 16-byte boundary."""
    e = off_bytes // t.element_size()
    buf = torch.empty(t.numel() + e + 16, dtype=t.dtype, device=t.device)
    lead = (-buf.data_ptr() % 16) // t.element_size() + e
    v = buf[lead:lead + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == off_bytes
    return v


def f32dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to("cuda")


def check(name, got, want64, dtype, ctx, max_bar=True):
    want = orc.round_to(np.asarray(want64), dtype) if dtype != "f32" else np.asarray(want64)
    got = P.to_host(got)
    assert got.shape == want.shape, (ctx, name, got.shape, want.shape)
    assert np.isfinite(got).all(), (ctx, name)
    l2, mx = P.errors(got, want)
    print(ctx, name, "l2 %.3g max %.3g" % (l2, mx))
    assert l2 <= P.L2_BAR[dtype] and (mx <= P.MAX_BAR[dtype] or not max_bar), (ctx, name, l2, mx)


def bits_equal(torch, a, b):
    """Bit for bit (a -0 is not a +0)."""
    iv = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))


def split_dev(torch, h, ax):
    """Contiguous copies of the four slices of a fused device tensor."""
    return tuple(p.contiguous() for p in torch.chunk(h, 4, dim=ax))


def run(torch, lstm, c, h, eh, ec, b, ax, form):
    """Forward and backward through the low-level pair in one of the three forms -> the seven outputs, the d-gates as four views."""
    gates = split_dev(torch, h, ax) if form == "four" else (h,)
    bias = b if form == "fused-bias" else None
    cn, hn = lstm.fused_lstm_gates_fwd(c, *gates, bias=bias, forget_bias=FB, axis=ax)
    dc, dg = lstm.fused_lstm_gates_bwd(c, *gates, eh=eh, ec=ec, bias=bias, forget_bias=FB, axis=ax)
    if form == "four":
        assert isinstance(dg, tuple) and len(dg) == 4 and all(g.shape == c.shape and g.dtype == c.dtype for g in dg)
    else:
        assert dg.shape == h.shape and dg.dtype == h.dtype and dg.is_contiguous()       # ONE tensor, the slices written in place
        dg = torch.chunk(dg, 4, dim=ax)
    for t in (cn, hn, dc):
        assert t.shape == c.shape and t.dtype == c.dtype
    return (cn, hn, dc) + tuple(dg)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", PATHS, ids=IDS)
def test_gates_against_float64(env, case, dtype, form):
    torch, lstm = env
    K, N, axis = case
    c = make_case(K, N, axis, dtype)
    want, _ = reference(c, form == "fused-bias")
    dev = [P.to_dev(c[n], dtype, torch) for n in ("C", "H", "EH", "EC")]
    got = run(torch, lstm, *dev, f32dev(torch, c["B"]), c["ax"], form)
    for name, g, w in zip(NAMES, got, want):
        check(name, g, w, dtype, (case, dtype, form))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_absent_gradients_equal_explicit_zeros_bit_for_bit(env, case, dtype):
    """The statement is the bit equality.  Against float64 the one-sided gradients are held to the L2 bar only: with one term of dC missing
    they are heavy-tailed (largest element up to ~19 x the mean magnitude), and the max bar presumes that one 16-bit step on the largest
    element stays below 6 % of the mean -- one value on a rounding boundary would then decide the figure whichever way it is rounded."""
    torch, lstm = env
    K, N, axis = case
    c = make_case(K, N, axis, dtype)
    x, h, eh, ec = (P.to_dev(c[n], dtype, torch) for n in ("C", "H", "EH", "EC"))
    b, ax = f32dev(torch, c["B"]), c["ax"]
    zero = torch.zeros_like(x)
    for form in FORMS:
        for grads, kw_none, kw_zero in (("eh", dict(eh=eh, ec=None), dict(eh=eh, ec=zero)), ("ec", dict(eh=None, ec=ec), dict(eh=zero, ec=ec))):
            a = run(torch, lstm, x, h, kw_none["eh"], kw_none["ec"], b, ax, form)
            z = run(torch, lstm, x, h, kw_zero["eh"], kw_zero["ec"], b, ax, form)
            for name, s, t in zip(NAMES, a, z):
                assert bits_equal(torch, s, t), (case, dtype, form, grads, name)
            want, _ = reference(c, form == "fused-bias", grads)
            for name, g, w in zip(NAMES, a, want):
                check(name, g, w, dtype, (case, dtype, form, grads), max_bar=name in ("c_next", "h_next"))
    with pytest.raises(ValueError):
        lstm.fused_lstm_gates_bwd(x, h, eh=None, ec=None, axis=ax)


@pytest.mark.parametrize("with_bias", (False, True), ids=("no-bias", "bias"))
@pytest.mark.parametrize("dtype", DTYPES)
def test_one_cell_function_on_every_path(env, dtype, with_bias):
    """The same values through the 16-byte path on axis 1 (fused: K = 40 keeps every slice 16-byte aligned), the four-tensor form, axis 0 on
    the transposed data (N = 24) and the element path (every input 2 bytes off an aligned address, 4 in fp32): the same bits in all seven
    outputs.  The four-tensor form takes no bias and sits out the run with one."""
    torch, lstm = env
    K, N = 40, 24
    c = make_case(K, N, 1, dtype)
    x, h, eh, ec = (P.to_dev(c[n], dtype, torch) for n in ("C", "H", "EH", "EC"))
    b = f32dev(torch, c["B"])
    form = "fused-bias" if with_bias else "fused"
    base = run(torch, lstm, x, h, eh, ec, b, -1, form)
    for name, g, w in zip(NAMES, base, reference(c, with_bias)[0]):
        check(name, g, w, dtype, (dtype, form))
    others = {}
    if not with_bias:
        others["four"] = run(torch, lstm, x, h, eh, ec, b, -1, "four")
    tr = lambda t: t.t().contiguous()
    h0 = torch.cat([tr(p) for p in torch.chunk(h, 4, dim=-1)], dim=0)                    # (4K, N): four (K, N) chunks
    others["axis0"] = tuple(tr(t) for t in run(torch, lstm, tr(x), h0, tr(eh), tr(ec), b, 0, form))
    off = 4 if dtype == "f32" else 2
    others["element"] = run(torch, lstm, *(at_offset(torch, t, off) for t in (x, h, eh, ec)), b, -1, form)
    for path, outs in others.items():
        for name, s, t in zip(NAMES, base, outs):
            assert bits_equal(torch, s.contiguous(), t.contiguous()), (dtype, form, path, name)


@pytest.mark.parametrize("dtype", DTYPES)
def test_saturation(env, dtype):
    """c and the four gates from {0, +-1, +-20, +-88, +-1e4} (fp16: +-65504 in place of +-1e4), every combination (9^5 = 59049 cells, as
    243 x 243 in the four-tensor form), eh = ec = 1: finite outputs inside the bars."""
    torch, lstm = env
    big = 65504.0 if dtype == "f16" else 1e4
    vals = orc.round_to(np.array([0.0, 1.0, -1.0, 20.0, -20.0, 88.0, -88.0, big, -big], dtype=np.float32), dtype)
    grid = np.array(list(itertools.product(vals, repeat=5)), dtype=np.float32)
    C, parts = grid[:, 0].reshape(243, 243), [grid[:, q].reshape(243, 243) for q in range(1, 5)]
    E = np.ones_like(C)
    cn, hn = LR.forward(C, parts, None, FB)
    dc, d, _ = LR.backward(C, parts, E, E, None, FB)
    for a in (cn, hn, dc) + d:
        assert np.isfinite(a).all() and np.isfinite(orc.round_to(a, dtype) if dtype != "f32" else a).all()
    x, e = P.to_dev(C, dtype, torch), P.to_dev(E, dtype, torch)
    gates = [P.to_dev(p, dtype, torch) for p in parts]
    for ax in (-1, 0):                                                      # (element-wise: the same cells in either layout)
        gcn, ghn = lstm.fused_lstm_gates_fwd(x, *gates, forget_bias=FB, axis=ax)
        gdc, gd = lstm.fused_lstm_gates_bwd(x, *gates, eh=e, ec=e, forget_bias=FB, axis=ax)
        for name, g, w in zip(NAMES, (gcn, ghn, gdc) + tuple(gd), (cn, hn, dc) + d):
            assert torch.isfinite(g.float()).all(), (dtype, ax, name)
            check(name, g, w, dtype, (dtype, ax))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", SMALL, ids=SMALL_IDS)
def test_twice_gives_the_same_bits(env, case, dtype):
    torch, lstm = env
    K, N, axis = case
    c = make_case(K, N, axis, dtype)
    dev = [P.to_dev(c[n], dtype, torch) for n in ("C", "H", "EH", "EC")]
    b = f32dev(torch, c["B"])
    for form in FORMS:
        first = run(torch, lstm, *dev, b, c["ax"], form)
        torch.empty(1 << 20, device="cuda").fill_(float("nan"))             # (other blocks, with other contents, for the second run)
        second = run(torch, lstm, *dev, b, c["ax"], form)
        for name, s, t in zip(NAMES, first, second):
            assert bits_equal(torch, s, t), (case, dtype, form, name)


@pytest.mark.parametrize("loss_on", ("h", "c", "both"))
@pytest.mark.parametrize("axis", (0, -1))
def test_autograd_gives_the_low_level_gradients(env, axis, loss_on):
    """Rank-3 inputs -- (24, 3, 8) cells first, (3, 5, 40) cells last -- in bf16: backward() through fused_lstm_gates with a loss on h_next
    only, on c_next only and on both, in the fused form with a bias and in the four-tensor form."""
    torch, lstm = env
    from blocksparse_amd import ewops, fused_lstm_gates
    shape = (24, 3, 8) if axis == 0 else (3, 5, 40)
    K = shape[axis]
    c = make_case(K, int(np.prod(shape)) // K, axis, "bf16", shape=shape)
    x, h, eh, ec = (P.to_dev(c[n], "bf16", torch) for n in ("C", "H", "EH", "EC"))
    b = f32dev(torch, c["B"]).view(4, K)                                     # (the gradient comes back in the shape of the bias)
    eh = eh if loss_on in ("h", "both") else None
    ec = ec if loss_on in ("c", "both") else None
    outs_of = lambda cn, hn: [t for t, e in ((cn, ec), (hn, eh)) if e is not None]
    grads_of = [e for e in (ec, eh) if e is not None]
    # fused, with a bias
    xr, hr, br = x.clone().requires_grad_(True), h.clone().requires_grad_(True), b.clone().requires_grad_(True)
    cn, hn = fused_lstm_gates(xr, hr, bias=br, forget_bias=FB, axis=axis)
    torch.autograd.backward(outs_of(cn, hn), grads_of)
    wcn, whn = lstm.fused_lstm_gates_fwd(x, h, bias=b, forget_bias=FB, axis=axis)
    wdc, wdh = lstm.fused_lstm_gates_bwd(x, h, eh=eh, ec=ec, bias=b, forget_bias=FB, axis=axis)
    wdb = ewops.bias_relu_bwd(wdh, None, b, axis=axis)[1]
    assert bits_equal(torch, cn.detach(), wcn) and bits_equal(torch, hn.detach(), whn)
    assert hr.grad.shape == h.shape and hr.grad.dtype == torch.bfloat16                 # ONE (N.., 4K) / (4K, ..N) tensor
    assert br.grad.shape == b.shape and br.grad.dtype == torch.float32
    assert bits_equal(torch, xr.grad, wdc) and bits_equal(torch, hr.grad, wdh) and bits_equal(torch, br.grad, wdb)
    want, _ = reference(c, True, {"h": "eh", "c": "ec", "both": "both"}[loss_on])
    for name, g, w in zip(NAMES, (wcn, whn, wdc) + tuple(torch.chunk(wdh, 4, dim=axis)), want):
        check(name, g, w, "bf16", (axis, loss_on), max_bar=loss_on == "both" or name in ("c_next", "h_next"))      # (one-sided: see above)
    # db is the fp32 sum of the STORED gate gradients (blocksparse/lstm.py:65)
    other = tuple(d for d in range(len(shape)) if d != (axis % len(shape)))
    check("db", wdb.reshape(-1), P.to_host(wdh).astype(np.float64).sum(axis=other), "f32", (axis, loss_on))
    # four tensors
    parts = split_dev(torch, h, axis)
    xr = x.clone().requires_grad_(True)
    pr = [p.clone().requires_grad_(True) for p in parts]
    cn, hn = fused_lstm_gates(xr, *pr, forget_bias=FB, axis=axis)
    torch.autograd.backward(outs_of(cn, hn), grads_of)
    wdc, wd = lstm.fused_lstm_gates_bwd(x, *parts, eh=eh, ec=ec, forget_bias=FB, axis=axis)
    assert bits_equal(torch, xr.grad, wdc)
    for p, w in zip(pr, wd):
        assert bits_equal(torch, p.grad, w)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("axis", (0, 1))
def test_two_chained_time_steps(env, axis, dtype):
    """A recurrence without a matmul: the h_next of step 1, four times over, is added to the gates of step 2, and its c_next is step 2's c.
    The float64 chain rounds where the device stores (c_1, h_1, the new gates), so both see the same step-2 inputs up to a last-place flip
    of step 1."""
    torch, lstm = env
    K, N = 40, 96
    c = make_case(K, N, axis, dtype)
    ax = c["ax"]
    rnd = lambda a: orc.round_to(np.asarray(a).astype(np.float32), dtype).astype(np.float64) if dtype != "f32" else np.asarray(a, dtype=np.float32).astype(np.float64)
    c1, h1 = (rnd(a) for a in LR.forward(c["C"], LR.split(c["H"], ax), c["B"], FB, ax))
    H2 = rnd(c["H"].astype(np.float64) + LR.fuse([h1] * 4, ax))
    c2, h2 = LR.forward(c1, LR.split(H2, ax), c["B"], FB, ax)
    x, h, b = P.to_dev(c["C"], dtype, torch), P.to_dev(c["H"], dtype, torch), f32dev(torch, c["B"])
    g1c, g1h = lstm.fused_lstm_gates_fwd(x, h, bias=b, forget_bias=FB, axis=ax)
    g2c, g2h = lstm.fused_lstm_gates_fwd(g1c, h + torch.cat([g1h] * 4, dim=ax), bias=b, forget_bias=FB, axis=ax)
    check("c_1", g1c, c1, dtype, (axis, dtype))
    check("h_1", g1h, h1, dtype, (axis, dtype))
    check("c_2", g2c, c2, dtype, (axis, dtype))
    check("h_2", g2h, h2, dtype, (axis, dtype))


@pytest.mark.parametrize("axis", (0, 1))
def test_captured_step_follows_its_inputs(env, axis):
    """Forward + backward + bias gradient captured on one stream; the inputs are then overwritten in place and the replay must give the
    float64 result of the NEW inputs."""
    torch, lstm = env
    from blocksparse_amd import ewops
    K, N = 40, 96
    old = make_case(K, N, axis, "bf16")
    ax = old["ax"]
    fresh = dict(zip(("C", "H", "EH", "EC", "B"), LR.make_inputs(K, N, axis, "bf16", 77 + axis)))
    assert not np.array_equal(fresh["C"], old["C"])
    x, h, eh, ec = (P.to_dev(old[n], "bf16", torch) for n in ("C", "H", "EH", "EC"))
    b = f32dev(torch, old["B"])

    def step():
        cn, hn = lstm.fused_lstm_gates_fwd(x, h, bias=b, forget_bias=FB, axis=ax)
        dc, dh = lstm.fused_lstm_gates_bwd(x, h, eh=eh, ec=ec, bias=b, forget_bias=FB, axis=ax)
        return cn, hn, dc, dh, ewops.bias_relu_bwd(dh, None, b, axis=ax)[1]

    step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = step()
    torch.cuda.synchronize()
    for t, n in ((x, "C"), (h, "H"), (eh, "EH"), (ec, "EC")):
        t.copy_(P.to_dev(fresh[n], "bf16", torch))
    b.copy_(f32dev(torch, fresh["B"]))
    graph.replay()
    torch.cuda.synchronize()
    gates = LR.split(fresh["H"], ax)
    cn, hn = LR.forward(fresh["C"], gates, fresh["B"], FB, ax)
    dc, d, _ = LR.backward(fresh["C"], gates, fresh["EH"], fresh["EC"], fresh["B"], FB, ax)
    for name, g, w in zip(NAMES, tuple(outs[:3]) + tuple(torch.chunk(outs[3], 4, dim=ax)), (cn, hn, dc) + d):
        check(name, g, w, "bf16", (axis, "replay"))
    assert bits_equal(torch, outs[4], ewops.bias_relu_bwd(outs[3], None, b, axis=ax)[1])


def test_bad_arguments_raise_before_any_launch(env):
    torch, lstm = env
    from blocksparse_amd import fused_lstm_gates
    c = torch.zeros(6, 4, 8, device="cuda")
    h_last, h_first = torch.zeros(6, 4, 32, device="cuda"), torch.zeros(24, 4, 8, device="cuda")
    b32, b24 = torch.zeros(32, device="cuda"), torch.zeros(24, device="cuda")
    for call in (fused_lstm_gates, lstm.fused_lstm_gates_fwd):
        with pytest.raises(ValueError):
            call(c)                                                          # no gates
        with pytest.raises(ValueError):
            call(c, h_last, h_last)                                          # two tensors
        with pytest.raises(ValueError):
            call(c, c, c, c, c, c)                                           # five
        with pytest.raises(ValueError):
            call(c, c, c, c, c, bias=b32)                                    # a bias with four tensors
        with pytest.raises(ValueError):
            call(c, h_first, axis=-1)                                        # the fused tensor of the other layout
        with pytest.raises(ValueError):
            call(c, h_last, axis=0)
        with pytest.raises(ValueError):
            call(c, h_last, axis=1)                                          # a middle axis
        with pytest.raises(ValueError):
            call(c, h_last.half())                                           # dtypes differ
        with pytest.raises(ValueError):
            call(c.double(), h_last.double())
        with pytest.raises(ValueError):
            call(c, c, c, c, c[:3])                                          # one gate of another shape
        with pytest.raises(ValueError):
            call(c, h_last, bias=b24)                                        # 4K = 32
        with pytest.raises(ValueError):
            call(c, h_last, bias=b32.half())
        with pytest.raises(ValueError):
            call(c.transpose(0, 1), h_last.transpose(0, 1))                  # not contiguous
        with pytest.raises(ValueError):
            call(c, torch.zeros(6, 4, 64, device="cuda")[..., ::2])
        with pytest.raises(ValueError):
            call(c, h_last.cpu())                                            # a gate on another device
    with pytest.raises(ValueError):
        lstm.fused_lstm_gates_bwd(c, h_last)                                 # no gradient at all
    with pytest.raises(ValueError):
        lstm.fused_lstm_gates_bwd(c, h_last, eh=c[:3])
    with pytest.raises(ValueError):
        lstm.fused_lstm_gates_bwd(c, h_last, ec=c.half())
    cn, hn = fused_lstm_gates(c, h_first, bias=b24.view(4, 6), axis=0, name="cell")     # the bias in any shape; name accepted
    assert cn.shape == c.shape and hn.shape == c.shape
