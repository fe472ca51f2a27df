"""GPU tier of the tensor-list weight update (include/bsmm_optim_list.h, ``AdamOptimizer.prepare``).

The rule under test is exact: for the same inputs and the same fp32 rates, one ``step.run()`` -- at most five launches over the whole
list -- leaves the bits of the per-tensor sequence ``clip_by_global_norm``, ``adam_step`` per row, ``ema_step`` per row.  So nearly
every comparison here is ``torch.equal``; the float64 bars (tests/test_optimize_gpu.py derives them: L2 2e-6, max 2e-5 for three steps of
this arithmetic) are run as well so that the new path does not rest on the old one alone.

Lists: the smallest at which a list kernel can go wrong.
  mixed  T = 8: 37 blocks each of bsize 8 / 16 / 32 / 64, flat 1 / 63 / 4097, and one flat fp32 row of 1024 * 256 * 4 + 1027 elements
         (past the cap of the sum of squares on the 16-byte path: its slices stride).  Gradient types cycle, every second row starts one
         element into its allocation (both access paths in one launch), one row has no working copy, one an fp16 one, three block-sparse
         rows are gated (the suite's pattern: blocks 0 and 36 off), one gated and one ungated row select ``lr_new``, all rows but one have
         an average, in mixed storage types.
  one    T = 1: bsize 32, every optional present.
  tiny   T = 70: the sizes 1 + (7 i) % 40 of test_global_norm_many_tensors -- the row search at every boundary.
"""
import collections
import functools

import numpy as np
import pytest

import _optimize_ref as OR
import _parity as P
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu

BLOCKS = 37
LR, LR_NEW, DECAY = 1e-3, 5e-3, 0.99
B1, B2 = 0.9, 0.999
SETTINGS = dict(grad_scale=0.5, saturate=2.0, clip_sigma=3.0)
BIG = 1024 * 256 * 4 + 1027
DTS = ("f32", "f16", "bf16")
ITYPE = {4: "int32", 2: "int16"}

# bs (0: flat), size (flat rows), gradient type, misalign, working-copy type, gated, lr_select, type of the average
Row = collections.namedtuple("Row", "bs size gdt mis wdt gated sel edt")
LISTS = {
    "mixed": (Row(8, 0, "f32", 1, "bf16", True, False, "f32"),
              Row(16, 0, "f16", 0, "f16", True, True, "f16"),
              Row(32, 0, "bf16", 1, "bf16", False, True, "bf16"),
              Row(64, 0, "f32", 0, "bf16", True, False, "f32"),
              Row(0, 1, "f16", 1, None, False, False, "bf16"),
              Row(0, 63, "bf16", 0, "bf16", False, False, None),
              Row(0, 4097, "f32", 1, "bf16", False, False, "f32"),
              Row(0, BIG, "f32", 0, "bf16", False, False, "f16")),
    "one": (Row(32, 0, "bf16", 0, "bf16", True, True, "f32"),),
    "tiny": tuple(Row(0, 1 + (7 * i) % 40, DTS[i % 3], i % 2, "bf16", False, False, DTS[(i + 1) % 3]) for i in range(70)),
}
Host = collections.namedtuple("Host", "p m v g gate sel e live")


@pytest.fixture(scope="module")
def env():
    import torch
    from blocksparse_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    _lib.load()
    return torch, _lib


def _inputs(n, gdt, seed):
    """The inputs of tests/test_optimize_gpu.py: outliers in g, zeros in m and v."""
    rng = np.random.RandomState(seed)
    g = rng.normal(0.0, 0.1, n).astype(np.float32)
    g[::97] *= 50.0
    g = orc.round_to(g, gdt).astype(np.float32)
    p = rng.normal(0.0, 0.01, n).astype(np.float32)
    m = rng.normal(0.0, 0.01, n).astype(np.float32)
    v = rng.uniform(0.0, 1e-2, n).astype(np.float32)
    m[::53] = 0.0
    v[::53] = 0.0
    return p, m, v, g


def _size(r):
    return BLOCKS * r.bs * r.bs if r.bs else r.size


@functools.lru_cache(maxsize=None)
def _host(name):
    """Host side of a list, computed once and never written again; and a clip norm that scales its gradients by about 0.7."""
    out = []
    for i, r in enumerate(LISTS[name]):
        n = _size(r)
        p, m, v, g = _inputs(n, r.gdt, 1000 * len(name) + i)
        rng = np.random.RandomState(77 + i)
        gate = OR.gate_pattern(BLOCKS, rng) if r.gated else None
        sel = None
        if r.sel:
            sel = (rng.rand(BLOCKS) < 0.4).astype(np.float32)
            sel[1], sel[2], sel[4] = 1.0, 0.0, 1.0                    # (block 4 is live under the suite's gate)
        e = orc.round_to(p + rng.normal(0.0, 0.003, n).astype(np.float32), r.edt).astype(np.float32) if r.edt else None
        live = np.repeat(gate != 0, r.bs * r.bs) if r.gated else np.ones(n, dtype=bool)
        for a in (p, m, v, g, gate, sel, e, live):
            if a is not None:
                a.setflags(write=False)
        out.append(Host(p, m, v, g, gate, sel, e, live))
    norm, _ = OR.clip([OR.sum_squared(h.g, 0.5, 2.0) for h in out], 1.0)
    return tuple(out), 0.7 * norm


@functools.lru_cache(maxsize=None)
def _new_grads(name, k):
    """Gradient set k of a list (the capture test copies a new one into the static grads before every replay)."""
    out = []
    for i, r in enumerate(LISTS[name]):
        g = _inputs(_size(r), r.gdt, 5000 + 100 * k + i)[3]
        g.setflags(write=False)
        out.append(g)
    return tuple(out)


def _dev(torch, a, dtype="f32", shape=None, misalign=0):
    """A device copy of ``a``; misalign = 1: a view that starts one element into a larger allocation (the element path)."""
    t = torch.from_numpy(np.array(a, dtype=np.float32)).cuda().to(getattr(torch, P.TORCH_DT[dtype]))
    if misalign:
        big = torch.full((t.numel() + 8,), 3.0, dtype=t.dtype, device="cuda")
        big[misalign:misalign + t.numel()].copy_(t)
        t = big[misalign:misalign + t.numel()]
        assert t.data_ptr() % 16 != 0
    return t.view(shape) if shape is not None else t


def _around(torch, t):
    """The elements of ``t``'s allocation outside ``t`` (a misaligned view), as integers; None for a whole allocation."""
    base = t._base
    if base is None or base.numel() == t.numel():
        return None
    raw = base.view(-1).view(getattr(torch, ITYPE[base.element_size()]))
    off = (t.data_ptr() - base.data_ptr()) // base.element_size()
    return torch.cat([raw[:off], raw[off + t.numel():]]).clone()


class State(object):
    """One device copy of a list: params (with ``.gate``), grads, an AdamOptimizer whose slots are placed by the test, an Ema."""

    def __init__(self, torch, name, saturate=SETTINGS["saturate"], **opt_kw):
        from blocksparse_amd import AdamOptimizer, Ema
        self.settings = dict(SETTINGS, saturate=saturate)
        self.rows, (self.host, self.clip) = LISTS[name], _host(name)
        self.params, self.grads, self.sels, self.ema_params = [], [], [], []
        for r, h in zip(self.rows, self.host):
            shape = (BLOCKS, r.bs, r.bs) if r.bs else None
            p = _dev(torch, h.p, shape=shape, misalign=r.mis)
            if r.gated:
                p.gate = torch.from_numpy(np.array(h.gate)).cuda()
            self.params.append(p)
            self.grads.append(_dev(torch, h.g, r.gdt, shape, r.mis))
            self.sels.append(torch.from_numpy(np.array(h.sel)).cuda() if r.sel else None)
        self.opt = AdamOptimizer(self.params, learning_rate=LR, beta1=B1, beta2=B2, clip_sigmas=SETTINGS["clip_sigma"], grad_scale=SETTINGS["grad_scale"],
                                 saturate=saturate, gated=True, working_dtype=torch.bfloat16, **opt_kw)
        self.ema = Ema(DECAY, gated=True)
        for i, (r, h, p) in enumerate(zip(self.rows, self.host, self.params)):
            shape = (BLOCKS, r.bs, r.bs) if r.bs else None
            slot = {"Mean": _dev(torch, h.m, shape=shape, misalign=r.mis), "Var": _dev(torch, h.v, shape=shape, misalign=r.mis)}
            if r.wdt:
                slot["working"] = _dev(torch, np.full(h.p.shape, 7.0), r.wdt, shape, r.mis)
            self.opt.slots[i] = slot
            if r.edt:
                self.ema.averages[id(p)] = (p, _dev(torch, h.e, r.edt, shape, r.mis))
                self.ema_params.append(p)

    def prepare(self, param_grads=False):
        any_sel = any(s is not None for s in self.sels)
        return self.opt.prepare(grads=None if param_grads else self.grads, clip_norm=self.clip, ema=self.ema,
                                lr_select=self.sels if any_sel else None, lr_new=LR_NEW if any_sel else None, ema_params=self.ema_params)

    def tensors(self, which=("param", "Mean", "Var", "working", "ema")):
        """[(name, row, tensor)] of everything a step may write."""
        out = []
        for i, p in enumerate(self.params):
            slot = self.opt.slots[i]
            for k, t in (("param", p), ("Mean", slot["Mean"]), ("Var", slot["Var"]), ("working", slot.get("working")), ("ema", self.ema.average(p))):
                if t is not None and k in which:
                    out.append((k, i, t))
        return out

    def eager(self, lr_t, lr_new_t):
        """The per-tensor sequence with the given corrected rates; returns (norm, scale)."""
        from blocksparse_amd import adam_step, clip_by_global_norm, ema_step
        norm, scale = clip_by_global_norm(self.grads, clip_norm=self.clip, grad_scale=SETTINGS["grad_scale"], saturate=self.settings["saturate"])
        for i, p in enumerate(self.params):
            slot, sel = self.opt.slots[i], self.sels[i]
            adam_step(p, self.grads[i], slot["Mean"], slot["Var"], lr_t, beta1=B1, beta2=B2, gate=getattr(p, "gate", None), lr_select=sel,
                      lr_new=lr_new_t if sel is not None else None, norm_scale=scale, param16=slot.get("working"), **self.settings)
        for p in self.ema_params:
            ema_step(self.ema.average(p), p, DECAY, gate=getattr(p, "gate", None))
        return norm, scale


def _assert_same(torch, a, b, ctx):
    ta, tb = a.tensors(), b.tensors()
    assert [(k, i) for k, i, _ in ta] == [(k, i) for k, i, _ in tb]
    for (k, i, x), (_, _, y) in zip(ta, tb):
        assert torch.equal(x, y), (ctx, k, "row %d" % i, a.rows[i])


def _rates(step):
    lr_t, lr_new_t = step.rates().tolist()
    return lr_t, lr_new_t


# ---------------------------------------------------------------------------------------------------------------- bits and values
@pytest.mark.parametrize("name", ("mixed", "one", "tiny"))
def test_list_step_equals_the_per_tensor_sequence(env, name):
    torch, _ = env
    A, B = State(torch, name), State(torch, name)
    around = [(k, i, _around(torch, t), t) for k, i, t in A.tensors()]
    assert name != "mixed" or sum(1 for _, _, a, _ in around if a is not None) >= 16
    step = A.prepare()
    assert step.learning_rate.dtype == torch.float32 and step.learning_rate.shape == (1,) and float(step.learning_rate) == np.float32(LR)
    versions = [t._version for _, _, t in A.tensors()]
    device_steps = []
    for t in range(1, 4):
        step.run()
        lr_t, lr_new_t = _rates(step)
        norm, scale = B.eager(lr_t, lr_new_t)
        _assert_same(torch, A, B, (name, "step %d" % t))
        assert torch.equal(step.global_norm, norm) and torch.equal(step.norm_scale, scale), (name, t)
        assert 0.0 < float(scale) < 1.0                                  # (the clip does scale: the norm reaches the Adam pass)
        device_steps.append((lr_t, lr_new_t, float(scale)))
        assert A.opt.steps == t
    assert all(t._version > old for (_, _, t), old in zip(A.tensors(), versions))
    assert step.sync_host() == 3
    # the elements around misaligned views, and the gated-off blocks of every tensor, keep their bits
    for k, i, before, t in around:
        if before is not None:
            assert torch.equal(_around(torch, t), before), (name, k, i)
    for k, i, t in A.tensors():
        r, h = A.rows[i], A.host[i]
        if not r.gated:
            continue
        assert (~h.live).sum() >= 2 * r.bs * r.bs
        old = {"param": h.p, "Mean": h.m, "Var": h.v, "working": np.full(h.p.shape, 7.0, dtype=np.float32), "ema": h.e}[k]
        got = P.to_host(t).reshape(-1)
        assert np.array_equal(got[~h.live], old[~h.live]) and not np.array_equal(got[h.live], old[h.live]), (name, k, i)
    # values against float64, from the rates and the scale the device stepped with
    ref = [(h.p, h.m, h.v) for h in A.host]
    for lr_t, lr_new_t, scale in device_steps:
        ref = [OR.adam(p, m, v, h.g, lr_t, gate=h.gate, bsize=r.bs, lr_select=h.sel, lr_new=lr_new_t, norm_scale=scale, beta1=B1, beta2=B2, **SETTINGS)
               for (p, m, v), h, r in zip(ref, A.host, A.rows)]
    for q, key in enumerate(("param", "Mean", "Var")):
        got = [P.to_host(t).reshape(-1) for _, _, t in A.tensors((key,))]
        l2, mx = P.errors(np.concatenate(got), np.concatenate([x[q] for x in ref]))
        print("list %s %s, all rows: L2 %.3e max %.3e" % (name, key, l2, mx))
        assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (name, key, l2, mx)
        for i, (g, x) in enumerate(zip(got, ref)):
            if g.size >= 63:                                            # (a row of a few elements has no mean to speak of: it is in the list-wide figure)
                l2, mx = P.errors(g, x[q])
                assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (name, key, i, l2, mx)
    for k, i, t in A.tensors(("working",)):
        lv = torch.from_numpy(np.array(A.host[i].live)).cuda()
        assert torch.equal(t.reshape(-1)[lv], A.params[i].reshape(-1).to(t.dtype)[lv]), (name, i)


# ---------------------------------------------------------------------------------------------------------------- the rate
def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def test_device_rate_follows_the_host_correction(env):
    """lr_t = fp32(fp64(fp32(base)) * c_t) with c_t in double on both sides: the device's powers may differ from the host's by a few double
    ulps before the single rounding to fp32, so the results differ by at most one fp32 ulp."""
    torch, _ = env
    from blocksparse_amd import optimize
    bases = (1e-3, 3e-3, 5e-4, 7e-4, 2e-3)
    S = State(torch, "one")
    step = S.prepare()
    assert float(step.lr_new) == np.float32(LR_NEW)
    for t, base in enumerate(bases, 1):
        step.learning_rate.fill_(base)
        step.run()
        lr_t, lr_new_t = _rates(step)
        c = optimize.lr_correction(t, B1, B2)
        want, want_new = np.float32(np.float64(np.float32(base)) * c), np.float32(np.float64(np.float32(LR_NEW)) * c)
        print("rate step %d: device %.9e host %.9e" % (t, lr_t, want))
        assert abs(lr_t - float(want)) <= _ulp(want) and abs(lr_new_t - float(want_new)) <= _ulp(want_new), (t, lr_t, want, lr_new_t, want_new)
    assert step.sync_host() == len(bases)
    Z = State(torch, "one", zero_init_variables=True)
    zstep = Z.opt.prepare(grads=Z.grads)                          # no lr_new: lr_new_t is lr_t
    assert zstep.lr_new is None and zstep.global_norm is None and zstep.norm_scale is None
    for base in bases[:3]:
        zstep.learning_rate.fill_(base)
        zstep.run()
        lr_t, lr_new_t = _rates(zstep)
        assert np.float32(lr_t) == np.float32(base) and lr_new_t == lr_t


# ---------------------------------------------------------------------------------------------------------------- the clip's sentinel
def test_an_overflow_skips_every_row(env):
    """An Inf in one row's gradient: the norm is not finite, the scale is 0 and no row is stepped.  Without ``saturate`` here and in the
    capture test: the clamp comes before the square (include/bsmm_optim.h), so with it an Inf is a finite +-saturate and nothing overflows."""
    torch, _ = env
    A, B = State(torch, "mixed", saturate=0.0), State(torch, "mixed", saturate=0.0)
    for S in (A, B):
        S.grads[3].view(-1)[12345] = float("inf")
    step = A.prepare()
    before = [(k, i, t.clone()) for k, i, t in A.tensors()]
    step.run()
    assert float(step.norm_scale) == 0.0 and not np.isfinite(float(step.global_norm))
    B.eager(*_rates(step))
    _assert_same(torch, A, B, "skip")
    for (k, i, t), (_, _, old) in zip(A.tensors(), before):
        if k == "ema":
            assert t.numel() < 63 or not torch.equal(t, old), ("the average still moves", i)      # (a single 16-bit element may round back)
        else:
            assert torch.equal(t, old), (k, i)
    assert A.opt.steps == 1 and step.sync_host() == 1              # the count advances on a skipped step too


# ---------------------------------------------------------------------------------------------------------------- capture
def test_captured_step_follows_the_rate_on_the_device(env):
    """The capability itself: clip + Adam + moving average of the mixed list captured once; three replays, each with new gradients in the
    static buffers and another learning rate on the device, the second with an Inf.  Every replay leaves the bits of the eager per-tensor
    sequence at that replay's rate; replay 3 differs from the same sequence at the rate of replay 1, which is what a rate baked in at
    capture time would give."""
    torch, _ = env
    name = "mixed"
    C, E, F = (State(torch, name, saturate=0.0) for _ in range(3))
    step = C.prepare()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                 # one real step: first-call host work stays out of the capture
        step.run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    warm = _rates(step)
    for S in (E, F):
        S.eager(*warm)
    _assert_same(torch, C, E, "warm-up")
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step.run()
    torch.cuda.synchronize()
    _assert_same(torch, C, E, "capturing ran nothing")
    assert C.opt.steps == 1
    lrs = (1e-3, 3e-3, 5e-4)
    first = None
    for k, base in enumerate(lrs):
        new = [np.array(g) for g in _new_grads(name, k)]
        if k == 1:
            new[1][777] = np.inf
        before = [(key, i, t.clone()) for key, i, t in C.tensors()]
        for S in (C, E, F):
            for g, h in zip(S.grads, new):
                g.copy_(torch.from_numpy(h).cuda().to(g.dtype).view_as(g))
        step.learning_rate.copy_(torch.full((1,), base, device="cuda"))
        graph.replay()
        torch.cuda.synchronize()
        rates = _rates(step)
        first = first or rates
        c = rates[0] / float(np.float32(base))
        assert abs(c - np.sqrt(1 - B2 ** (k + 2)) / (1 - B1 ** (k + 2))) <= 1e-6 * c          # step k + 2 of this state, at this replay's rate
        E.eager(*rates)
        _assert_same(torch, C, E, ("replay", k))
        changed = {(key, i) for (key, i, t), (_, _, old) in zip(C.tensors(), before) if not torch.equal(t, old)}
        if k == 1:
            assert float(step.norm_scale) == 0.0 and {key for key, _ in changed} == {"ema"}, changed
        else:
            assert changed >= {(key, i) for key, i, t in before if key != "ema" or t.numel() >= 63}, (k, len(changed))
        if k < 2:
            F.eager(*rates)
        else:
            F.eager(*first)                                        # the rates of replay 1, as a baked-in capture would replay them
            for (key, i, x), (_, _, y) in zip(C.tensors(("param",)), F.tensors(("param",))):
                assert not torch.equal(x, y), ("replay 3 stepped at the capture-time rate", i)
    assert step.sync_host() == 3 + 1 and C.opt.steps == 4          # three replays and the warm-up step


# ---------------------------------------------------------------------------------------------------------------- moved tensors
def test_a_moved_grad_is_refused_before_any_launch(env):
    torch, _ = env
    S = State(torch, "one")
    p = S.params[0]
    p.grad = _dev(torch, S.host[0].g, shape=tuple(p.shape))     # fp32: a tensor's .grad has the tensor's type
    S.grads = [p.grad]
    step = S.prepare(param_grads=True)
    step.run()
    before = [(k, i, t.clone()) for k, i, t in S.tensors()]
    rates = step.rates().clone()
    p.grad = p.grad.clone()                                       # what zero_grad(set_to_none=True) and a new backward leave: another tensor
    with pytest.raises(ValueError, match=r"zero_grad\(set_to_none=False\)"):
        step.run()
    torch.cuda.synchronize()
    for (k, i, t), (_, _, old) in zip(S.tensors(), before):
        assert torch.equal(t, old), k
    assert torch.equal(step.rates(), rates) and S.opt.steps == 1
    p.grad = S.grads[0]                                           # back in place: the step runs again
    step.run()
    assert S.opt.steps == 2 and step.sync_host() == 2 and not torch.equal(S.params[0], before[0][2])
    with pytest.raises(ValueError, match="no grad"):
        State(torch, "one").opt.prepare()                         # every param of a prepared step needs a gradient


# ---------------------------------------------------------------------------------------------------------------- caches
def _f32_operator(env):
    """bsize 32, feature axis 1, fp32 with the plan forced (the caller sets the kernel variant): the kernel that multiplies with prepared
    bf16 pieces of W, cached per weights version -- the construction of tests/test_optimize_gpu.py."""
    torch, lib = env
    from blocksparse_amd import BlocksparseMatMul
    lay = P.random_layout(40, 40, 0.2, seed=5)
    b = BlocksparseMatMul(lay, block_size=32, feature_axis=1)
    gen = P.gen(torch, 2)
    w = torch.randn(b.w_shape, device="cuda", generator=gen) * 0.05
    x = torch.randn(b.i_shape(256), device="cuda", generator=gen) * 0.1
    dw = torch.randn(b.w_shape, device="cuda", generator=gen) * 0.1
    return lay, b, w, x, dw


def test_fprop_after_a_list_step_uses_the_stepped_weights(env):
    torch, lib = env
    from blocksparse_amd import AdamOptimizer
    lib.set_kernel_variant(3)
    try:
        lay, b, w, x, dw = _f32_operator(env)
        y0 = b.fprop(x, w)
        assert lib.last_kernel() == lib.K_XCOL32_F32SPLIT and lib.OP_FPROP in b._prepared_w and b._prepared_w[lib.OP_FPROP][0]() is w      # else: vacuous
        w_old, version = w.clone(), w._version
        w.grad = dw
        opt = AdamOptimizer([w], learning_rate=1e-2)
        opt.prepare().run()
        assert opt.steps == 1 and float(opt.get_slot(w, "Var").abs().sum()) > 0
        torch.cuda.synchronize()
        assert not torch.equal(w, w_old)
        assert w._version > version, "a write through the C ABI must move the version counter"
        y1 = b.fprop(x, w)
        assert lib.last_kernel() == lib.K_XCOL32_F32SPLIT
        t = orc.build_layout_luts(lay, 32)
        ref = orc.fprop_fast(t, P.to_host(x).astype(np.float64), P.to_host(w).astype(np.float64), 1, np.float64)
        l2, mx = P.errors(P.to_host(y1), ref)
        stale, _ = P.errors(P.to_host(y0), ref)
        print("fprop after the list step: L2 %.3e (the result of the old weights: %.3e)" % (l2, stale))
        assert stale > 1e-3                                    # (the write moved the result far beyond the bar: a stale cache cannot pass)
        assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (l2, mx)
    finally:
        lib.set_kernel_variant(0)
