"""GPU tier of Adafactor (include/bsmm_adafactor.h, blocksparse_amd/optimize.py) against the float64 definitions of tests/_adafactor_ref.py
on the named cases of tests/_adafactor_cases.py.

Steps: three, with decay = adafactor_decay(t, 0.999), lr 1e-3, grad_scale 0.5, saturate 2.0, norm_scale 0.7; grads fp32 / fp16 / bf16.
Shapes: the 2-d shapes the issue names, plus (33, 1028) and (33, 257): the kernels' tiles are 32 rows x 1024 columns on the 16-byte path
and 32 x 256 on the element path, so those are the shapes one past both tile boundaries of either path ((300, 520) is ten slabs but a
single chunk on the 16-byte path; its misaligned twin has three).  1-d sizes 1, 63, 4097, and 4096 aligned and one element off; 37
blocks of every block size with the suite's gate, one fp32 case ungated, one block case one element off.
Bars against float64: param inside the project's fp32 bars (L2 2e-6, max 2e-5), the update p_new - p_old within 1e-5 (L2), rv and cv per
element relative within 2e-5 -- sums of non-negative terms, nothing cancels.  The float32 model of the kernels' order stays below 1.3e-6
(param max), 7e-8 (param L2), 2.5e-7 (update) and 4.2e-7 (moments) on these cases (tests/test_adafactor_host.py); the measured device
figures are in profiles/adafactor_tests.md.  Everything "unchanged" or "equal to another run" is compared bit for bit.

One block as a matrix: the block form walks a 32 x 32 block with rows spread over the lanes of one wave, the 2-d form with rows in a lane's
chain, so their pinned summation orders differ and the two are held to the fp32 bars against each other, not to equal bits."""
import numpy as np
import pytest

import _adafactor_cases as AC
import _parity as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    from blocksparse_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    _lib.load()
    return torch, _lib


def _dev(torch, a, dtype="f32", shape=None, misalign=0):
    """A device copy of ``a``; misalign = 1: a view that starts one element into a larger allocation (the element path)."""
    t = torch.from_numpy(np.array(a, dtype=np.float32)).cuda().to(getattr(torch, P.TORCH_DT[dtype]))
    if misalign:
        big = torch.empty(t.numel() + 8, dtype=t.dtype, device="cuda")
        big[misalign:misalign + t.numel()].copy_(t)
        t = big[misalign:misalign + t.numel()]
        assert t.data_ptr() % 16 != 0
    return t.view(shape) if shape is not None else t


def _state(torch, c, p16dt="bf16"):
    """Device tensors of a case: (p, g, cv, rv, p16, gate)."""
    shape, m = AC.shape_of(c), c.misalign
    slot_shape = (c.rows, c.bs) if c.bs else None
    p = _dev(torch, c.p, "f32", shape, m)
    g = _dev(torch, c.g, c.gdt, shape, m)
    cv = _dev(torch, c.cv, "f32", slot_shape, m)
    rv = _dev(torch, c.rv, "f32", slot_shape, m) if c.rv is not None else None
    p16 = _dev(torch, np.full(c.p.shape, 7.0), p16dt, shape, m)
    gate = torch.from_numpy(np.array(c.gate)).cuda() if c.gate is not None else None
    return p, g, cv, rv, p16, gate


def _steps(torch, c, st, steps=AC.STEPS, ns=AC.NORM_SCALE):
    from blocksparse_amd import adafactor_step
    p, g, cv, rv, p16, gate = st
    scale = torch.full((1,), ns, device="cuda")
    for t in range(1, steps + 1):
        adafactor_step(p, g, cv, rv, lr=AC.LR, decay=AC.decay(t), gate=gate, norm_scale=scale, param16=p16, **AC.SETTINGS)


@pytest.mark.parametrize("name", sorted(AC.CASES))
def test_adafactor_parity(env, name):
    torch, _ = env
    c = AC.case(name)
    st = _state(torch, c, "f16" if c.gdt == "f16" else "bf16")
    p, g, cv, rv, p16, gate = st
    written = [t for t in (p, cv, rv, p16) if t is not None]
    versions = [t._version for t in written]
    _steps(torch, c, st)
    assert all(t._version > old for t, old in zip(written, versions))
    host = lambda t: None if t is None else P.to_host(t).reshape(-1)
    AC.check(c, host(p), host(cv), host(rv), "device")
    live, ls = c.live, c.live_slots
    if c.gate is not None:
        assert (~live).sum() >= 2 * c.cols and live.sum() > 0
        # gated-off blocks keep their bits in every tensor
        for got, old, mask in ((p, c.p, live), (p16, np.full(c.p.shape, 7.0, dtype=np.float32), live), (cv, c.cv, ls), (rv, c.rv, ls)):
            assert np.array_equal(host(got)[~mask], old[~mask]), name
    lv = torch.from_numpy(live).cuda()
    assert torch.equal(p16.reshape(-1)[lv], p.reshape(-1).to(p16.dtype)[lv]), name               # param rounded once
    if c.form == "2d":
        assert np.array_equal(host(p).reshape(c.rows, c.cols)[c.rows // 2], c.p.reshape(c.rows, c.cols)[c.rows // 2])      # a row of zero gradients
        assert np.array_equal(host(p).reshape(c.rows, c.cols)[:, c.cols // 3], c.p.reshape(c.rows, c.cols)[:, c.cols // 3])


def test_clip_coverage_on_the_host_values():
    for names, form_set in ((AC.CLIP_ACTIVE, "above"), (AC.CLIP_INACTIVE + AC.CLIP_INACTIVE_FIRST_STEP, "below")):
        assert sorted(AC.case(n).form for n in names) == ["1d", "2d", "block"], form_set
    for n in AC.CLIP_ACTIVE:
        assert min(AC.case(n).rms) > 1.0, (n, AC.case(n).rms)
    for n in AC.CLIP_INACTIVE:
        assert max(AC.case(n).rms) < 1.0, (n, AC.case(n).rms)
    for n in AC.CLIP_INACTIVE_FIRST_STEP:
        assert AC.case(n).rms[0] < 1.0, (n, AC.case(n).rms)


FORMS = ("2d-300x520-clip", "2d-67x131-element", "1d-4097", "block-8", "block-64")


@pytest.mark.parametrize("name", FORMS)
def test_identical_calls_give_identical_bits(env, name):
    torch, _ = env
    c = AC.case(name)
    a, b = _state(torch, c), _state(torch, c)
    _steps(torch, c, a, steps=2)
    torch.empty(1 << 20, device="cuda").fill_(float("nan"))          # whatever the second run's workspace lands on, it is not the first run's
    _steps(torch, c, b, steps=2)
    for x, y in zip(a[:5], b[:5]):
        assert x is None or torch.equal(x, y), name


@pytest.mark.parametrize("name", FORMS)
def test_norm_scale_zero_stores_nothing(env, name):
    torch, _ = env
    c = AC.case(name)
    st, old = _state(torch, c), _state(torch, c)
    _steps(torch, c, st, steps=1, ns=0.0)
    for x, y in zip(st[:5], old[:5]):
        assert x is None or torch.equal(x, y), name


def test_all_gates_zero_stores_nothing(env):
    torch, _ = env
    c = AC.case("block-16")
    st, old = _state(torch, c), _state(torch, c)
    st = st[:5] + (torch.zeros(c.rows, device="cuda"),)
    _steps(torch, c, st, steps=1)
    for x, y in zip(st[:5], old[:5]):
        assert torch.equal(x, y)


def test_one_ungated_block_against_the_2d_form(env):
    """Orders differ (module docstring): fp32 bars between the two forms, and each inside the bars against float64."""
    import _adafactor_ref as AR
    from blocksparse_amd import adafactor_step
    torch, _ = env
    rng = np.random.RandomState(32)
    g0 = rng.normal(0.0, 0.1, 1024).astype(np.float32)
    g0[::97] *= 50.0
    p0, cv0, rv0 = rng.normal(0.0, 0.01, 1024).astype(np.float32), rng.uniform(0, 1e-2, 32).astype(np.float32), rng.uniform(0, 1e-2, 32).astype(np.float32)
    kw = dict(lr=AC.LR, decay=AC.decay(2), **AC.SETTINGS)
    ref = AR.dense(p0, cv0, rv0, g0, 32, 32, **kw)
    out = {}
    for form, shape, slot in (("block", (1, 32, 32), (1, 32)), ("2d", (32, 32), (32,))):
        p, g, cv, rv = _dev(torch, p0, shape=shape), _dev(torch, g0, shape=shape), _dev(torch, cv0, shape=slot), _dev(torch, rv0, shape=slot)
        adafactor_step(p, g, cv, rv, **kw)
        out[form] = [P.to_host(t).reshape(-1) for t in (p, cv, rv)]
        for got, want, name in zip(out[form], ref[:3], ("p", "cv", "rv")):
            l2, mx = P.errors(got, want)
            print("one block as %s, %s vs float64: L2 %.3e max %.3e" % (form, name, l2, mx))
            assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (form, name, l2, mx)
    for a, b, name in zip(out["block"], out["2d"], ("p", "cv", "rv")):
        l2, mx = P.errors(a, b)
        print("one block, block form vs 2-d form, %s: L2 %.3e max %.3e" % (name, l2, mx))
        assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (name, l2, mx)


# ---------------------------------------------------------------------------------------------------------------- AdafactorOptimizer
def _mixed(torch):
    """(params, grads): a 2-d, a 1-d and a gated block-sparse param with their grads."""
    cs = [AC.case(n) for n in ("2d-67x136-zero-slots", "1d-4097", "block-16")]
    params = [_dev(torch, c.p, shape=AC.shape_of(c)) for c in cs]
    grads = [_dev(torch, c.g, c.gdt, AC.shape_of(c)) for c in cs]
    params[2].gate = torch.from_numpy(np.array(cs[2].gate)).cuda()
    return params, grads


def test_optimizer_equals_the_step_calls_bit_for_bit(env):
    from blocksparse_amd import AdafactorOptimizer, adafactor_step
    torch, _ = env
    params, grads = _mixed(torch)
    ns = torch.full((1,), AC.NORM_SCALE, device="cuda")
    opt = AdafactorOptimizer(params, learning_rate=AC.LR, beta2=AC.BETA2, gated=True, working_dtype=torch.bfloat16, **AC.SETTINGS)
    assert opt.get_slot(params[0], "rv").shape == (67,) and opt.get_slot(params[0], "cv").shape == (136,)
    assert opt.get_slot(params[1], "rv") is None and opt.get_slot(params[1], "cv").shape == (4097,)
    assert opt.get_slot(params[2], "rv").shape == (AC.BLOCKS, 16) and not bool(opt.get_slot(params[2], "cv").any())
    mine, _g = _mixed(torch)
    slots = [{k: torch.zeros_like(opt.get_slot(p, k)) for k in ("cv", "rv") if opt.get_slot(p, k) is not None} for p in params]
    work = [p.to(torch.bfloat16) for p in mine]
    for t in range(1, AC.STEPS + 1):
        opt.step(grads=grads, norm_scale=ns)
        for p, g, s, w in zip(mine, grads, slots, work):
            adafactor_step(p, g, s["cv"], s.get("rv"), lr=AC.LR, decay=AC.decay(t), gate=getattr(p, "gate", None), norm_scale=ns, param16=w,
                           **AC.SETTINGS)
    for p, q, s, w in zip(params, mine, slots, work):
        assert torch.equal(p, q) and torch.equal(opt.working_copy(p), w)
        for k in s:
            assert torch.equal(opt.get_slot(p, k), s[k])
    assert opt.steps == AC.STEPS and abs(opt.current_decay() - AC.decay(AC.STEPS)) == 0


def test_optimizer_state_dict_round_trip_continues_with_the_same_bits(env):
    from blocksparse_amd import AdafactorOptimizer
    torch, _ = env
    kw = dict(learning_rate=AC.LR, beta2=AC.BETA2, gated=True, working_dtype=torch.bfloat16, **AC.SETTINGS)
    params, grads = _mixed(torch)
    opt = AdafactorOptimizer(params, **kw)
    opt.step(grads=grads)
    opt.step(grads=grads)
    state = opt.state_dict()
    twins, _g = _mixed(torch)
    for p, q in zip(twins, params):
        p.copy_(q)
    opt2 = AdafactorOptimizer(twins, **kw)
    opt2.load_state_dict(state)
    opt.step(grads=grads)
    opt2.step(grads=grads)
    for p, q in zip(params, twins):
        assert torch.equal(p, q) and torch.equal(opt.working_copy(p), opt2.working_copy(q))
        for k in ("cv", "rv"):
            assert opt.get_slot(p, k) is None or torch.equal(opt.get_slot(p, k), opt2.get_slot(q, k))
    assert opt2.steps == 3


def test_optimizer_rejects_other_shapes(env):
    from blocksparse_amd import AdafactorOptimizer, adafactor_step
    torch, _ = env
    w = torch.zeros(2, 3, 4, 5, device="cuda")
    with pytest.raises(ValueError, match="only 1 or 2d params are supported"):
        AdafactorOptimizer([w])
    with pytest.raises(ValueError, match="only 1 or 2d params are supported"):
        adafactor_step(w, w, torch.zeros(5, device="cuda"), torch.zeros(2, device="cuda"))
    with pytest.raises(ValueError, match="only 1 or 2d params are supported"):
        AdafactorOptimizer([torch.zeros(3, 5, 7, device="cuda")])                                # three dimensions, no block size


def test_captured_step_replays_like_eager_steps(env):
    """One captured 2-d step (a linear chain of four launches) replayed twice equals two eager steps with the same decay."""
    from blocksparse_amd import adafactor_step
    torch, _ = env
    c = AC.case("2d-300x520-clip")
    kw = dict(lr=AC.LR, decay=AC.decay(2), **AC.SETTINGS)
    eager, cap = _state(torch, c), _state(torch, c)
    ns = torch.full((1,), AC.NORM_SCALE, device="cuda")
    for _ in range(2):
        adafactor_step(eager[0], eager[1], eager[2], eager[3], norm_scale=ns, param16=eager[4], **kw)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        adafactor_step(cap[0], cap[1], cap[2], cap[3], norm_scale=ns, param16=cap[4], **kw)
    for t, old in zip(cap[:5], _state(torch, c)[:5]):
        assert torch.equal(t, old)                                                                # capturing runs nothing
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for x, y in zip(eager[:5], cap[:5]):
        assert torch.equal(x, y)
