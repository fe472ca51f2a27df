"""GPU tier of the composed model (tests/_model_ref.py): every operator family in one step -- embedding, two tied block-sparse matmuls
(one gated) per time step, fused LSTM gates, layer norm, matmul + bias / fast-GELU / dropout / residual, matmul, softmax cross-entropy,
clipped gated Adam with 16-bit working copies and a moving average.

  1  autograd equals the chain of low-level calls, bit for bit                        test_autograd_equals_the_hand_written_chain
  2  every operator in place against float64 on the device's own inputs               test_every_operator_in_place
  3  the optimizer step in place, and the forward after it                            test_optimizer_step_in_place
  4  three steps through the list optimizer, eagerly                                   test_three_eager_steps_through_the_list_optimizer
     (not captured: closing a capture of forward, ``torch.autograd.grad`` and the list optimizer in one graph is a segmentation fault
     of the process whose cause is not known -- DESIGN.md, "Known fault")
  5  end to end in fp32 against the twin                                              test_end_to_end_fp32
  6  scratch a captured call points at, outgrown by a later eager call                test_outgrown_scratch_under_a_captured_graph

No tolerance is made up here: item 2 applies the criterion of each operator's own GPU test, item 3 the bars of tests/test_optimize_gpu.py.
A bar gives way only by the rule of ``judge``: where the float32 NumPy evaluation of the same helper on the same inputs misses it too,
the bar is 4 x that evaluation's error (fp32 ordering noise passes, a dropped term cannot)."""
import numpy as np
import pytest

import _ends_ref as XR
import _ewops_ref as ER
import _layer_norm_ref as NR
import _lstm_ref as LR
import _model_ref as M
import _optimize_ref as OR
import _parity as P
from oracle import bsmm_oracle as orc

pytestmark = pytest.mark.gpu

NAMES = list(M.VARIANTS)
T, N = M.T, M.N


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    import blocksparse_amd as B
    from blocksparse_amd import _lib
    _lib.load()
    return torch, B, _lib


def host(t):
    return P.to_host(t)


def h64(t):
    return host(t).astype(np.float64)


def batch_dev(torch, name, step=0):
    tokens, labels = M.batch(name, step)
    return torch.from_numpy(np.array(tokens)).cuda(), torch.from_numpy(np.array(labels)).cuda()


def judge(name, got, want64, dtype, ctx, model32=None, max_bar=True, l2_bar=None):
    """The ``check`` of tests/test_lstm_gpu.py, test_ewops_gpu.py and test_layer_norm_gpu.py: finite, and against float64 rounded once to the
    storage type inside the L2 and max bars of the dtype.  ``model32``: the float32 NumPy evaluation of the same helper on the same inputs;
    only where that misses a bar too does the bar become 4 x its error.  ``l2_bar``: another L2 bar than the dtype's (the update of
    tests/test_optimize_gpu.py: 1e-5), then without a max bar.  Returns the figures."""
    want = orc.round_to(np.asarray(want64), dtype) if dtype != "f32" else np.asarray(want64)
    got = host(got) if hasattr(got, "detach") else np.asarray(got)
    assert got.shape == want.shape, (ctx, name, got.shape, want.shape)
    assert np.isfinite(got).all(), (ctx, name)
    l2, mx = P.errors(got, want)
    l2_bar, mx_bar = (P.L2_BAR[dtype], (P.MAX_BAR[dtype] if max_bar else np.inf)) if l2_bar is None else (l2_bar, np.inf)
    note = ""
    if (l2 > l2_bar or mx > mx_bar) and model32 is not None:
        evaluations = model32()                                      # (one array, or a list: the orders float32 can take the formula in)
        evaluations = evaluations if isinstance(evaluations, list) else [evaluations]
        figures = [P.errors(orc.round_to(m, dtype) if dtype != "f32" else np.asarray(m, dtype=np.float32), want) for m in evaluations]
        ml2, mmx = max(e[0] for e in figures), max(e[1] for e in figures)
        if ml2 > l2_bar:
            l2_bar = 4.0 * ml2
        if mmx > mx_bar:
            mx_bar = 4.0 * mmx
        note = "  [float32 evaluation: l2 %.3g max %.3g -> bars %.3g / %.3g]" % (ml2, mmx, l2_bar, mx_bar)
    print(ctx, name, "l2 %.3g max %.3g%s" % (l2, mx, note))
    assert l2 <= l2_bar and mx <= mx_bar, (ctx, name, l2, mx, l2_bar, mx_bar)
    return l2, mx


# ---- one aliased autograd step per variant, shared by items 1 and 2 -----------------------------------------------------------------------
_runs = {}


def aliased_run(env, name):
    """One step through the autograd functions with every intermediate's gradient retained and every use of a tied tensor aliased; made once
    per variant and only read afterwards."""
    torch, B, _ = env
    if name not in _runs:
        model, twin = M.build(name, torch, alias=True)
        tokens, labels = batch_dev(torch, name)
        B.set_entropy(M.SEED, offset=M.OFFSET)
        loss, mask, f = model.forward(tokens, labels, keep=True)
        loss.backward()
        torch.cuda.synchronize()
        _runs[name] = (model, twin, tokens, labels, mask, f)
    return _runs[name]


def hand_chain(env, model, tokens, labels, mask):
    """The same step through the low-level calls, in the order autograd ran them: ({name: intermediate}, {name: gradient})."""
    torch, B, _ = env
    s, L, ops = model.spec, model.leaf, model.ops
    ax = M.ax_of(s)
    f, d = {}, {}
    f["emb"], order = B.embed.embedding_lookup_fwd(L["table"], tokens)
    c, h = L["c0"], L["h0"]
    cin, hin = [], []
    for t in range(T):
        x = f["x%d" % t] = f["emb"][t] if s.axis else f["emb"][t].t().contiguous()
        cin.append(c), hin.append(h)
        a = f["a%d" % t] = ops["x"].fprop(x, L["Wx"], gate=L["gx"])
        b = f["b%d" % t] = ops["h"].fprop(h, L["Wh"])
        z = f["z%d" % t] = a + b
        c, h = B.lstm.fused_lstm_gates_fwd(c, z, bias=L["bg"], forget_bias=M.FB, axis=ax)
        f["c%d" % (t + 1)], f["h%d" % (t + 1)] = c, h
    y, mean, rstd = B.norms.layer_norm_fwd(h, L["g"], L["b"], s.axis, 1, M.EPS)
    f["y"] = y
    o = f["o"] = ops["o"].fprop(y, L["Wo"])
    u, mask2 = B.ewops.bias_dropout_fwd(o, L["bo"], M.KEEP, ax, False, True, y, mask)       # the first run's mask, read
    assert mask2 is mask or torch.equal(mask2, mask)
    f["u"] = u
    logits = f["logits"] = ops["l"].fprop(u, L["Wl"])
    rows = logits if s.axis else logits.t().contiguous()
    if not s.axis:
        f["rows"] = rows
    f["loss_rows"], stash = B.xent.softmax_cross_entropy_fwd(rows, labels)
    f["loss"] = f["loss_rows"].mean()
    # backward
    d["loss_rows"] = torch.full((N,), 1.0 / N, dtype=torch.float32, device="cuda")
    drows = B.xent.softmax_cross_entropy_bwd(stash, d["loss_rows"])
    if not s.axis:
        d["rows"] = drows
    d["logits"] = drows if s.axis else drows.t()                     # non-contiguous, as autograd hands it on
    d["u"] = ops["l"].bprop(d["logits"], L["Wl"])
    d["Wl"] = ops["l"].updat(u, d["logits"])
    d["o"], d["bo"] = B.ewops.bias_dropout_bwd(d["u"], o, L["bo"], mask, M.KEEP, ax, False, True)
    d["o_bprop"] = ops["o"].bprop(d["o"], L["Wo"])
    d["Wo"] = ops["o"].updat(y, d["o"])
    d["y"] = d["u"] + d["o_bprop"]                                  # the residual's gradient is du itself
    eh, d["g"], d["b"] = B.norms.layer_norm_bwd(d["y"], f["h%d" % T], L["g"], L["b"], mean, rstd, s.axis, 1, M.EPS)
    ec = None
    demb = [None] * T
    for t in reversed(range(T)):
        d["h%d" % (t + 1)], d["c%d" % (t + 1)] = eh, ec
        dc, dz = B.lstm.fused_lstm_gates_bwd(cin[t], f["z%d" % t], eh=eh, ec=ec, bias=L["bg"], forget_bias=M.FB, axis=ax)
        d["z%d" % t] = d["a%d" % t] = d["b%d" % t] = dz
        d[("bg", t)] = B.ewops.bias_relu_bwd(dz, None, L["bg"], axis=ax)[1]
        eh_prev = ops["h"].bprop(dz, L["Wh"])
        d[("Wh", t)] = ops["h"].updat(hin[t], dz)
        dx = d["x%d" % t] = ops["x"].bprop(dz, L["Wx"], gate=L["gx"])
        dw = ops["x"].updat(f["x%d" % t], dz, gate=L["gx"])
        d[("Wx", t)], d[("gx", t)] = ops["x"].gate_grad(dw, L["Wx"], L["gx"])
        demb[t] = dx if s.axis else dx.t()
        eh, ec = eh_prev, dc
    d["h0"], d["c0"] = eh, ec
    d["emb"] = torch.stack(demb)
    d["table"] = B.embed.embedding_lookup_bwd(d["emb"], tokens, M.V, order=order).to(L["table"].dtype)
    return f, d


@pytest.mark.parametrize("name", NAMES)
def test_autograd_equals_the_hand_written_chain(env, name):
    """Item 1.  The same step twice: the autograd functions with ``loss.backward()``, then fprop / bprop / updat / gate_grad, the ``*_fwd`` /
    ``*_bwd`` calls and ``embedding_lookup_bwd`` in the order autograd ran them, on the mask the first run returned.  ``torch.equal`` on
    every intermediate, every retained gradient, every parameter gradient, dg and the mask words.
    A tied tensor's gradient is read per use through an alias (``w.view_as(w)`` per time step, ``retain_grad``).  Backward runs the time steps
    last to first and AccumulateGrad adds each use's gradient as it arrives, in the leaf's dtype: the leaf holds (g[T-1] + g[T-2]) + ... + g[0]."""
    torch, B, _ = env
    model, twin, tokens, labels, mask, f = aliased_run(env, name)
    L = model.leaf
    assert np.array_equal(ER.as_u32(mask), twin.mask_words), "the mask is not the generating call's"
    hf, hd = hand_chain(env, model, tokens, labels, mask)
    torch.cuda.synchronize()
    assert set(hf) == set(f), set(hf) ^ set(f)
    for k in sorted(f):
        assert f[k].dtype == hf[k].dtype and torch.equal(f[k], hf[k]), (name, "forward", k)
    for k in sorted(f):
        if k == "loss":
            continue
        got = f[k].grad
        if k == "c%d" % T:                                           # the last cell state feeds nothing
            assert got is None and hd[k] is None
            continue
        assert got is not None and got.dtype == hd[k].dtype and torch.equal(got, hd[k]), (name, "gradient of", k)
    for k in ("table", "g", "b", "Wo", "bo", "Wl", "c0", "h0"):
        assert L[k].grad.dtype == L[k].dtype and torch.equal(L[k].grad, hd[k]), (name, "leaf gradient", k)
    for k in M.TIED:
        per_use = [model.uses[(k, t)].grad for t in range(T)]
        for t in range(T):
            assert torch.equal(per_use[t], hd[(k, t)]), (name, "gradient of use", k, t)
        total = per_use[T - 1]
        for t in reversed(range(T - 1)):
            total = total + per_use[t]
        assert L[k].grad.dtype == L[k].dtype and torch.equal(L[k].grad, total), (name, "tied gradient is not (g[T-1] + ...) + g[0]", k)
        assert not torch.equal(per_use[0], per_use[1])


# ---- item 2 ---------------------------------------------------------------------------------------------------------------------------------
def _blocks(got, want64, dtype, groups, ctx):
    """P.assert_blocks, with the figures printed."""
    rep = P.assert_blocks(got, want64, dtype, groups, ctx)
    print(ctx, "tensor l2 %.3g worst block %.3g adjacent %d" % (rep["tensor_l2"], rep["block_l2"], rep["elem_flips"]))
    return rep


def _blocks_act(got, want64, s, F, ctx):
    fb = F // s.bsize
    return _blocks(P.act_blocks(host(got), s.axis, N, fb, s.bsize), P.act_blocks(want64, s.axis, N, fb, s.bsize), s.dtype, fb, ctx)


@pytest.mark.parametrize("name", NAMES)
def test_every_operator_in_place(env, name):
    """Item 2.  Every operator instance of the aliased autograd step, forward and backward: its inputs as the device had them (the incoming
    gradient included) go to the host, its float64 helper is evaluated on them, and the criterion of that operator's own GPU test applies:
    P.assert_blocks per block column / per block for the matmuls (a gated weight gradient as tests/test_gating.py takes it: the float64
    updat rounded as the kernel leaves it, then gate_grad), ``check`` for the LSTM gates (gradients without the max bar, db as the fp32 sum of
    the stored gate gradients), the layer norm and the fused bias / fast-GELU / dropout, exact rows, check_16bit / check_dw and the fp32
    bounds for the ends.  Two gradients autograd never shows on their own are recomputed through the low-level call on the same device
    tensors and tied to what autograd produced bit for bit: bprop of the head matmul (autograd adds the residual's gradient to it) and the
    stash of the cross-entropy."""
    torch, B, _ = env
    model, twin, tokens, labels, mask, f = aliased_run(env, name)
    s, L, tab, ops = model.spec, model.leaf, twin.tab, model.ops
    ax, dt = M.ax_of(s), s.dtype
    feats = M.features(s)
    gx = h64(L["gx"])
    tok = np.asarray(twin.tokens).reshape(-1)

    # embedding
    table = host(L["table"])
    assert np.array_equal(host(f["emb"]).reshape(T * N, s.C), XR.embed_fwd_ref(table, tok)), "embedding rows"
    want, named = XR.embed_grad_ref(host(f["emb"].grad).reshape(T * N, s.C), tok, M.V)
    got = host(L["table"].grad)
    assert named.sum() == M.V - 2
    if dt == "f32":
        XR.check_dw(got, want, named, (name, "table"))
    else:
        assert not got[~named].any(), (name, "rows no token names")
        XR.check_16bit(got[named], want[named], dt, (name, "table"))

    # the recurrence
    for t in range(T):
        x, dz = h64(f["x%d" % t]), h64(f["z%d" % t].grad)
        hin = h64(f["h%d" % t] if t else L["h0"])
        cin_t = f["c%d" % t] if t else L["c0"]
        for op, inp, out in (("x", x, "a%d" % t), ("h", hin, "b%d" % t)):
            w, gate = h64(L[M.WEIGHT_OF[op]]), (gx if op == "x" else None)
            _blocks_act(f[out], orc.fprop(tab[op], inp, w, s.axis, gate=gate), s, feats[op][1], (name, t, op, "fprop"))
            dinp = f["x%d" % t].grad if op == "x" else (f["h%d" % t].grad if t else L["h0"].grad)
            _blocks_act(dinp, orc.bprop(tab[op], dz, w, s.axis, gate=gate), s, feats[op][0], (name, t, op, "bprop"))
            blocks = tab[op]["blocks"]
            dw = host(model.uses[(M.WEIGHT_OF[op], t)].grad)
            if op == "h":
                _blocks(dw, orc.updat(tab[op], inp, dz, s.axis), dt, blocks, (name, t, op, "updat"))
            else:
                stored = P.round_to_storage(orc.updat(tab[op], inp, dz, s.axis, gate=gate), dt)
                dw_ref, dg_ref = orc.gate_grad(stored, w, gate)
                _blocks(dw, dw_ref, dt, blocks, (name, t, op, "gated updat + gate_grad"))
                l2, _ = P.errors(host(model.uses[("gx", t)].grad), dg_ref)
                print((name, t), "dg l2 %.3g" % l2)
                assert l2 <= max(P.L2_BAR[dt], 2e-6), (name, t, "dg", l2)
                assert not dw[gx == 0].any()
        # (the sum of two stored tensors, rounded once)
        judge("a + b", f["z%d" % t], h64(f["a%d" % t]) + h64(f["b%d" % t]), dt, (name, t))
        c32, z32, bg = host(cin_t), host(f["z%d" % t]), host(L["bg"])
        gates = LR.split(z32, ax)
        cn, hn = LR.forward(c32, gates, bg, M.FB, ax)
        fwd32 = lambda i: (lambda: B.lstm.fused_lstm_gates_test(c32, z32, bias=bg, forget_bias=M.FB, axis=ax)[i])
        judge("c_next", f["c%d" % (t + 1)], cn, dt, (name, t), fwd32(0))
        judge("h_next", f["h%d" % (t + 1)], hn, dt, (name, t), fwd32(1))
        eh, ec = f["h%d" % (t + 1)].grad, f["c%d" % (t + 1)].grad
        assert eh is not None and (ec is None) == (t == T - 1)
        eh, ec = host(eh), (None if ec is None else host(ec))
        dc, dgates, _ = LR.backward(c32, gates, eh, ec, bg, M.FB, ax)
        bwd32 = lambda i: (lambda: B.lstm.fused_lstm_gates_grad_test(c32, z32, eh=eh, ec=ec, bias=bg, forget_bias=M.FB, axis=ax)[i])
        judge("dc", cin_t.grad, dc, dt, (name, t), bwd32(0), max_bar=False)
        judge("dgates", f["z%d" % t].grad, LR.fuse(dgates, ax), dt, (name, t), bwd32(1), max_bar=False)
        other = tuple(q for q in range(2) if q != (ax % 2))
        judge("db", model.uses[("bg", t)].grad, h64(f["z%d" % t].grad).sum(axis=other), "f32", (name, t))

    # layer norm
    hT, g, b, dy = host(f["h%d" % T]), host(L["g"]), host(L["b"]), host(f["y"].grad)
    mean32, rstd32 = NR.stats_f32_two_pass(hT, ax, 1, M.EPS)
    judge("ln y", f["y"], NR.forward(hT, g, b, ax, 1, M.EPS), dt, name, lambda: NR.forward_f32(hT, g, b, mean32, rstd32, ax, 1))
    dx, dg, db = NR.backward(dy, hT, g, b, ax, 1, M.EPS)
    ln32 = lambda i: (lambda: NR.backward_f32(dy, hT, g, mean32, rstd32, ax, 1)[i])
    judge("ln dx", f["h%d" % T].grad, dx, dt, name, ln32(0))
    judge("ln dg", L["g"].grad, dg, "f32", name, ln32(1))
    judge("ln db", L["b"].grad, db, "f32", name, ln32(2))

    # head matmul, fused bias / fast-GELU / dropout / residual
    y, o, u = h64(f["y"]), host(f["o"]), host(f["u"])
    wo, bo = h64(L["Wo"]), host(L["bo"])
    _blocks_act(f["o"], orc.fprop(tab["o"], y, wo, s.axis), s, s.H, (name, "o", "fprop"))
    assert np.array_equal(ER.as_u32(mask), twin.mask_words)
    kept = ER.unpack(ER.as_u32(mask), N * s.H).reshape(o.shape)
    scale = ER.scale_of(M.KEEP)
    y32 = host(f["y"])
    judge("dropout y", f["u"], ER.forward(o, bo, ax, 2, kept, scale, y32), dt, name,
          lambda: B.ewops.bias_dropout_test(o, bo, ER.as_u32(mask).view(np.int32), M.KEEP, axis=ax, fast_gelu=True, residual=y32))
    du = host(f["u"].grad)
    dxo, dbo = ER.backward(du, o, bo, ax, 2, kept, scale)
    ew32 = lambda i: (lambda: B.ewops.bias_dropout_grad_test(du, o, bo, ER.as_u32(mask).view(np.int32), M.KEEP, axis=ax, fast_gelu=True)[i])
    judge("dropout dx", f["o"].grad, dxo, dt, name, ew32(0))
    judge("dropout db", L["bo"].grad, dbo, "f32", name, ew32(1))
    bp = ops["o"].bprop(f["o"].grad, L["Wo"])
    assert torch.equal(f["y"].grad, f["u"].grad + bp), (name, "the layer norm's incoming gradient is not residual + bprop")
    _blocks_act(bp, orc.bprop(tab["o"], h64(f["o"].grad), wo, s.axis), s, s.H, (name, "o", "bprop"))
    _blocks(host(L["Wo"].grad), orc.updat(tab["o"], y, h64(f["o"].grad), s.axis), dt, tab["o"]["blocks"], (name, "o", "updat"))

    # logits and the loss
    wl, dlog = h64(L["Wl"]), h64(f["logits"].grad)
    _blocks_act(f["logits"], orc.fprop(tab["l"], u.astype(np.float64), wl, s.axis), s, s.classes, (name, "l", "fprop"))
    _blocks_act(f["u"].grad, orc.bprop(tab["l"], dlog, wl, s.axis), s, s.H, (name, "l", "bprop"))
    _blocks(host(L["Wl"].grad), orc.updat(tab["l"], u.astype(np.float64), dlog, s.axis), dt, tab["l"]["blocks"], (name, "l", "updat"))
    rows_t = f["logits"] if s.axis else f["rows"]
    rows = host(rows_t)
    lab = np.asarray(twin.labels)
    wloss, wg, wp, wdist = XR.xent_ref(rows, lab)
    l2, mx = P.errors(host(f["loss_rows"]), wloss)
    print(name, "loss rows l2 %.3g max %.3g" % (l2, mx))
    assert l2 <= P.L2_BAR["f32"] and mx <= P.MAX_BAR["f32"], (name, "loss", l2, mx)
    loss2, stash = B.xent.softmax_cross_entropy_fwd(rows_t.detach(), labels)
    assert torch.equal(loss2, f["loss_rows"])
    dyl = host(f["loss_rows"].grad)
    assert np.array_equal(dyl, np.full(N, 1.0 / N, dtype=np.float32))
    assert torch.equal(B.xent.softmax_cross_entropy_bwd(stash, f["loss_rows"].grad), rows_t.grad), (name, "the stash is not the one autograd kept")
    sc = XR.stash_scale(dt)
    st, gdx = host(stash), host(rows_t.grad)
    if dt == "f32":
        ratio, at = XR.f32_g_ratio(st, wg, wp, wdist)
        print(name, "fp32 g worst ratio to the bound %.3f" % ratio)
        assert ratio <= 1.0, (name, "fp32 g beyond its bound", ratio, at)
        XR.check_f32_dx(gdx, st, dyl, (name, "xent dx"))
    else:
        XR.check_16bit(st, wg * sc, dt, (name, "xent g"))
        XR.check_16bit(gdx, st.astype(np.float64) / sc * dyl.astype(np.float64)[:, None], dt, (name, "xent dx"))
    assert not gdx[lab < 0].any() and host(f["loss_rows"])[lab < 0] == 0
    l2, mx = P.errors(np.array([float(f["loss"].detach())]), np.array([h64(f["loss_rows"]).mean()]))
    assert l2 <= P.L2_BAR["f32"], (name, "mean", l2)


# ---- items 3 and 5: one plain step, the optimizer, a second forward --------------------------------------------------------------------------
_plain = {}


def plain_run(env, name):
    """Forward, backward, clip, ``AdamOptimizer.step``, ``Ema.apply`` and a second forward on one model without aliases (the parameter objects
    themselves reach the matmuls, so the per-weights caches are in play); made once per variant and only read afterwards."""
    torch, B, _ = env
    if name not in _plain:
        model, twin = M.build(name, torch)
        tokens, labels = batch_dev(torch, name)
        tf = twin.forward()
        td = twin.backward(tf)
        clip = twin.clip_norm(td)
        B.set_entropy(M.SEED, offset=M.OFFSET)
        loss, mask, f = model.forward(tokens, labels)
        loss.backward()
        r = dict(model=model, twin=twin, tf=tf, td=td, clip=clip, loss=float(loss.detach()), mask=mask.clone(), a0=f["a0"].detach().clone())
        r["grads"] = {k: model.leaf[k].grad.clone() for k in M.PARAMS + M.EXTRA}
        r["before"] = {k: v.clone() for k, v in model.state().items()}
        r["norm"], r["scale"] = B.clip_by_global_norm(model.grads(), clip_norm=clip)
        model.opt.step(grads=model.grads(), norm_scale=r["scale"])
        model.ema.apply([model.master[k] for k in M.PARAMS])
        r["after"] = {k: v.clone() for k, v in model.state().items()}
        with torch.no_grad():
            _, _, f2 = model.forward(tokens, labels)
        r["x0"], r["a0_after"] = f2["x0"].clone(), f2["a0"].clone()
        torch.cuda.synchronize()
        _plain[name] = r
    return _plain[name]


@pytest.mark.parametrize("name", NAMES)
def test_optimizer_step_in_place(env, name):
    """Item 3.  From the device's own gradients: the clip against _optimize_ref.clip (2e-6 relative, as tests/test_optimize_gpu.py), then param,
    Mean and Var of every tensor against _optimize_ref.adam at the fp32 bars of that file, with the device's own norm scale.  Gated-off
    blocks keep their bits in master, moments, working copy and average; a working copy is its master rounded once; an average starts as
    its stepped param.  Then the forward after the step: the first matmul per block column against float64 on the STEPPED weights, where
    the result of the old weights is far outside the bar.
    Bars replaced under the rule of ``judge`` (device / float32 evaluation of _optimize_ref.adam, _model_ref.adam_float32 / new bar):
      Var of Wx, max |diff| / mean |ref| against 2e-5:  row32-bf16 2.21e-5 / 2.21e-5 / 8.83e-5,  row32-f32 3.46e-5 / 3.46e-5 / 1.38e-4
        (the moments start at zero, so Var is (1 - beta2) g^2 with no floor: its largest element is well over a hundred times its mean, where three fp32
        roundings of that element are already 2e-5 of the mean -- the remark in test_optimizer_and_ema_classes of tests/test_optimize_gpu.py)
      the update p - p0, L2 against 1e-5 (float32 evaluation: adam_float32's param less p0 -- half an ulp of a param near 1 against a step
      of 2e-3):  table 2.21e-5 / 2.21e-5 / 8.82e-5 (row32-bf16), 2.17e-5 / 2.17e-5 / 8.68e-5 (col16-f16), 2.22e-5 / 2.22e-5 / 8.89e-5 (row32-f32);
        col16-f16 Wh 1.32e-5 / 1.32e-5 / 5.30e-5 and g 1.10e-5 / 1.10e-5 / 4.42e-5."""
    torch, B, _ = env
    r = plain_run(env, name)
    model, twin = r["model"], r["twin"]
    s = model.spec
    G = {k: h64(r["grads"][k]) for k in M.PARAMS}
    want_norm, want_scale = OR.clip([OR.sum_squared(G[k]) for k in M.PARAMS], r["clip"])
    norm, scale = float(r["norm"]), float(r["scale"])
    print(name, "norm %.6g scale %.6g (float64: %.6g %.6g)" % (norm, scale, want_norm, want_scale))
    assert abs(norm - want_norm) <= 2e-6 * want_norm and abs(scale - want_scale) <= 2e-6 * want_scale
    assert 0.6 <= scale <= 0.8                                       # about CLIP_SHARE: the clip norm comes from the float64 twin
    before, after = r["before"], r["after"]
    state0 = {k: (h64(before["p." + k]).reshape(-1), h64(before["m." + k]).reshape(-1), h64(before["v." + k]).reshape(-1), None) for k in M.PARAMS}
    state1, _ = twin.optimizer_step(state0, G, r["clip"], 1, norm_scale=np.float32(scale))
    assert model.opt.steps == 1
    lr_t = M.LRATE * OR.lr_correction_loop(1, 0.9, 0.999)
    for k in M.PARAMS:
        gate, bs = (twin.p["gx"], s.bsize) if k == "Wx" else (None, 0)
        f32 = lambda i, k=k, gate=gate, bs=bs: [M.adam_float32(*state0[k][:3], G[k], lr_t, gate=gate, bsize=bs, clip_sigma=M.CLIP_SIGMAS,
                                                                 norm_scale=np.float32(scale), square_first=sq)[i] for sq in (False, True)]
        for i, (tag, ref) in enumerate(zip("pmv", state1[k][:3])):
            got = host(after[tag + "." + k]).reshape(-1)
            assert not np.array_equal(got, host(before[tag + "." + k]).reshape(-1)), (name, k, tag, "did not move")
            judge("%s.%s" % (tag, k), got, ref, "f32", name, lambda i=i, f32=f32: f32(i))
        # the update p - p0 at the 1e-5 of tests/test_optimize_gpu.py (float32 evaluation: the float32 param of adam_float32 less p0)
        judge("update of " + k, h64(after["p." + k]).reshape(-1) - state0[k][0], state1[k][0] - state0[k][0], "f32", name,
              lambda f32=f32, k=k: [m.astype(np.float64) - state0[k][0] for m in f32(0)], l2_bar=1e-5)
        assert torch.equal(after["e." + k], after["p." + k]), (name, k, "an average starts as its stepped param")
        if "w." + k in after:
            assert torch.equal(after["w." + k], after["p." + k].to(after["w." + k].dtype)), (name, k, "working copy is not the master rounded once")
    off = model.gx.detach() == 0
    assert int(off.sum()) >= 2
    for tag in "pmvwe":
        if tag + ".Wx" in after:
            old = before.get(tag + ".Wx", before["p.Wx"])
            assert torch.equal(after[tag + ".Wx"][off], old[off]), (name, tag, "a gated-off block moved")
            assert not torch.equal(after[tag + ".Wx"][~off], old[~off])
    # the forward after the step
    tab = twin.tab["x"]
    w_now = h64(model.leaf["Wx"])
    assert not np.array_equal(w_now, np.asarray(twin.p["Wx"], dtype=np.float64))
    want = orc.fprop(tab, h64(r["x0"]), w_now, s.axis, gate=h64(model.gx))
    stale, _ = P.errors(host(r["a0"]), P.round_to_storage(want, s.dtype))
    print(name, "first matmul after the step: the old weights' result is off by %.3g" % stale)
    assert stale > 4 * P.L2_BAR[s.dtype]
    _blocks_act(r["a0_after"], want, s, 4 * s.H, (name, "fprop after the step"))


def test_end_to_end_fp32(env):
    """Item 5.  row32-f32, step 0: loss and parameter gradients of the device against the float64 twin run end to end, no teacher forcing.
    The bar of each tensor is 4 x the error of the twin evaluated in float32 (on the host, against the float64 twin), with the floor
    P.L2_BAR["f32"]; both figures are printed.  Measured (device / float32 twin / bar): loss 2.8e-8 / 4.3e-9 / 2e-6; table 7.7e-7 / 6.8e-7 /
    2.7e-6; Wx 7.9e-7 / 7.7e-7 / 3.1e-6; Wh 8.4e-7 / 7.0e-7 / 2.8e-6; bg 7.0e-7 / 6.0e-7 / 2.4e-6; g 3.3e-7 / 2.9e-7 / 2e-6; b 3.4e-7 / 3.8e-7 /
    2e-6; Wo 5.7e-7 / 5.0e-7 / 2e-6; bo 3.9e-7 / 3.4e-7 / 2e-6; Wl 4.6e-7 / 4.1e-7 / 2e-6; gx 1.18e-6 / 1.02e-6 / 4.1e-6; c0 8.1e-7 / 6.3e-7 /
    2.5e-6; h0 9.2e-7 / 7.9e-7 / 3.2e-6."""
    torch, B, _ = env
    name = "row32-f32"
    r = plain_run(env, name)
    twin, tf, td = r["twin"], r["tf"], r["td"]
    f32 = twin.forward(prec="f32")
    d32 = twin.backward(f32)
    assert torch.equal(torch.from_numpy(twin.mask_words.view(np.int32)), r["mask"].cpu())
    model_err = abs(f32["loss"] - tf["loss"]) / abs(tf["loss"])
    bar = max(4.0 * model_err, P.L2_BAR["f32"])
    err = abs(r["loss"] - tf["loss"]) / abs(tf["loss"])
    print("loss %.8g (float64 %.8g): error %.3g, float32 twin %.3g, bar %.3g" % (r["loss"], tf["loss"], err, model_err, bar))
    failed = [] if err <= bar else [("loss", err, bar)]
    for k in M.PARAMS + M.EXTRA:
        model_err, _ = P.errors(d32[k], td[k])
        bar = max(4.0 * model_err, P.L2_BAR["f32"])
        err, _ = P.errors(h64(r["grads"][k]), td[k])
        print("%-6s error %.3g, float32 twin %.3g, bar %.3g" % (k, err, model_err, bar))
        if not err <= bar:
            failed.append((k, err, bar))
    assert not failed, failed


# ---- item 4, eagerly --------------------------------------------------------------------------------------------------------------------------
class _Trainer(object):
    """A model with static inputs and gradient buffers and the list optimizer bound to them.  ``step`` is forward, ``torch.autograd.grad``,
    a copy into the static gradients (plus ``poison``: 0, or Inf for a step that must skip itself) and the prepared clip / Adam / average."""

    def __init__(self, env, name, clip):
        torch, B, _ = env
        self.torch, self.name, self.model = torch, name, M.build(name, torch)[0]
        m = self.model
        self.tokens, self.labels = (t.clone() for t in batch_dev(torch, name))
        self.static = [torch.zeros_like(m.leaf[k]) for k in M.PARAMS]
        self.poison = torch.zeros(1, dtype=self.static[3].dtype, device="cuda")
        self.prepared = m.opt.prepare(grads=self.static, clip_norm=clip, ema=m.ema)

    def step(self, step, poison):
        m = self.model
        tokens, labels = batch_dev(self.torch, self.name, step)
        self.tokens.copy_(tokens), self.labels.copy_(labels)
        self.poison.fill_(poison)
        loss, mask, _ = m.forward(self.tokens, self.labels)
        grads = self.torch.autograd.grad(loss, [m.leaf[k] for k in M.PARAMS] + [m.gx])
        for dst, g in zip(self.static, grads):
            dst.copy_(g)
        clean = [g.clone() for g in self.static]
        self.static[3].view(-1)[5:6].add_(self.poison)               # (bg, fp32)
        self.prepared.run()
        return loss.detach(), mask, clean


POISON = (0.0, float("inf"), 0.0)


@pytest.mark.parametrize("name", ["row32-bf16", "row32-f32"])
def test_three_eager_steps_through_the_list_optimizer(env, name):
    """What item 4 runs, without the capture: three steps of forward, ``torch.autograd.grad``, a copy into static gradient buffers and
    ``opt.prepare(grads=static, clip_norm=.., ema=..).run()`` on fresh tokens and labels, the second with an Inf planted in a gradient.
    Every step from the device's own state and gradients against _optimize_ref (the twin's ``optimizer_step``, step number i + 1, the
    device's own norm scale) at the bars of item 3; the mask is the generating call's at offset OFFSET + i; ``rates()`` is the corrected rate
    of step i + 1 (the count advances on a skipped step too); the Inf step has scale 0 and leaves params, moments and working copies
    bit for bit while the averages move on.  row32-f32: loss and gradients of every step against the float64 twin on the weights the
    device holds at that step, at the bar of item 5 -- a tensor saved for backward that the optimizer overwrote, or a per-weights cache
    that outlived a step, cannot pass that.
    Bars replaced under the rule of ``judge``: step 0 only, Var of Wx as in item 3 (2.21e-5 / 2.21e-5 / 8.83e-5 for row32-bf16, 3.46e-5 /
    3.46e-5 / 1.38e-4 for row32-f32); from the second step on the moments have a floor.  row32-f32, worst over the three steps (device /
    float32 twin / bar): loss 2.8e-8 / 4.3e-9 / 2e-6, gradients Wx 9.1e-7 / 8.7e-7 / 3.5e-6."""
    torch, B, _ = env
    first = M.Twin(name)
    clip = first.clip_norm(first.backward(first.forward()))
    B.set_entropy(M.SEED, offset=M.OFFSET)
    tr = _Trainer(env, name, clip)
    model, s = tr.model, tr.model.spec
    masks = []
    for i in range(3):
        twin = M.Twin(name, step=i)
        before = {k: v.clone() for k, v in model.state().items()}
        held = {k: host(model.leaf[k]) for k in M.PARAMS + M.EXTRA}  # the weights this step's forward reads
        loss, mask, clean = tr.step(i, POISON[i])
        torch.cuda.synchronize()
        after = {k: v.clone() for k, v in model.state().items()}
        assert np.array_equal(ER.as_u32(mask), twin.mask_words), (name, i, "mask")
        masks.append(mask.clone())
        if s.dtype == "f32":
            f64 = twin.forward(values=held)
            d64 = twin.backward(f64)
            f32 = twin.forward(values=held, prec="f32")
            d32 = twin.backward(f32)
            model_err = abs(f32["loss"] - f64["loss"]) / abs(f64["loss"])
            err, bar = abs(float(loss) - f64["loss"]) / abs(f64["loss"]), max(4.0 * model_err, P.L2_BAR["f32"])
            print(name, i, "loss error %.3g, float32 twin %.3g, bar %.3g" % (err, model_err, bar))
            assert err <= bar, (name, i, "loss", err, bar)
            for k, g in zip(M.PARAMS, clean):
                model_err, _ = P.errors(d32[k], d64[k])
                err, _ = P.errors(h64(g), d64[k])
                bar = max(4.0 * model_err, P.L2_BAR["f32"])
                print(name, i, "%-6s error %.3g, float32 twin %.3g, bar %.3g" % (k, err, model_err, bar))
                assert err <= bar, (name, i, k, err, bar)
        scale, norm = float(tr.prepared.norm_scale), float(tr.prepared.global_norm)
        G = {k: h64(g) for k, g in zip(M.PARAMS, tr.static)}
        lr_t = M.LRATE * OR.lr_correction_loop(i + 1, 0.9, 0.999)
        rate = float(tr.prepared.rates()[0])
        assert abs(rate - lr_t) <= 2e-6 * lr_t, (name, i, "rates()", rate, lr_t)
        moved = [k for k in before if not torch.equal(after[k], before[k])]
        if POISON[i]:
            assert scale == 0.0 and not np.isfinite(norm)
            assert not [k for k in moved if k[0] in "pmvw"], (name, i, moved)
            assert [k for k in moved if k[0] == "e"], (name, i, "the averages stand still")
        else:
            want_norm, want_scale = OR.clip([OR.sum_squared(G[k]) for k in M.PARAMS], clip)
            assert abs(norm - want_norm) <= 2e-6 * want_norm and abs(scale - want_scale) <= 2e-6 * want_scale and 0 < scale < 1
            assert set(moved) == set(before), (name, i, sorted(set(before) - set(moved)))
        flat = lambda t: h64(t).reshape(-1)
        state0 = {k: tuple(flat(before[tag + "." + k]) for tag in "pmve") for k in M.PARAMS}
        state1, _ = twin.optimizer_step(state0, G, clip, i + 1, norm_scale=np.float32(scale))
        for k in M.PARAMS:
            gate, bs = (twin.p["gx"], s.bsize) if k == "Wx" else (None, 0)
            f32m = lambda j, k=k, gate=gate, bs=bs: [M.adam_float32(*state0[k][:3], G[k], lr_t, gate=gate, bsize=bs, clip_sigma=M.CLIP_SIGMAS,
                                                                     norm_scale=np.float32(scale), square_first=sq)[j] for sq in (False, True)]
            for j, tag in enumerate("pmv"):
                if POISON[i]:
                    assert np.array_equal(state1[k][j], state0[k][j])
                else:
                    judge("%s.%s" % (tag, k), flat(after[tag + "." + k]), state1[k][j], "f32", (name, i), lambda j=j, f32m=f32m: f32m(j))
            l2, _ = P.errors(flat(after["e." + k]), state1[k][3])
            assert l2 <= P.L2_BAR["f32"], (name, i, "average", k, l2)
            if "w." + k in after:
                assert torch.equal(after["w." + k], after["p." + k].to(after["w." + k].dtype)), (name, i, k, "working copy")
        off = model.gx.detach() == 0
        for tag in "pmvwe":
            if tag + ".Wx" in after:
                assert torch.equal(after[tag + ".Wx"][off], before[tag + ".Wx"][off]), (name, i, tag, "a gated-off block moved")
    assert not torch.equal(masks[0], masks[1]) and not torch.equal(masks[1], masks[2])


# ---- item 6 ---------------------------------------------------------------------------------------------------------------------------------
def _recycle(torch, nbytes, old_ptr, tries):
    """uint8 tensors of ``nbytes`` until one starts at ``old_ptr``: (that tensor or None, everything allocated -- held, so that the
    allocator moves on)."""
    held = []
    for _ in range(tries):
        t = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        held.append(t)
        if t.data_ptr() == old_ptr:
            return t, held
    return None, held


def _outgrown(env, b, tag, small, large, result):
    """``small()`` warmed up and captured on a side stream, replayed; then ``large()`` eagerly on that stream, which outgrows the scratch of
    ``tag``.  The bytes the captured call was pointed at must not come back from the allocator while the operator lives: either the operator
    still holds them, or -- where they did come back -- a replay must leave a tensor that now owns them untouched.  Either way the replay
    computes what the eager small call computes."""
    torch, B, _ = env
    SENTINEL = 0xA5
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        small()
        torch.cuda.synchronize()
        keys = [k for k in b._workspaces if k[2] == tag]
        assert len(keys) == 1, keys
        old = b._workspaces[keys[0]]
        old_ptr, old_bytes = old.data_ptr(), old.numel()
        del old
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            small()
        assert b._workspaces[keys[0]].data_ptr() == old_ptr, "the capture did not reuse the warm-up's scratch: nothing to outgrow"
        graph.replay()
        torch.cuda.synchronize()
        want = result().clone()
        large()
        torch.cuda.synchronize()
        new = b._workspaces[keys[0]]
        assert new.numel() > old_bytes and new.data_ptr() != old_ptr, "the scratch did not grow"
        guard, held = _recycle(torch, old_bytes, old_ptr, 64 if old_bytes < (1 << 20) else 6)
        recycled = guard is not None
        retained = any(t.data_ptr() == old_ptr for t in getattr(b, "_captured_scratch", []))
        print(tag, "old scratch %d bytes at %#x: recycled %s, retained by the operator %s" % (old_bytes, old_ptr, recycled, retained))
        if recycled:
            guard.fill_(SENTINEL)
        result().zero_()
        graph.replay()
        torch.cuda.synchronize()
        touched = int((guard != SENTINEL).sum()) if recycled else 0
        got = result().clone()
    torch.cuda.current_stream().wait_stream(s)
    assert recycled or retained, (tag, "the old scratch was neither handed out again nor retained: the test shows nothing")
    assert touched == 0, (tag, "a replay wrote %d bytes of a tensor that owns the captured call's old scratch" % touched)
    assert torch.equal(got, want), (tag, "the replay differs from the eager result")
    del held


def test_outgrown_scratch_under_a_captured_graph(env):
    """Item 6.  bsize 32, feature axis 1, fp32, the 4 x 12 layout of the model's first matmul.  ``updat`` at N = 64 is warmed up and captured
    on a side stream; an eager ``updat`` at N = 4096 on that stream then needs a larger scratch (67 401 744 -> 79 788 048 bytes).  Second
    case, same construction: ``block_reduced_full_dw`` captured with 1 pair, then run eagerly with 8 (4 096 -> 16 384 bytes).
    The N = 64 case does not discriminate: it passes with or without the retention, because the per-block kernel of short minibatches
    never touches its reserved scratch; it is kept as the construction the other two share.
    Third case: ``updat`` captured at N = 256, the shortest minibatch at which the fp32 weight gradient writes its scratch.
    Before BlocksparseMatMul._scratch retained such buffers, the replaced tensor went back to the allocator with its address baked into
    the graph.  What that showed: at N = 64 the old 67 418 128-byte block came back on the first allocation and the replay left the sentinel
    untouched (the per-block kernel of short minibatches never reads its reserved scratch); at N = 256 the old 68 007 952-byte block came
    back and the replay wrote 7 956 413 bytes of the tensor that owned it; the 4 096-byte block of ``reduced_dw`` did not come back within
    64 allocations of the small pool.  No ``empty_cache()``: the old bytes stay mapped, whoever owns them."""
    torch, B, lib = env
    lay = M.layouts("row32-f32")["x"]
    assert lay.shape == (4, 12)
    b = B.BlocksparseMatMul(lay, block_size=32, feature_axis=1)
    gen = P.gen(torch, 6)
    rand = lambda shape: torch.randn(shape, device="cuda", generator=gen) * 0.1
    x, e = rand(b.i_shape(64)), rand(b.o_shape(64))
    xl, el = rand(b.i_shape(4096)), rand(b.o_shape(4096))
    dw, dwl = torch.zeros(b.w_shape, device="cuda"), torch.zeros(b.w_shape, device="cuda")
    _outgrown(env, b, lib.OP_UPDAT, lambda: b.updat(x, e, dw=dw), lambda: b.updat(xl, el, dw=dwl), lambda: dw)
    t = orc.build_layout_luts(lay, 32)
    P.assert_blocks(host(dw), orc.updat(t, h64(x), h64(e), 1), "f32", b.blocks, "updat N = 64")
    P.assert_blocks(host(dwl), orc.updat_fast(t, h64(xl), h64(el), 1, np.float64), "f32", b.blocks, "updat N = 4096")

    # the same at N = 256, the shortest minibatch at which the fp32 updat takes its split route (bsmm_updat_dispatch.h, f32_split_route) and
    # WRITES the scratch: the bf16 pieces of X and DY and the streaming sums.  At N = 64 the per-block kernel runs and the reserved bytes stay unread
    b1 = B.BlocksparseMatMul(lay, block_size=32, feature_axis=1)
    xm, em = rand(b1.i_shape(256)), rand(b1.o_shape(256))
    dwm = torch.zeros(b1.w_shape, device="cuda")
    _outgrown(env, b1, lib.OP_UPDAT, lambda: b1.updat(xm, em, dw=dwm), lambda: b1.updat(xl, el, dw=dwl), lambda: dwm)
    P.assert_blocks(host(dwm), orc.updat(t, h64(xm), h64(em), 1), "f32", b1.blocks, "updat N = 256")

    b2 = B.BlocksparseMatMul(lay, block_size=32, feature_axis=1)
    xs, es = [rand(b2.i_shape(64)) for _ in range(8)], [rand(b2.o_shape(64)) for _ in range(8)]
    full, full8 = torch.zeros(4, 12, device="cuda"), torch.zeros(4, 12, device="cuda")

    def reduced(pairs, out):
        out.zero_()
        b2.block_reduced_full_dw(xs[:pairs], es[:pairs], dw_full=out)
    _outgrown(env, b2, "reduced_dw", lambda: reduced(1, full), lambda: reduced(8, full8), lambda: full)
    assert float(full.min()) > 0 and float((full8 - full).min()) > 0
