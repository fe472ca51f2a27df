"""One small recurrent model that runs every operator family of the package in one step, and its float64 twin.

    tokens [T, N] -> embedding_lookup(table [V, C])
    t < T:   gates = bsmm_x(x_t, Wx, gate=gx, gate_grad=True, dw_gated=True) + bsmm_h(h, Wh)        (Wx, Wh, bg, gx tied over time)
             c, h  = fused_lstm_gates(c, gates, bias=bg, forget_bias=1.0)
    y      = layer_norm(h_T, g, b)
    u, m   = bias_dropout(bsmm_o(y, Wo), bo, 0.8, fast_gelu=True, residual=y)
    loss   = softmax_cross_entropy(bsmm_l(u, Wl), labels).mean()                                    (one label is -1: an ignored row)

``build`` returns the device model (made of the package's public autograd functions; None without torch) and the twin, both from the same
seeded NumPy inputs.  The twin is assembled from the float64 helpers of the operator tests (oracle/bsmm_oracle.py, _lstm_ref, _layer_norm_ref,
_ewops_ref, _ends_ref, _optimize_ref); the only arithmetic of its own is the sum of two tensors and the mean of the loss.  With feature axis 0
every activation is (features, N): the embedding rows and the logits pass through ``t().contiguous()`` on the device, a plain transpose here.

What the operator registers for a gated weight is not the derivative: with ``dw_gated`` AND ``gate_grad`` the weight gradient carries the
gate twice (updat gates the sums, gate_grad gates them again) and dg is taken of the gated sums -- blocksparse_matmul_grad of the reference
does the same.  The twin returns both: ``Wx`` / ``gx`` as registered, ``Wx_true`` / ``gx_true`` as the derivative (what central differences
see); tests/test_model_host.py pins the relation between the two."""
import collections
import functools

import numpy as np

import _ends_ref as XR
import _ewops_ref as ER
import _layer_norm_ref as NR
import _lstm_ref as LR
import _optimize_ref as OR
import _parity as P
from oracle import bsmm_oracle as orc

N, T, V = 64, 3, 50
KEEP, FB, EPS = 0.8, 1.0, 1e-6
SEED, OFFSET = 0x5EED0123, 7             # the dropout stream: the one generating call of step s sees the offset OFFSET + s
LRATE, DECAY, CLIP_SIGMAS, CLIP_SHARE = 2e-2, 0.99, 3.0, 0.7      # (a first step of about two bf16 steps of a weight)
HEAVY_ROW, ABSENT_ROWS = 7, (13, 41)     # the vocabulary row that holds a quarter of the tokens, the two that no token names

Spec = collections.namedtuple("Spec", "name axis bsize dtype C H classes")
VARIANTS = collections.OrderedDict((s.name, s) for s in (
    Spec("row32-bf16", 1, 32, "bf16", 128, 96, 128),
    Spec("col16-f16", 0, 16, "f16", 64, 48, 64),
    Spec("row32-f32", 1, 32, "f32", 128, 96, 128),      # prepared-weight pieces and the N-dependent fp32 updat scratch are in play
))
OPS = ("x", "h", "o", "l")                               # the four matmuls: input -> gates, hidden -> gates, head, logits
WEIGHT_OF = {"x": "Wx", "h": "Wh", "o": "Wo", "l": "Wl"}
PARAMS = ("table", "Wx", "Wh", "bg", "g", "b", "Wo", "bo", "Wl")      # the optimizer's order
SIXTEEN = ("table", "Wx", "Wh", "Wo", "Wl")              # params the kernels read in the working type (the others are fp32 everywhere)
TIED = ("Wx", "Wh", "bg", "gx")                          # used at every time step
EXTRA = ("gx", "c0", "h0")                               # differentiated, not stepped


def features(spec):
    """op -> (input features, output features)"""
    return {"x": (spec.C, 4 * spec.H), "h": (spec.H, 4 * spec.H), "o": (spec.H, spec.H), "l": (spec.H, spec.classes)}


@functools.lru_cache(maxsize=None)
def layouts(name):
    spec = VARIANTS[name]
    return {op: P.random_layout(fi // spec.bsize, fo // spec.bsize, 0.5, 11 + 7 * i) for i, (op, (fi, fo)) in enumerate(features(spec).items())}


@functools.lru_cache(maxsize=None)
def tables(name):
    return {op: orc.build_layout_luts(lay, VARIANTS[name].bsize) for op, lay in layouts(name).items()}


def act_shape(spec, F):
    return (N, F) if spec.axis else (F, N)


def ax_of(spec):
    return -1 if spec.axis else 0


@functools.lru_cache(maxsize=None)
def batch(name, step=0):
    """(tokens int64 [T, N], labels int64 [N]) of one step, read-only.  One vocabulary row holds more than a quarter of the tokens, two hold
    none, every other occurs; the labels name as many classes as N - 1 live rows can with two classes left out and one named twice; one row
    is ignored (label -1)."""
    spec = VARIANTS[name]
    rng = np.random.RandomState(100 + 17 * step + spec.classes)
    others = np.array([r for r in range(V) if r != HEAVY_ROW and r not in ABSENT_ROWS])
    heavy = T * N // 4 + 8
    rest = T * N - heavy - others.size
    tokens = np.concatenate([np.full(heavy, HEAVY_ROW), others, others[rng.randint(0, others.size, rest)]])
    tokens = rng.permutation(tokens).reshape(T, N).astype(np.int64)
    named = rng.permutation(spec.classes)[:min(spec.classes - 2, N - 2)]
    labels = np.concatenate([named, named[rng.randint(0, named.size, N - 1 - named.size)]])
    labels = np.insert(rng.permutation(labels), rng.randint(0, N), -1).astype(np.int64)
    tokens.setflags(write=False), labels.setflags(write=False)
    return tokens, labels


@functools.lru_cache(maxsize=None)
def initial(name):
    """The parameters, the gate of Wx and the initial state, float32 arrays of values the storage type holds, read-only.  The scales are
    not the N(0, 0.1) of the operator tests: the gate pre-activations have a standard deviation near 3 (saturated sigmoids), some embedding
    rows are three times the others, the layer-norm gain spreads around 1."""
    spec = VARIANTS[name]
    rng = np.random.RandomState(7 + spec.bsize + spec.H)
    tab = tables(name)
    rnd = lambda a: XR.rounded(a, spec.dtype)
    w = lambda op, std: rnd(rng.normal(0.0, std, (tab[op]["blocks"], spec.bsize, spec.bsize)))
    density = lambda op: tab[op]["blocks"] / float(tab[op]["CB"] * tab[op]["KB"])
    p = {}
    p["table"] = rng.normal(0.0, 1.0, (V, spec.C))
    p["table"][::5] *= 3.0
    p["table"] = rnd(p["table"])
    p["Wx"] = w("x", 2.2 / np.sqrt(spec.C * density("x") * 2.2))      # (x has a second moment near 2.2 with the tripled rows)
    p["Wh"] = w("h", 2.5 / np.sqrt(spec.H * density("h") * 0.3))      # (h = sigmoid * tanh has a second moment near 0.3)
    p["bg"] = rng.normal(0.0, 0.5, 4 * spec.H)
    p["g"] = 1.0 + rng.normal(0.0, 0.3, spec.H)
    p["b"] = rng.normal(0.0, 0.3, spec.H)
    p["Wo"] = w("o", 1.5 / np.sqrt(spec.H * density("o")))
    p["bo"] = rng.normal(0.0, 0.5, spec.H)
    p["Wl"] = w("l", 2.0 / np.sqrt(spec.H * density("l") * 2.0))
    blocks = tab["x"]["blocks"]
    gx = rng.uniform(0.25, 1.75, blocks)
    order = rng.permutation(blocks)
    fifth = max(blocks // 5, 1)
    gx[order[:fifth]], gx[order[fifth:2 * fifth]] = 0.0, 1.0          # about a fifth exactly 0 and a fifth exactly 1
    p["gx"] = gx
    p["c0"] = rnd(rng.normal(0.0, 1.0, act_shape(spec, spec.H)))
    p["h0"] = rnd(rng.uniform(-0.9, 0.9, act_shape(spec, spec.H)))
    out = {}
    for k, a in p.items():
        out[k] = np.ascontiguousarray(a, dtype=np.float32)
        out[k].setflags(write=False)
    return out


def kept_bits(spec, step=0):
    """bool, shaped like the dropout's input: what the one generating call of step ``step`` keeps."""
    return ER.keep_bits(N * spec.H, SEED, OFFSET + step, ER.threshold_of(KEEP)).reshape(act_shape(spec, spec.H))


# ---- the twin ---------------------------------------------------------------------------------------------------------------------------
class _Arith(object):
    """The helpers in float64, or ("f32") their float32 evaluation: the matmuls accumulate in float32 (the oracle's batched forms), the layer
    norm is the two-pass float32 model of its own tests, and every other tensor is rounded to float32 where a kernel would store it."""

    def __init__(self, prec):
        assert prec in ("f64", "f32")
        self.f32 = prec == "f32"
        self.dt = np.float32 if self.f32 else np.float64

    def st(self, a):
        return tuple(self.st(q) for q in a) if isinstance(a, tuple) else (None if a is None else np.asarray(a, dtype=self.dt))

    def _w(self, w, gate):
        return self.st(orc._gated(w, gate))

    def fprop(self, t, x, w, axis, gate=None):
        return self.st(orc.fprop_fast(t, x, self._w(w, gate), axis, self.dt) if self.f32 else orc.fprop(t, x, w, axis, gate=gate))

    def bprop(self, t, e, w, axis, gate=None):
        return self.st(orc.bprop_fast(t, e, self._w(w, gate), axis, self.dt) if self.f32 else orc.bprop(t, e, w, axis, gate=gate))

    def updat(self, t, x, e, axis):
        return self.st(orc.updat_fast(t, x, e, axis, self.dt) if self.f32 else orc.updat(t, x, e, axis))

    def ln_fwd(self, x, g, b, ax):
        if self.f32:
            mean, rstd = NR.stats_f32_two_pass(x, ax, 1, EPS)
            return NR.forward_f32(x, g, b, mean, rstd, ax, 1)
        return NR.forward(x, g, b, ax, 1, EPS)

    def ln_bwd(self, dy, x, g, b, ax):
        if self.f32:
            mean, rstd = NR.stats_f32_two_pass(x, ax, 1, EPS)
            return NR.backward_f32(dy, x, g, mean, rstd, ax, 1)
        return NR.backward(dy, x, g, b, ax, 1, EPS)


class Twin(object):
    """The model on the host.  ``forward`` returns every intermediate by name, ``backward`` every gradient; ``values`` overrides single
    inputs (central differences), ``kept`` the dropout mask (default: the bits of this step's generating call)."""

    def __init__(self, name, step=0):
        self.spec, self.step = VARIANTS[name], step
        self.tab = tables(name)
        self.p = dict(initial(name))
        self.tokens, self.labels = batch(name, step)
        self.kept = kept_bits(self.spec, step)
        self.mask_words = ER.pack_fast(self.kept)

    def forward(self, values=None, kept=None, prec="f64"):
        s, A, tab = self.spec, _Arith(prec), self.tab
        p = dict(self.p, **(values or {}))
        p = {k: A.st(v) for k, v in p.items()}
        ax, kept = ax_of(s), (self.kept if kept is None else kept)
        f = {"p": p, "kept": kept, "prec": prec}
        f["emb"] = XR.embed_fwd_ref(p["table"], self.tokens.reshape(-1)).reshape(T, N, s.C)
        c, h = p["c0"], p["h0"]
        for t in range(T):
            x = f["x%d" % t] = f["emb"][t] if s.axis else np.ascontiguousarray(f["emb"][t].T)
            f["c_in%d" % t], f["h_in%d" % t] = c, h
            a = f["a%d" % t] = A.fprop(tab["x"], x, p["Wx"], s.axis, gate=p["gx"])
            b = f["b%d" % t] = A.fprop(tab["h"], h, p["Wh"], s.axis)
            z = f["z%d" % t] = A.st(a + b)
            c, h = A.st(LR.forward(c, LR.split(z, ax), p["bg"], FB, ax))
            f["c%d" % (t + 1)], f["h%d" % (t + 1)] = c, h
        y = f["y"] = A.st(A.ln_fwd(h, p["g"], p["b"], ax))
        o = f["o"] = A.fprop(tab["o"], y, p["Wo"], s.axis)
        u = f["u"] = A.st(ER.forward(o, p["bo"], ax, 2, kept, ER.scale_of(KEEP), y))
        f["logits"] = A.fprop(tab["l"], u, p["Wl"], s.axis)
        f["rows"] = f["logits"] if s.axis else np.ascontiguousarray(f["logits"].T)
        loss_rows, g, _, _ = XR.xent_ref(f["rows"], self.labels)
        f["loss_rows"], f["xent_g"] = A.st(loss_rows), A.st(g)
        f["loss"] = float(np.asarray(f["loss_rows"], dtype=np.float64).mean())
        return f

    def backward(self, f):
        s, A, tab, p = self.spec, _Arith(f["prec"]), self.tab, f["p"]
        ax, kept = ax_of(s), f["kept"]
        d = {}
        d["rows"] = A.st(f["xent_g"] * (1.0 / N))
        d["logits"] = d["rows"] if s.axis else np.ascontiguousarray(d["rows"].T)
        d["u"] = A.bprop(tab["l"], d["logits"], p["Wl"], s.axis)
        d["Wl"] = A.updat(tab["l"], f["u"], d["logits"], s.axis)
        do, dbo = ER.backward(d["u"], f["o"], p["bo"], ax, 2, kept, ER.scale_of(KEEP))
        d["o"], d["bo"] = A.st(do), A.st(dbo)
        d["Wo"] = A.updat(tab["o"], f["y"], d["o"], s.axis)
        d["y"] = A.st(d["u"] + A.bprop(tab["o"], d["o"], p["Wo"], s.axis))          # the residual's gradient is du itself
        eh, d["g"], d["b"] = A.st(tuple(A.ln_bwd(d["y"], f["h%d" % T], p["g"], p["b"], ax)))
        ec = None
        zero = lambda k: np.zeros(p[k].shape, dtype=A.dt)
        d["Wx"], d["Wx_true"], d["Wh"], d["bg"], d["gx"], d["gx_true"] = zero("Wx"), zero("Wx"), zero("Wh"), zero("bg"), zero("gx"), zero("gx")
        d["emb"] = np.zeros((T, N, s.C), dtype=A.dt)
        for t in reversed(range(T)):
            d["h%d" % (t + 1)], d["c%d" % (t + 1)] = eh, ec
            dc, dgates, dbg = LR.backward(f["c_in%d" % t], LR.split(f["z%d" % t], ax), eh, ec, p["bg"], FB, ax)
            dz = d["z%d" % t] = A.st(LR.fuse(dgates, ax))
            d["bg"] = A.st(d["bg"] + A.st(dbg))
            d["Wh"] = A.st(d["Wh"] + A.updat(tab["h"], f["h_in%d" % t], dz, s.axis))
            raw = A.updat(tab["x"], f["x%d" % t], dz, s.axis)
            gated = A.st(raw * p["gx"][:, None, None])                               # dw_gated: what updat hands to gate_grad
            reg_w, reg_g = orc.gate_grad(gated, p["Wx"], p["gx"])
            d["Wx"], d["gx"] = A.st(d["Wx"] + A.st(reg_w)), A.st(d["gx"] + A.st(reg_g))
            d["Wx_true"] = A.st(d["Wx_true"] + gated)
            d["gx_true"] = A.st(d["gx_true"] + A.st(orc.gate_grad(raw, p["Wx"], p["gx"])[1]))
            dx = d["x%d" % t] = A.bprop(tab["x"], dz, p["Wx"], s.axis, gate=p["gx"])
            d["emb"][t] = dx if s.axis else dx.T
            eh, ec = A.bprop(tab["h"], dz, p["Wh"], s.axis), A.st(dc)
        d["h0"], d["c0"] = eh, ec
        dtab, _ = XR.embed_grad_ref(d["emb"].reshape(T * N, s.C), self.tokens.reshape(-1), V)
        d["table"] = A.st(dtab)
        return d

    # ---- the optimizer step ------------------------------------------------------------------------------------------------------------
    def clip_norm(self, grads):
        """The clip norm that scales these gradients by CLIP_SHARE."""
        return CLIP_SHARE * OR.clip([OR.sum_squared(grads[k]) for k in PARAMS], 9e9)[0]

    def optimizer_step(self, state, grads, clip_norm, step_no, norm_scale=None):
        """One clipped Adam step and the moving averages: _optimize_ref unchanged.  ``state``: {param: (p, m, v, average or None)} of flat
        float64 arrays; returns the new state and (norm, scale).  ``norm_scale``: the device's own scale instead of the computed one."""
        norm, scale = OR.clip([OR.sum_squared(grads[k]) for k in PARAMS], clip_norm)
        lr_t = LRATE * OR.lr_correction_loop(step_no, 0.9, 0.999)
        new = {}
        for k in PARAMS:
            pk, m, v, e = state[k]
            gate, bs = (self.p["gx"], self.spec.bsize) if k == "Wx" else (None, 0)
            pk, m, v = OR.adam(pk, m, v, grads[k], lr_t, gate=gate, bsize=bs, clip_sigma=CLIP_SIGMAS, norm_scale=scale if norm_scale is None else norm_scale)
            e = OR.ema(pk if e is None else e, pk, DECAY, gate, bs)                  # (an average starts as a copy of its param at the first apply)
            new[k] = (pk, m, v, e)
        return new, (norm, scale)

    def fresh_state(self):
        flat = lambda a: np.asarray(a, dtype=np.float64).reshape(-1)
        return {k: (flat(self.p[k]), np.zeros(self.p[k].size), np.zeros(self.p[k].size), None) for k in PARAMS}


def adam_float32(p, m, v, g, lr, gate=None, bsize=0, clip_sigma=0.0, norm_scale=1.0, square_first=False):
    """_optimize_ref.adam (the settings the model uses: no grad scale, no saturation, a sigma clip) with every operation in float32: what
    an fp32 kernel can reach on these inputs.  ``square_first``: (1 - beta2) (g g) instead of the helper's ((1 - beta2) g) g -- the two
    orders in which float32 can take that product.  Flat float32 arrays."""
    f = np.float32
    p, m, v = (np.array(a, dtype=f).reshape(-1) for a in (p, m, v))
    g = np.asarray(g, dtype=f).reshape(-1) * (f(1.0) * f(norm_scale))
    b1, b2, eps = f(0.9), f(0.999), f(1e-8)
    v2 = b2 * v + ((f(1.0) - b2) * (g * g) if square_first else (f(1.0) - b2) * g * g)
    sigma = np.sqrt(v2)
    if clip_sigma != 0.0:
        clip = f(clip_sigma) * sigma
        g = np.minimum(np.maximum(g, -clip), clip)
    m2 = b1 * m + (f(1.0) - b1) * g
    p2 = p - f(lr) * m2 / (sigma + eps)
    assert p2.dtype == f and m2.dtype == f and v2.dtype == f
    live = OR._live(p.size, gate, bsize)
    return np.where(live, p2, p), np.where(live, m2, m), np.where(live, v2, v)


# ---- the device model -------------------------------------------------------------------------------------------------------------------
class DeviceModel(object):
    """The model on the device.  fp32 masters in ``master``; what autograd differentiates is ``leaf``: the optimizer's 16-bit working copies
    (SIXTEEN, 16-bit variants) or the masters themselves.  ``alias=True``: every use of a tied tensor goes through ``w.view_as(w)`` with
    ``retain_grad`` (kept in ``uses``), so that each time step's gradient can be read on its own."""

    def __init__(self, torch, name, alias=False):
        import blocksparse_amd as B
        self.torch, self.B, self.spec, self.alias = torch, B, VARIANTS[name], alias
        s, p = self.spec, initial(name)
        self.dt = getattr(torch, P.TORCH_DT[s.dtype])
        dev = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda().to(dt)
        self.ops = {op: B.BlocksparseMatMul(lay, block_size=s.bsize, feature_axis=s.axis) for op, lay in layouts(name).items()}
        self.master = {k: dev(p[k]) for k in PARAMS}
        self.gx = dev(p["gx"]).requires_grad_()
        self.master["Wx"].gate = self.gx.detach()
        work = None if s.dtype == "f32" else self.dt
        self.opt = B.AdamOptimizer([self.master[k] for k in PARAMS], learning_rate=LRATE, gated=True, clip_sigmas=CLIP_SIGMAS, working_dtype=work)
        self.ema = B.Ema(DECAY, gated=True)
        self.leaf = {k: (self.opt.working_copy(self.master[k]) if (work is not None and k in SIXTEEN) else self.master[k]).requires_grad_()
                     for k in PARAMS}
        self.leaf["gx"] = self.gx
        self.leaf["c0"], self.leaf["h0"] = dev(p["c0"], self.dt).requires_grad_(), dev(p["h0"], self.dt).requires_grad_()
        self.uses = {}

    def leaves(self):
        return [self.leaf[k] for k in PARAMS + EXTRA]

    def _use(self, k, t):
        w = self.leaf[k]
        if not self.alias:
            return w
        v = w.view_as(w)
        v.retain_grad()
        self.uses[(k, t)] = v
        return v

    def forward(self, tokens, labels, mask=None, keep=False):
        """(loss, mask, {name: intermediate}); ``keep``: retain the gradient of every intermediate."""
        B, s, L = self.B, self.spec, self.leaf
        ax, f = ax_of(s), {}

        def note(name, t):
            if keep and t.requires_grad:
                t.retain_grad()
            f[name] = t
            return t
        emb = note("emb", B.embedding_lookup(L["table"], tokens))
        c, h = L["c0"], L["h0"]
        for t in range(T):
            x = note("x%d" % t, emb[t] if s.axis else emb[t].t().contiguous())
            a = note("a%d" % t, self.ops["x"](x, self._use("Wx", t), gate=self._use("gx", t), gate_grad=True, dw_gated=True))
            b = note("b%d" % t, self.ops["h"](h, self._use("Wh", t)))
            z = note("z%d" % t, a + b)
            c, h = B.fused_lstm_gates(c, z, bias=self._use("bg", t), forget_bias=FB, axis=ax)
            note("c%d" % (t + 1), c), note("h%d" % (t + 1), h)
        y = note("y", B.layer_norm(h, L["g"], L["b"], axis=s.axis, epsilon=EPS))
        o = note("o", self.ops["o"](y, L["Wo"]))
        u, mask = B.bias_dropout(o, L["bo"], KEEP, axis=ax, fast_gelu=True, residual=y, mask=mask)
        note("u", u)
        logits = note("logits", self.ops["l"](u, L["Wl"]))
        rows = logits if s.axis else note("rows", logits.t().contiguous())
        loss_rows = note("loss_rows", B.softmax_cross_entropy(logits=rows, labels=labels))
        return note("loss", loss_rows.mean()), mask, f

    def grads(self):
        return [self.leaf[k].grad for k in PARAMS]

    def zero_grad(self):
        for t in self.leaves():
            t.grad = None
        self.uses = {}

    def state(self):
        """Every tensor a step writes, by name."""
        out = {}
        for k in PARAMS:
            m = self.master[k]
            out["p." + k], out["m." + k], out["v." + k] = m, self.opt.get_slot(m, "Mean"), self.opt.get_slot(m, "Var")
            if self.opt.working_copy(m) is not None:
                out["w." + k] = self.opt.working_copy(m)
            if self.ema.average(m) is not None:
                out["e." + k] = self.ema.average(m)
        return out


def build(name, torch=None, step=0, alias=False):
    """(device model or None without torch, twin) of one variant, from the same seeded inputs."""
    return (DeviceModel(torch, name, alias=alias) if torch is not None else None), Twin(name, step)
