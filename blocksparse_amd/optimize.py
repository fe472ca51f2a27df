"""Weight updates that know about gates: Adam, a moving average and the global-norm clip.

The reference's names and arguments (blocksparse/optimize.py:20-110, 193-289) over the C ABI of include/bsmm_optim.h:

    norm, scale = clip_by_global_norm(grads, clip_norm=1.0)        # two device fp32 scalars, no host sync; scale == 0 after an overflow
    adam_step(w, dw, mean, var, lr, gate=gate, norm_scale=scale, param16=w16)
    ema_step(avg, w, 0.999, gate=gate)

    opt = AdamOptimizer([w, bias], learning_rate=3e-4, gated=True, working_dtype=torch.bfloat16)     # reads ``w.gate``
    opt.step(norm_scale=scale)                                     # p.grad by default; opt.working_copy(w) is what the kernels read
    ema = Ema(0.999, gated=True);  ema.apply([w, bias]);  ema.average(w)

A block-sparse tensor is ``[blocks, bsize, bsize]`` with bsize 8 / 16 / 32 / 64; anything else (biases, embeddings) is a flat tensor and
takes neither a gate nor an lr select.  Blocks whose gate is exactly 0 are neither read nor written -- moments, weights, the 16-bit
working copy and the average all keep their bits.  ``lr_select`` (fp32 per block) steps the blocks with a non-zero entry at ``lr_new``:
the blocks ``relayout`` has just added.  A ``norm_scale`` of 0 skips the whole step on the device.

For these per-tensor calls the learning rate is a host scalar: a step captured in a graph replays with the rate (and the step-size
correction) it was captured with.  The list form (include/bsmm_optim_list.h) lifts both limits:

    step = opt.prepare(clip_norm=1.0, ema=ema)                     # binds p, p.grad, slots, gates, averages: one table on the device
    step.learning_rate.fill_(schedule(t))                          # a device fp32 [1]: ordinary device work, inside or outside a graph
    step.run()                                                     # at most 5 launches whatever len(params); capturable

with the step number and the corrected rates on the device, so a captured step follows a schedule.  Its results equal the per-tensor
calls bit for bit.

Adafactor (include/bsmm_adafactor.h), the reference's other optimizer (blocksparse/optimize.py:118-191), with factored second moments:

    adafactor_step(w, dw, cv, rv, lr=5e-4, decay=adafactor_decay(t, 0.999), gate=gate, norm_scale=scale, param16=w16)
    opt = AdafactorOptimizer([w, bias], gated=True, working_dtype=torch.bfloat16);  opt.step(norm_scale=scale)

2-d params keep a row and a column moment, 1-d params one moment per element, block-sparse params a row and a column moment per block
(2 / bsize of Adam's state) with one update rate over the live blocks.  ``lr`` and ``decay`` are host scalars.

Every tensor a call writes gets its version counter bumped (``_lib.wrote``).  PyTorch is plumbing here as everywhere in the package;
there is no CPU fallback.
"""
import ctypes
import math

from . import _lib

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

_BSIZES = (8, 16, 32, 64)
_dtype_code = _lib.require_dtype_code


def _on_device(t, what):
    if torch is None:
        raise RuntimeError("blocksparse_amd needs PyTorch-ROCm for device memory")
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError("blocksparse_amd: %s must be a tensor on a ROCm device (no CPU fallback)" % what)
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)


def _bsize_of(param):
    """Block size of a [blocks, bsize, bsize] tensor; 0 = a flat tensor."""
    if param.dim() == 3 and param.shape[1] == param.shape[2] and param.shape[1] in _BSIZES:
        return int(param.shape[1])
    return 0


def _like(t, ref, what, dtypes=None):
    _on_device(t, what)
    if t.numel() != ref.numel() or t.device != ref.device:
        raise ValueError("%s must have the param's %d elements and device" % (what, ref.numel()))
    if dtypes is not None and t.dtype not in dtypes:
        raise TypeError("%s: unsupported dtype %s" % (what, t.dtype))


def _per_block(t, param, bsize, what):
    if t is None:
        return None
    if bsize == 0:
        raise ValueError("%s needs a [blocks, bsize, bsize] param with bsize in %s, got %s" % (what, _BSIZES, tuple(param.shape)))
    _on_device(t, what)
    if t.dtype != torch.float32 or t.numel() != param.shape[0] or t.device != param.device:
        raise ValueError("%s: expected a contiguous float32 tensor with one entry per block (%d) on the param's device" % (what, param.shape[0]))
    return t.data_ptr()


def _scalar(t, ref, what):
    if t is None:
        return None
    _on_device(t, what)
    if t.dtype != torch.float32 or t.numel() != 1 or t.device != ref.device:
        raise ValueError("%s: expected one float32 on the param's device" % what)
    return t.data_ptr()


def adam_step(param, grad, mean, var, lr, beta1=0.9, beta2=0.999, epsilon=1e-8, grad_scale=1.0, clip_sigma=0.0, saturate=0.0,
              zero_infs=False, zero_nans=False, gate=None, lr_select=None, lr_new=None, norm_scale=None, param16=None):
    """One Adam step in place on ``param`` / ``mean`` / ``var`` (fp32) from ``grad`` (fp32 / fp16 / bf16); returns ``param``.
    ``param16`` (fp16 / bf16) is written in the same pass: ``param`` rounded once.  See include/bsmm_optim.h for the arithmetic."""
    _on_device(param, "param")
    if param.dtype != torch.float32:
        raise TypeError("param must be float32 (the 16-bit copy the kernels read is param16)")
    bsize = _bsize_of(param)
    _like(grad, param, "grad")
    _like(mean, param, "mean", (torch.float32,))
    _like(var, param, "var", (torch.float32,))
    if param16 is not None:
        _like(param16, param, "param16", (torch.float16, torch.bfloat16))
    if lr_select is not None and lr_new is None:
        raise ValueError("lr_select needs lr_new")
    a = _lib.BsmmAdamArgs()
    a.param, a.mean, a.var, a.grad = param.data_ptr(), mean.data_ptr(), var.data_ptr(), grad.data_ptr()
    a.param16 = param16.data_ptr() if param16 is not None else None
    a.gate = _per_block(gate, param, bsize, "gate")
    a.lr_select = _per_block(lr_select, param, bsize, "lr_select")
    a.norm_scale = _scalar(norm_scale, param, "norm_scale")
    a.stream = _lib.raw_stream(param.device)
    a.size, a.bsize = param.numel(), bsize
    a.grad_dtype = _dtype_code(grad.dtype)
    a.param16_dtype = _dtype_code(param16.dtype) if param16 is not None else 0
    a.zero_infs, a.zero_nans = int(bool(zero_infs)), int(bool(zero_nans))
    a.lr, a.lr_new = float(lr), float(lr_new if lr_new is not None else lr)
    a.beta1, a.beta2, a.epsilon = float(beta1), float(beta2), float(epsilon)
    a.grad_scale, a.clip_sigma, a.saturate = float(grad_scale), float(clip_sigma), float(saturate)
    _lib.check(_lib.load().bsmm_adam(ctypes.byref(a)), "bsmm_adam")
    _lib.wrote(param, mean, var, param16)
    return param


def ema_step(ema, param, decay, gate=None):
    """``ema -= (1 - decay) * (ema - param)`` in place (``ema``: fp32 / fp16 / bf16, ``param``: fp32); returns ``ema``."""
    _on_device(param, "param")
    if param.dtype != torch.float32:
        raise TypeError("param must be float32")
    bsize = _bsize_of(param)
    _like(ema, param, "ema")
    _lib.check(_lib.load().bsmm_ema(ema.data_ptr(), param.data_ptr(), _per_block(gate, param, bsize, "gate"), float(decay), param.numel(), bsize,
                                    _dtype_code(ema.dtype), _lib.raw_stream(param.device)), "bsmm_ema")
    _lib.wrote(ema)
    return ema


def clip_by_global_norm(grads, clip_norm=1.0, grad_scale=1.0, saturate=0.0, zero_infs=False, zero_nans=False):
    """``(global_norm, norm_scale)`` of a list of gradients (mixed dtypes allowed): two device fp32 scalars, no host sync.
    ``global_norm = sqrt(sum (grad_scale * g)^2)``; ``norm_scale = clip_norm / max(global_norm, clip_norm)``, or 0 when the norm is not
    finite -- the value that makes ``adam_step`` skip.  Deterministic: the same gradients at the same addresses give the same bits."""
    grads = list(grads)
    if not grads:
        raise ValueError("clip_by_global_norm needs at least one gradient")
    for g in grads:
        _on_device(g, "grad")
        if g.device != grads[0].device:
            raise ValueError("all gradients must be on one device")
        if g.numel() == 0:
            raise ValueError("empty gradient")
    lib = _lib.load()
    dev = grads[0].device
    cnt = len(grads)
    need = int(lib.bsmm_sum_squared_workspace_bytes(cnt))
    ws = torch.empty(need // 4, dtype=torch.float32, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    st = _lib.raw_stream(dev)
    for i, g in enumerate(grads):
        _lib.check(lib.bsmm_sum_squared(g.data_ptr(), g.numel(), _dtype_code(g.dtype), float(grad_scale), float(saturate), int(bool(zero_infs)),
                                        int(bool(zero_nans)), i, cnt, ws.data_ptr(), need, st), "bsmm_sum_squared")
    _lib.check(lib.bsmm_clip_norm(ws.data_ptr(), need, cnt, float(clip_norm), out.data_ptr(), out.data_ptr() + 4, st), "bsmm_clip_norm")
    return out[0], out[1]


def global_norm(grads, grad_scale=1.0, saturate=0.0, zero_infs=False, zero_nans=False):
    """The global norm alone (blocksparse/optimize.py:222-224)."""
    return clip_by_global_norm(grads, clip_norm=9e9, grad_scale=grad_scale, saturate=saturate, zero_infs=zero_infs, zero_nans=zero_nans)[0]


def lr_correction(step, beta1, beta2, zero_init_variables=False):
    """``sqrt(1 - beta2^t) / (1 - beta1^t)`` for call number ``step`` (1, 2, ...): the reference's beta-power accumulators start at beta and
    are multiplied by beta after every call (blocksparse/optimize.py:45-57, 104-110).  With ``zero_init_variables`` they start at 0 and
    stay there: no correction, the setting for moments that are loaded rather than grown from zero."""
    if zero_init_variables:
        return 1.0
    t = max(int(step), 1)
    return math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


class AdamOptimizer(object):
    """Adam over a list of fp32 tensors (block-sparse or flat) with fp32 ``Mean`` / ``Var`` slots.  ``gated=True`` reads ``param.gate``.
    ``working_dtype``: keep a 16-bit copy of every param, rewritten by the step itself (``working_copy(param)``)."""

    def __init__(self, params, learning_rate=3e-4, beta1=0.9, beta2=0.999, epsilon=1e-8, clip_sigmas=0.0, norm_scale=None, grad_scale=1.0,
                 saturate=0.0, zero_infs=False, zero_nans=False, gated=False, zero_init_variables=False, working_dtype=None):
        self.params = list(params)
        if not self.params:
            raise ValueError("AdamOptimizer needs at least one param")
        self.learning_rate, self.beta1, self.beta2, self.epsilon = float(learning_rate), float(beta1), float(beta2), float(epsilon)
        self.clip_sigmas, self.grad_scale, self.saturate = float(clip_sigmas), float(grad_scale), float(saturate)
        self.zero_infs, self.zero_nans, self.gated, self.zero_init_variables = bool(zero_infs), bool(zero_nans), bool(gated), bool(zero_init_variables)
        self.norm_scale = norm_scale
        self.working_dtype = working_dtype
        self.steps = 0
        self.slots = []
        for p in self.params:
            _on_device(p, "param")
            if p.dtype != torch.float32:
                raise TypeError("AdamOptimizer keeps fp32 params (working_dtype gives the 16-bit copies)")
            d = p.detach()
            slot = {"Mean": torch.zeros_like(d), "Var": torch.zeros_like(d)}
            if working_dtype is not None:
                slot["working"] = d.to(working_dtype)
            self.slots.append(slot)

    def _index(self, param):
        for i, p in enumerate(self.params):
            if p is param:
                return i
        raise KeyError("not a param of this optimizer")

    def get_slot(self, param, name):
        """The ``"Mean"`` or ``"Var"`` tensor of ``param``."""
        return self.slots[self._index(param)][name]

    def working_copy(self, param):
        """The 16-bit copy of ``param`` (``None`` without ``working_dtype``)."""
        return self.slots[self._index(param)].get("working")

    def current_lr(self, learning_rate=None):
        """The corrected step size of the most recent call of ``step``."""
        lr = self.learning_rate if learning_rate is None else float(learning_rate)
        return lr * lr_correction(self.steps, self.beta1, self.beta2, self.zero_init_variables)

    def step(self, grads=None, lr_select=None, lr_new=None, norm_scale=None):
        """One step for every param.  ``grads``: a list parallel to the params (default: ``p.grad``; params without one are left out).
        ``lr_select``: a list parallel to the params (``None`` entries allowed) or a dict ``{param index: tensor}``; ``lr_new``: the rate
        of the selected blocks, corrected like the learning rate.  ``norm_scale`` overrides the constructor's.  The step counter advances on
        every call, also when the device skips the step."""
        self.steps += 1
        lr = self.current_lr()
        lr_new_t = self.current_lr(lr_new) if lr_new is not None else None
        ns = norm_scale if norm_scale is not None else self.norm_scale
        if grads is None:
            grads = [p.grad for p in self.params]
        grads = list(grads)
        if len(grads) != len(self.params):
            raise ValueError("need one gradient (or None) per param")
        for i, (p, g) in enumerate(zip(self.params, grads)):
            if g is None:
                continue
            sel = lr_select.get(i) if isinstance(lr_select, dict) else (lr_select[i] if lr_select is not None else None)
            gate = getattr(p, "gate", None) if self.gated else None
            slot = self.slots[i]
            adam_step(p.detach(), g.detach(), slot["Mean"], slot["Var"], lr, beta1=self.beta1, beta2=self.beta2, epsilon=self.epsilon,
                      grad_scale=self.grad_scale, clip_sigma=self.clip_sigmas, saturate=self.saturate, zero_infs=self.zero_infs,
                      zero_nans=self.zero_nans, gate=gate, lr_select=sel, lr_new=lr_new_t if sel is not None else None, norm_scale=ns,
                      param16=slot.get("working"))

    def prepare(self, grads=None, clip_norm=None, ema=None, lr_select=None, lr_new=None, ema_params=None):
        """Bind every tensor of the update once and return a ``PreparedStep`` whose ``run()`` is [sum of squares, clip,] advance, Adam
        [, moving average]: one launch per stage over all params.  ``grads``: a list parallel to the params (default ``p.grad``; every
        param must have one).  ``clip_norm``: clip by the global norm of the grads first (else the constructor's ``norm_scale``, if any,
        scales them).  ``ema``: an ``Ema`` whose averages follow the step (created as ``Ema.apply`` creates them; ``ema_params``
        restricts them to some of the params).  ``lr_select``: a list or dict as in ``step`` (``None`` entries allowed), with ``lr_new``."""
        return PreparedStep(self, grads, clip_norm, ema, lr_select, lr_new, ema_params)

    def state_dict(self):
        return {"steps": self.steps, "slots": [{"Mean": s["Mean"].clone(), "Var": s["Var"].clone()} for s in self.slots]}

    def load_state_dict(self, state):
        if len(state["slots"]) != len(self.slots):
            raise ValueError("state has %d slots, the optimizer %d params" % (len(state["slots"]), len(self.slots)))
        for s, new in zip(self.slots, state["slots"]):
            s["Mean"].copy_(new["Mean"])
            s["Var"].copy_(new["Var"])
        self.steps = int(state["steps"])
        for p, s in zip(self.params, self.slots):          # the working copies follow the params the caller has loaded
            if "working" in s:
                s["working"].copy_(p.detach())


def adafactor_step(param, grad, cv, rv=None, lr=5e-4, decay=0.999, epsilon=1e-30, clip_thresh=1.0, grad_scale=1.0, saturate=0.0,
                   zero_infs=False, zero_nans=False, gate=None, norm_scale=None, param16=None):
    """One Adafactor step in place on ``param`` (fp32) and its factored second moments from ``grad`` (fp32 / fp16 / bf16); returns
    ``param``.  The form follows the param's shape: ``[C, K]`` with C > 1 takes ``rv`` [C] and ``cv`` [K]; ``[K]`` or ``[1, K]`` takes
    ``cv`` [K] alone; ``[blocks, bsize, bsize]`` takes ``rv`` and ``cv`` [blocks, bsize] and, optionally, a ``gate``.  ``decay`` is the
    value of ``adafactor_decay`` for this call.  See include/bsmm_adafactor.h for the arithmetic and the order of every sum."""
    _on_device(param, "param")
    if param.dtype != torch.float32:
        raise TypeError("param must be float32 (the 16-bit copy the kernels read is param16)")
    bsize = _bsize_of(param)
    if bsize:
        rows, cols, nrv, ncv = param.shape[0], bsize * bsize, param.shape[0] * bsize, param.shape[0] * bsize
    elif param.dim() == 2 and param.shape[0] > 1:
        rows, cols, nrv, ncv = param.shape[0], param.shape[1], param.shape[0], param.shape[1]
    elif param.dim() == 1 or (param.dim() == 2 and param.shape[0] == 1):
        rows, cols, nrv, ncv = 1, param.numel(), 0, param.numel()
    else:
        raise ValueError("only 1 or 2d params are supported")
    if rows == 0 or cols == 0:
        raise ValueError("empty param")
    _like(grad, param, "grad")
    for t, n, what in ((cv, ncv, "cv"), (rv, nrv, "rv")):
        if n == 0 and t is None:
            continue
        if t is None:
            raise ValueError("this form needs %s" % what)
        _on_device(t, what)
        if t.dtype != torch.float32 or t.device != param.device or (n and t.numel() != n):
            raise ValueError("%s: expected a contiguous float32 tensor of %d elements on the param's device" % (what, n))
    if param16 is not None:
        _like(param16, param, "param16", (torch.float16, torch.bfloat16))
    lib = _lib.load()
    need = int(lib.bsmm_adafactor_workspace_bytes(rows, cols, bsize))
    ws = torch.empty(need // 4, dtype=torch.float32, device=param.device)
    a = _lib.BsmmAdafactorArgs()
    a.param, a.cv, a.grad = param.data_ptr(), cv.data_ptr(), grad.data_ptr()
    a.rv = rv.data_ptr() if rv is not None and nrv else None
    a.param16 = param16.data_ptr() if param16 is not None else None
    a.gate = _per_block(gate, param, bsize, "gate")
    a.norm_scale = _scalar(norm_scale, param, "norm_scale")
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    a.stream = _lib.raw_stream(param.device)
    a.rows, a.cols, a.bsize = rows, cols, bsize
    a.grad_dtype = _dtype_code(grad.dtype)
    a.param16_dtype = _dtype_code(param16.dtype) if param16 is not None else 0
    a.zero_infs, a.zero_nans = int(bool(zero_infs)), int(bool(zero_nans))
    a.lr, a.decay, a.epsilon, a.clip_thresh = float(lr), float(decay), float(epsilon), float(clip_thresh)
    a.grad_scale, a.saturate = float(grad_scale), float(saturate)
    _lib.check(lib.bsmm_adafactor(ctypes.byref(a)), "bsmm_adafactor")
    _lib.wrote(param, cv, rv if nrv else None, param16)
    return param


def adafactor_decay(step, beta2, zero_init_variables=False):
    """The moments' decay for call number ``step`` (1, 2, ...): ``beta2 (1 - beta2^t) / (1 - beta2^(2t))`` from the two accumulators
    ``decay1_power = beta2^t`` and ``decay2_power = beta2^(2t)`` (blocksparse/optimize.py:131-142).  With ``zero_init_variables`` both
    start at 0 and stay there: the decay is ``beta2``, the setting for moments that are loaded rather than grown from zero."""
    if zero_init_variables:
        return float(beta2)
    t = max(int(step), 1)
    return beta2 * (1.0 - beta2 ** t) / (1.0 - beta2 ** (2 * t))


class AdafactorOptimizer(object):
    """Adafactor over a list of fp32 tensors with fp32 ``cv`` / ``rv`` slots (zeros at the start): 2-d params with more than one row
    keep a row and a column moment, 1-d and ``(1, K)`` params one moment per element, ``[blocks, bsize, bsize]`` params a row and a
    column moment per block; anything else raises, as the reference does.  ``gated=True`` reads ``param.gate``.  ``working_dtype``:
    keep a 16-bit copy of every param, rewritten by the step itself (``working_copy(param)``).  The learning rate and the decay are host
    scalars: a captured step replays with the values it was captured with."""

    def __init__(self, params, learning_rate=5e-4, beta2=0.999, epsilon=1e-30, clip_thresh=1.0, norm_scale=None, grad_scale=1.0, saturate=0.0,
                 zero_infs=False, zero_nans=False, zero_init_variables=False, gated=False, working_dtype=None):
        self.params = list(params)
        if not self.params:
            raise ValueError("AdafactorOptimizer needs at least one param")
        self.learning_rate, self.beta2, self.epsilon, self.clip_thresh = float(learning_rate), float(beta2), float(epsilon), float(clip_thresh)
        self.grad_scale, self.saturate = float(grad_scale), float(saturate)
        self.zero_infs, self.zero_nans, self.gated, self.zero_init_variables = bool(zero_infs), bool(zero_nans), bool(gated), bool(zero_init_variables)
        self.norm_scale = norm_scale
        self.working_dtype = working_dtype
        self.steps = 0
        self.slots = []
        for p in self.params:
            _on_device(p, "param")
            if p.dtype != torch.float32:
                raise TypeError("AdafactorOptimizer keeps fp32 params (working_dtype gives the 16-bit copies)")
            d = p.detach()
            bsize = _bsize_of(d)
            zeros = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=d.device)
            if bsize:
                slot = {"cv": zeros(d.shape[0], bsize), "rv": zeros(d.shape[0], bsize)}
            elif d.dim() == 2 and d.shape[0] > 1:
                slot = {"cv": zeros(d.shape[1]), "rv": zeros(d.shape[0])}
            elif d.dim() == 1 or (d.dim() == 2 and d.shape[0] == 1):
                slot = {"cv": zeros(d.numel())}
            else:
                raise ValueError("only 1 or 2d params are supported")
            if working_dtype is not None:
                slot["working"] = d.to(working_dtype)
            self.slots.append(slot)

    def _index(self, param):
        for i, p in enumerate(self.params):
            if p is param:
                return i
        raise KeyError("not a param of this optimizer")

    def get_slot(self, param, name):
        """The ``"cv"`` or ``"rv"`` tensor of ``param`` (``None``: the 1-d form keeps no ``rv``)."""
        return self.slots[self._index(param)].get(name)

    def working_copy(self, param):
        """The 16-bit copy of ``param`` (``None`` without ``working_dtype``)."""
        return self.slots[self._index(param)].get("working")

    def current_decay(self):
        """The decay of the most recent call of ``step``."""
        return adafactor_decay(self.steps, self.beta2, self.zero_init_variables)

    def step(self, grads=None, norm_scale=None):
        """One step for every param.  ``grads``: a list parallel to the params (default: ``p.grad``; params without one are left out).
        ``norm_scale`` overrides the constructor's.  The step counter advances on every call, also when the device skips the step."""
        self.steps += 1
        decay = self.current_decay()
        ns = norm_scale if norm_scale is not None else self.norm_scale
        if grads is None:
            grads = [p.grad for p in self.params]
        grads = list(grads)
        if len(grads) != len(self.params):
            raise ValueError("need one gradient (or None) per param")
        for p, g, slot in zip(self.params, grads, self.slots):
            if g is None:
                continue
            gate = getattr(p, "gate", None) if self.gated and _bsize_of(p) else None
            adafactor_step(p.detach(), g.detach(), slot["cv"], slot.get("rv"), lr=self.learning_rate, decay=decay, epsilon=self.epsilon,
                           clip_thresh=self.clip_thresh, grad_scale=self.grad_scale, saturate=self.saturate, zero_infs=self.zero_infs,
                           zero_nans=self.zero_nans, gate=gate, norm_scale=ns, param16=slot.get("working"))

    def state_dict(self):
        return {"steps": self.steps, "slots": [{k: s[k].clone() for k in ("cv", "rv") if k in s} for s in self.slots]}

    def load_state_dict(self, state):
        if len(state["slots"]) != len(self.slots):
            raise ValueError("state has %d slots, the optimizer %d params" % (len(state["slots"]), len(self.slots)))
        for s, new in zip(self.slots, state["slots"]):
            for k in ("cv", "rv"):
                if k in s:
                    s[k].copy_(new[k])
        self.steps = int(state["steps"])
        for p, s in zip(self.params, self.slots):          # the working copies follow the params the caller has loaded
            if "working" in s:
                s["working"].copy_(p.detach())


class PreparedStep(object):
    """The list form of one optimizer step (``AdamOptimizer.prepare``): the tensors are bound once, in a table on the device, and every
    stage walks the table in one launch.  The step number and the corrected rates live on the device:

        learning_rate   device fp32 [1], starts at ``opt.learning_rate``; write it with ``fill_`` / ``copy_`` (a schedule)
        lr_new          device fp32 [1], or None without ``lr_new``
        global_norm, norm_scale   device scalars of the last run (None without ``clip_norm``)
        rates()         device fp32 [2]: the corrected ``lr_t, lr_new_t`` of the last run
        sync_host()     reads the device step count into ``opt.steps`` -- the one host sync; needed before ``state_dict()`` after replays

    The table holds addresses: ``run()`` refuses to launch when a bound tensor has moved (``p.grad`` reallocated -- keep it with
    ``zero_grad(set_to_none=False)``).  Results equal those of the per-tensor calls bit for bit."""

    def __init__(self, opt, grads, clip_norm, ema, lr_select, lr_new, ema_params):
        self.opt = opt
        params = opt.params
        dev = params[0].device
        if grads is not None:
            grads = list(grads)
            if len(grads) != len(params):
                raise ValueError("need one gradient per param")
        if lr_select is not None and lr_new is None:
            raise ValueError("lr_select needs lr_new")
        if ema is not None and ema.gated != opt.gated:
            raise ValueError("the list step reads one gate per param: Ema.gated and AdamOptimizer.gated must agree")
        if ema_params is not None and ema is None:
            raise ValueError("ema_params needs ema")
        averaged = None if ema_params is None else set(id(p) for p in ema_params)
        self._bound = []                                    # (what, how to find the tensor now, its address, type and size when bound)
        self._held = []                                     # every bound tensor stays alive as long as the table does
        self._written = []

        def bind(what, get):
            t = get()
            self._bound.append((what, get, (t.data_ptr(), t.dtype, t.numel())))
            self._held.append(t)
            return t.data_ptr()

        rows = (_lib.BsmmOptTensor * len(params))()
        for i, p in enumerate(params):
            if p.device != dev:
                raise ValueError("all params must be on one device")
            d = p.detach()
            bsize = _bsize_of(d)
            if grads is None:
                if p.grad is None:
                    raise ValueError("param %d has no grad: every param of a prepared step needs one" % i)
                g = p.grad
                get_grad = lambda p=p: p.grad
            else:
                g = grads[i]
                if g is None:
                    raise ValueError("param %d has no grad: every param of a prepared step needs one" % i)
                g = g.detach()
                get_grad = lambda g=g: g
            _like(g, d, "grad")
            slot = opt.slots[i]
            _like(slot["Mean"], d, "mean", (torch.float32,))
            _like(slot["Var"], d, "var", (torch.float32,))
            r = rows[i]
            r.param = bind("param %d" % i, lambda p=p: p)
            r.grad = bind("the grad of param %d" % i, get_grad)
            r.mean = bind("Mean of param %d" % i, lambda slot=slot: slot["Mean"])
            r.var = bind("Var of param %d" % i, lambda slot=slot: slot["Var"])
            self._written += [d, slot["Mean"], slot["Var"]]
            self._held.append(d)
            r.size, r.bsize, r.grad_dtype = d.numel(), bsize, _dtype_code(g.dtype)
            work = slot.get("working")
            if work is not None:
                _like(work, d, "param16", (torch.float16, torch.bfloat16))
                r.param16 = bind("the working copy of param %d" % i, lambda slot=slot: slot["working"])
                r.param16_dtype = _dtype_code(work.dtype)
                self._written.append(work)
            gate = getattr(p, "gate", None) if opt.gated else None
            if gate is not None:
                _per_block(gate, d, bsize, "gate")
                r.gate = bind("the gate of param %d" % i, lambda p=p: p.gate)
            sel = lr_select.get(i) if isinstance(lr_select, dict) else (lr_select[i] if lr_select is not None else None)
            if sel is not None:
                _per_block(sel, d, bsize, "lr_select")
                r.lr_select = bind("lr_select of param %d" % i, lambda sel=sel: sel)
            if ema is not None and (averaged is None or id(p) in averaged):
                ent = ema.averages.get(id(p))
                if ent is None:
                    ent = ema.averages[id(p)] = (p, d.to(ema.dtype or torch.float32, copy=True))
                _like(ent[1], d, "ema")
                r.ema = bind("the average of param %d" % i, lambda ema=ema, p=p: ema.averages[id(p)][1])
                r.ema_dtype = _dtype_code(ent[1].dtype)
                self._written.append(ent[1])
        lib = _lib.load()
        self._info = _lib.BsmmOptList()
        nbytes = int(lib.bsmm_opt_list_bytes(len(params)))
        host = (ctypes.c_ubyte * max(nbytes, 1))()
        _lib.check(lib.bsmm_opt_list_build(rows, len(params), host, nbytes, ctypes.byref(self._info)), "bsmm_opt_list_build")
        self._table = torch.frombuffer(host, dtype=torch.uint8, count=nbytes).to(dev)
        assert self._table.data_ptr() % 16 == 0
        self._state = torch.zeros(4, dtype=torch.int32, device=dev)
        self._state[0] = opt.steps
        self._steps = opt.steps                             # the host count the device state was last level with
        self.learning_rate = torch.full((1,), opt.learning_rate, dtype=torch.float32, device=dev)
        self.lr_new = torch.full((1,), float(lr_new), dtype=torch.float32, device=dev) if lr_new is not None else None
        self.ema = ema
        self.clip_norm = None if clip_norm is None else float(clip_norm)
        self.global_norm = self.norm_scale = None
        self._ns = _scalar(opt.norm_scale, params[0], "norm_scale")
        if opt.norm_scale is not None:
            self._held.append(opt.norm_scale)
        if clip_norm is not None:
            self._ws_bytes = int(lib.bsmm_sum_squared_workspace_bytes(len(params)))
            self._ws = torch.empty(self._ws_bytes // 4, dtype=torch.float32, device=dev)
            out = torch.zeros(2, dtype=torch.float32, device=dev)
            self.global_norm, self.norm_scale = out[0], out[1]
            self._ns = out.data_ptr() + 4
        self._settings = s = _lib.BsmmAdamSettings()
        s.beta1, s.beta2, s.epsilon, s.grad_scale, s.clip_sigma, s.saturate = opt.beta1, opt.beta2, opt.epsilon, opt.grad_scale, opt.clip_sigmas, opt.saturate
        s.zero_infs, s.zero_nans = int(opt.zero_infs), int(opt.zero_nans)
        self._device = dev

    def rates(self):
        """Device fp32 [2]: the corrected rates ``lr_t, lr_new_t`` the last run stepped with (a view of the device state)."""
        return self._state[1:3].view(torch.float32)

    def sync_host(self):
        """Read the device step count into ``opt.steps`` (a host sync) and return it."""
        self.opt.steps = self._steps = int(self._state[0].item())
        return self.opt.steps

    def _check_bound(self):
        for what, get, was in self._bound:
            t = get()
            if t is None or (t.data_ptr(), t.dtype, t.numel()) != was:          # (the allocator may hand a new tensor the old address)
                raise ValueError("%s has moved since prepare(): the table holds its old address.  Keep gradients in place with "
                                 "zero_grad(set_to_none=False) (or copy_ into them), or prepare() again" % what)

    def run(self):
        """One step: [sum of squares, clip,] advance, Adam [, moving average].  Only enqueues; capturable.  The device owns the step count:
        a replay advances it without the host seeing it, so after replays ``opt.steps`` is behind until ``sync_host()`` (an eager run does
        not catch it up; it only levels the device with a count the host has SET since, as ``load_state_dict`` does)."""
        opt, lib, info = self.opt, _lib.load(), ctypes.byref(self._info)
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self._check_bound()
            if opt.steps != self._steps:                    # the host count was set since (load_state_dict): level the device with it
                self._state[0] = opt.steps
        st, table, state = _lib.raw_stream(self._device), self._table.data_ptr(), self._state.data_ptr()
        if self.clip_norm is not None:
            _lib.check(lib.bsmm_sum_squared_list(info, table, opt.grad_scale, opt.saturate, int(opt.zero_infs), int(opt.zero_nans),
                                                 self._ws.data_ptr(), self._ws_bytes, st), "bsmm_sum_squared_list")
            _lib.check(lib.bsmm_clip_norm(self._ws.data_ptr(), self._ws_bytes, self._info.count, self.clip_norm, self.global_norm.data_ptr(),
                                          self.norm_scale.data_ptr(), st), "bsmm_clip_norm")
        _lib.check(lib.bsmm_opt_advance(state, self.learning_rate.data_ptr(), self.lr_new.data_ptr() if self.lr_new is not None else None,
                                        opt.beta1, opt.beta2, int(opt.zero_init_variables), st), "bsmm_opt_advance")
        _lib.check(lib.bsmm_adam_list(info, table, state, self._ns, ctypes.byref(self._settings), st), "bsmm_adam_list")
        if self.ema is not None:
            _lib.check(lib.bsmm_ema_list(info, table, self.ema.decay, st), "bsmm_ema_list")
        _lib.wrote(*self._written)
        if not capturing:
            opt.steps += 1
            self._steps = opt.steps


class Ema(object):
    """Moving averages of a set of params (blocksparse/optimize.py:235-289).  ``apply(params)`` updates them (an average starts as a copy
    of its param), ``average(param)`` returns one.  ``gated=True`` reads ``param.gate``; ``dtype``: storage type of the averages (fp32)."""

    def __init__(self, decay=0.999, gated=False, dtype=None):
        self.decay, self.gated, self.dtype = float(decay), bool(gated), dtype
        self.averages = {}                                  # id(param) -> (param, average): the param is held so that its id stays its own

    def apply(self, params):
        for p in params:
            _on_device(p, "param")
            ent = self.averages.get(id(p))
            if ent is None:
                ent = self.averages[id(p)] = (p, p.detach().to(self.dtype or torch.float32, copy=True))
            gate = getattr(p, "gate", None) if self.gated else None
            ema_step(ent[1], p.detach(), self.decay, gate=gate)

    def average(self, param):
        ent = self.averages.get(id(param))
        return ent[1] if ent is not None else None
