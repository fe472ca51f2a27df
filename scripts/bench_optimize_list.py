"""Times the tensor-list form of the weight update (include/bsmm_optim_list.h, ``AdamOptimizer.prepare``) against the per-tensor calls
(include/bsmm_optim.h) and writes a markdown table.

    python scripts/bench_optimize_list.py --out profiles/optimize_list_bench.md

1. T = 1 at the headline weight shape (4096 x 4096, block size 32, density 20 %, bf16 gradients, bf16 working copy): ``bsmm_adam_list`` /
   ``bsmm_ema_list`` / ``bsmm_sum_squared_list`` against ``bsmm_adam`` / ``bsmm_ema`` / ``bsmm_sum_squared``, all through the C ABI so that the
   kernels are compared and not the Python around them.  The list form adds one table read per workgroup and nothing per element, so it is
   accepted when its time is no worse than the per-tensor time plus the measured noise of the per-tensor time.
2. A 48-tensor model -- 12 x [one 1024 x 1024 block-size-32 weight at 20 %, one bias of 1024, two flat tensors of 1024] -- clip + Adam +
   moving average: the per-tensor sequence (145 launches) against ``step.run()`` (5), eager and as graph replays.  Accepted when the list
   form is faster by more than the noise in both modes; the ratio is recorded.

Timing: device events around ``--calls`` (>= 200) back-to-back calls after a warm-up of every shape; a *repeat* is the median of
``--windows`` such timings; every comparison takes ``--repeats`` (5) repeats of each form, the two forms alternating in one process.
Noise = max - min of the per-tensor form's repeats.  A measurement path that finds no GPU fails."""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _window(torch, fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls                 # us per call


def compare(torch, old, new, calls, windows, repeats):
    """Repeats (us per call) of the two forms, alternating; returns (old repeats, new repeats)."""
    for fn in (old, new):
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    out = ([], [])
    for _ in range(repeats):
        for k, fn in enumerate((old, new)):
            out[k].append(statistics.median(_window(torch, fn, calls) for _ in range(windows)))
    return out


def verdict(old, new, want_faster):
    med_old, med_new, noise = statistics.median(old), statistics.median(new), max(old) - min(old)
    ok = med_new < med_old - noise if want_faster else med_new <= med_old + noise
    return med_old, med_new, noise, ok


def headline(torch, lib, args):
    """T = 1 through the C ABI; returns [(stage, per-tensor repeats, list repeats)]."""
    import numpy as np
    L = lib.load()
    hidden, bs, density = 4096, 32, 0.20
    blocks = int((np.random.default_rng(1234).random((hidden // bs, hidden // bs)) < density).sum())      # the layout bench.py times
    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda scale: torch.randn((blocks, bs, bs), device="cuda", generator=gen) * scale
    p, g = rnd(0.01), rnd(0.1).to(torch.bfloat16)
    m, v, e, p16 = torch.zeros_like(p), torch.zeros_like(p), p.clone(), p.to(torch.bfloat16)
    n = p.numel()
    st = lib.raw_stream(p.device)
    rows = (lib.BsmmOptTensor * 1)()
    r = rows[0]
    r.param, r.mean, r.var, r.grad, r.param16, r.ema = (t.data_ptr() for t in (p, m, v, g, p16, e))
    r.size, r.bsize, r.grad_dtype, r.param16_dtype, r.ema_dtype = n, bs, lib.BF16, lib.BF16, lib.F32
    info = lib.BsmmOptList()
    nbytes = int(L.bsmm_opt_list_bytes(1))
    host = (ctypes.c_ubyte * nbytes)()
    lib.check(L.bsmm_opt_list_build(rows, 1, host, nbytes, ctypes.byref(info)), "bsmm_opt_list_build")
    table = torch.frombuffer(host, dtype=torch.uint8, count=nbytes).cuda()
    state = torch.zeros(4, dtype=torch.int32, device="cuda")
    lr = torch.full((1,), 3e-4, device="cuda")
    lib.check(L.bsmm_opt_advance(state.data_ptr(), lr.data_ptr(), None, 0.9, 0.999, 0, st), "bsmm_opt_advance")
    lr_t = float(state[1:2].view(torch.float32))
    s = lib.BsmmAdamSettings()
    s.beta1, s.beta2, s.epsilon, s.grad_scale = 0.9, 0.999, 1e-8, 1.0
    a = lib.BsmmAdamArgs()
    a.param, a.mean, a.var, a.grad, a.param16, a.stream = p.data_ptr(), m.data_ptr(), v.data_ptr(), g.data_ptr(), p16.data_ptr(), st
    a.size, a.bsize, a.grad_dtype, a.param16_dtype = n, bs, lib.BF16, lib.BF16
    a.lr, a.beta1, a.beta2, a.epsilon, a.grad_scale = lr_t, 0.9, 0.999, 1e-8, 1.0
    need = int(L.bsmm_sum_squared_workspace_bytes(1))
    ws = torch.empty(need // 4, device="cuda")
    pa, pi, ps = ctypes.byref(a), ctypes.byref(info), ctypes.byref(s)
    tp, sp, wp, ep, pp, gp = table.data_ptr(), state.data_ptr(), ws.data_ptr(), e.data_ptr(), p.data_ptr(), g.data_ptr()
    forms = [("adam", lambda: L.bsmm_adam(pa), lambda: L.bsmm_adam_list(pi, tp, sp, None, ps, st)),
             ("ema", lambda: L.bsmm_ema(ep, pp, None, 0.999, n, bs, lib.F32, st), lambda: L.bsmm_ema_list(pi, tp, 0.999, st)),
             ("sum of squares", lambda: L.bsmm_sum_squared(gp, n, lib.BF16, 1.0, 0.0, 0, 0, 0, 1, wp, need, st),
              lambda: L.bsmm_sum_squared_list(pi, tp, 1.0, 0.0, 0, 0, wp, need, st))]
    out = []
    for name, old, new in forms:
        assert old() == 0 and new() == 0, name
        out.append((name,) + compare(torch, old, new, args.calls, args.windows, args.repeats))
    shape = "%d x %d, bsize %d, %d blocks (%.2f M elements), bf16 gradient, bf16 working copy" % (hidden, hidden, bs, blocks, n / 1e6)
    return shape, out


def model(torch, lib, args):
    """The 48-tensor model through the Python surface; returns (launch counts, [(mode, per-tensor repeats, list repeats)])."""
    import numpy as np
    from blocksparse_amd import AdamOptimizer, Ema, adam_step, clip_by_global_norm, ema_step, optimize
    gen = torch.Generator(device="cuda").manual_seed(2)
    blocks = int((np.random.default_rng(7).random((32, 32)) < 0.20).sum())
    shapes = []
    for _ in range(12):
        shapes += [(blocks, 32, 32), (1024,), (1024,), (1024,)]

    def build():
        params = [torch.randn(s, device="cuda", generator=gen) * 0.01 for s in shapes]
        grads = [(torch.randn(s, device="cuda", generator=gen) * 0.1).to(torch.bfloat16 if len(s) == 3 else torch.float32) for s in shapes]
        opt = AdamOptimizer(params, learning_rate=3e-4, working_dtype=torch.bfloat16)
        ema = Ema(0.999)
        ema.apply(params)                                   # (creates the averages)
        return params, grads, opt, ema

    pa, ga, oa, ea = build()
    pb, gb, ob, eb = build()
    step = ob.prepare(grads=gb, clip_norm=1.0, ema=eb)
    lr_t = 3e-4 * optimize.lr_correction(10, 0.9, 0.999)

    def per_tensor():
        _, scale = clip_by_global_norm(ga, clip_norm=1.0)
        for i, p in enumerate(pa):
            slot = oa.slots[i]
            adam_step(p, ga[i], slot["Mean"], slot["Var"], lr_t, norm_scale=scale, param16=slot["working"])
        for p in pa:
            ema_step(ea.average(p), p, 0.999)

    launches = (len(pa) + 1 + 2 * len(pa), 5)
    graphs = []
    for fn in (per_tensor, step.run):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fn()
        graphs.append(gr)
    out = [("eager",) + compare(torch, per_tensor, step.run, args.calls, args.windows, args.repeats),
           ("graph replay",) + compare(torch, graphs[0].replay, graphs[1].replay, args.calls, args.windows, args.repeats)]
    shape = "12 x [1024 x 1024 bsize-32 weight at 20 %% (%d blocks, bf16 gradient), bias 1024, 2 flat 1024], bf16 working copies" % blocks
    return shape, launches, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimize_list_bench.md"))
    ap.add_argument("--calls", type=int, default=200, help="calls per timing (at least 200)")
    ap.add_argument("--windows", type=int, default=5, help="timings per repeat (the repeat is their median)")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    args.calls = max(args.calls, 200)
    import torch
    assert torch.cuda.is_available(), "bench_optimize_list needs a ROCm device"
    from blocksparse_amd import _lib as lib
    fmt = lambda xs: " ".join("%.2f" % x for x in xs)
    ok_all = True
    shape1, stages = headline(torch, lib, args)
    out = ["# Tensor-list weight update: measured times (one MI355X)", "",
           "Written by `scripts/bench_optimize_list.py`.  Device events around %d back-to-back calls after a warm-up; a repeat is the median of %d"
           % (args.calls, args.windows),
           "such timings; %d repeats of each form, the two forms alternating in one process.  Noise = max - min of the per-tensor repeats." % args.repeats,
           "Eager calls: a time includes whatever the host adds when it cannot keep ahead of the device.", "",
           "## T = 1: the list kernels against the per-tensor kernels (C ABI)", "", shape1 + ".",
           "Accepted when the list median <= the per-tensor median + noise.", "",
           "| stage | per-tensor us (median) | list us (median) | noise us | list - per-tensor us | verdict | per-tensor repeats | list repeats |",
           "|---|---|---|---|---|---|---|---|"]
    for name, old, new in stages:
        mo, mn, noise, ok = verdict(old, new, False)
        ok_all &= ok
        out.append("| %s | %.2f | %.2f | %.2f | %+.2f | %s | %s | %s |" % (name, mo, mn, noise, mn - mo, "accepted" if ok else "NOT accepted", fmt(old), fmt(new)))
    shape2, launches, modes = model(torch, lib, args)
    out += ["", "## A 48-tensor model: clip + Adam + moving average", "", shape2 + ".",
            "Launches per step, from the arguments: %d per tensor (T sums of squares, 1 clip, T Adam, T averages) against %d (`step.run()`)." % launches,
            "Accepted when the list median < the per-tensor median - noise.", "",
            "| mode | per-tensor us (median) | list us (median) | noise us | per-tensor / list | verdict | per-tensor repeats | list repeats |",
            "|---|---|---|---|---|---|---|---|"]
    for name, old, new in modes:
        mo, mn, noise, ok = verdict(old, new, True)
        ok_all &= ok
        out.append("| %s | %.1f | %.1f | %.1f | %.2f | %s | %s | %s |" % (name, mo, mn, noise, mo / mn, "accepted" if ok else "NOT accepted", fmt(old), fmt(new)))
    out.append("")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out))
    print("\n".join(out))
    print("wrote " + args.out)
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
